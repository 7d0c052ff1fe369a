/*
 * qgx.h — C ABI of the MI355X (gfx950) online parameterized-QG ensemble engine.
 *
 * Drop-in boundary for ONE hot path of m2lines/pyqg_generative: the per-step work
 * that `pyqg_generative/tools/simulate.py:109-145` (run_simulation) drives through
 * `pyqg.QGModel.run_with_snapshots` and the `Parameterization.__call__` plugin
 * (`pyqg_generative/models/parameterization.py:23-34`).  Each entry point cites the
 * reference interface it replaces (paths relative to the reference repository;
 * "pyqg" = pyqg 0.7.2, the un-vendored spectral core the reference calls into).
 *
 * Conventions
 *   - every function returns 0 on success or a negative qgx_status; nothing throws
 *     across the ABI; qgx_last_error() gives a thread-local message.
 *   - all `*_dev` pointers are DEVICE pointers (e.g. torch tensor.data_ptr()),
 *     caller-owned and kept alive by the caller until `stream` is synchronised.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     No entry point on the step path synchronises the device.
 *   - ensemble-batched layouts, C order:
 *       real fields      (B, 2, N, N)      double   [member][layer][y][x]
 *       spectral fields  (B, 2, N, N/2+1)  complex double, interleaved (re,im),
 *                        l index ordered [0..N/2-1, -N/2..-1], k index [0..N/2]
 *       latent noise z   (B, 2, N, N)      float (GAN/VAE) or double (GZ)
 *   - one host thread per handle; handles are not thread-safe.
 */
#ifndef QGX_H
#define QGX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum qgx_status {
    QGX_OK = 0,
    QGX_ERR_INVALID = -1,     /* bad argument / unsupported size            */
    QGX_ERR_HIP = -2,         /* a HIP runtime call failed                   */
    QGX_ERR_STATE = -3,       /* call not valid in the handle's state        */
    QGX_ERR_NOMEM = -4
} qgx_status;

/* ---- model ------------------------------------------------------------------
 * Replaces pyqg.QGModel(**pyqg_params) as constructed at simulate.py:83,121 and
 * stochastic_pyqg.py:78-79.  Field names and defaults are pyqg's. */
typedef struct qgx_config {
    int32_t nx;          /* N = nx = ny; even, N = 2^a 3^b, 8 <= N <= 512             */
    int32_t n_members;   /* B: ensemble members resident on this device               */
    int32_t device;      /* HIP device ordinal                                        */
    int32_t plan_only;   /* != 0: the handle is an FFT plan of its grid for qgx_rfft2 / qgx_irfft2 only: tables and
                            work space, NO model state (every state entry point returns QGX_ERR_STATE)              */
    double  L;           /* domain size [m]                     (pyqg default 1e6)     */
    double  dt;          /* time step [s]                       (7200)                */
    double  rek;         /* bottom drag [1/s]                   (5.787e-7)            */
    double  delta;       /* H1/H2                               (0.25)                */
    double  beta;        /* [1/(m s)]                           (1.5e-11)             */
    double  rd;          /* deformation radius [m]              (15000)               */
    double  U1, U2;      /* background zonal flow [m/s]         (0.025, 0)            */
    double  H1;          /* upper layer thickness [m]           (500)                 */
    double  filterfac;   /* exponential filter strength         (23.6)                */
} qgx_config;

typedef struct qgx_model qgx_model;          /* opaque */
typedef struct qgx_generator qgx_generator;  /* opaque */

enum qgx_field {               /* pyqg attribute of the same name */
    QGX_F_Q = 0,      /* m.q      real      */
    QGX_F_QH = 1,     /* m.qh     spectral  */
    QGX_F_PH = 2,     /* m.ph     spectral (from the last inversion)            */
    QGX_F_U = 3,      /* m.u      real     (from the last inversion)            */
    QGX_F_V = 4,      /* m.v      real                                          */
    QGX_F_DQHDT = 5,  /* m.dqhdt     spectral (tendency of the last step)       */
    QGX_F_DQHDT_P = 6,
    QGX_F_DQHDT_PP = 7,
    QGX_F_S = 8,      /* real: subgrid forcing used by the last step (m.PV_forcing) */
    QGX_F_Z = 9,      /* latent noise held by the sampler (float or double)     */
    QGX_F_P = 10      /* m.p      real: irfft2(ph), pyqg's derived streamfunction (to_dataset 'p') */
};

enum qgx_table {               /* grid constants, (N, N/2+1) double unless noted */
    QGX_T_FILTR = 0,  /* m.filtr */
    QGX_T_WV2 = 1,    /* m.wv2   */
    QGX_T_A = 2,      /* m.a  (2,2,N,N/2+1) */
    QGX_T_KK = 3,     /* m.kk (N/2+1)       */
    QGX_T_LL = 4      /* m.ll (N)           */
};

int qgx_create(const qgx_config *cfg, qgx_model **out);
int qgx_destroy(qgx_model *m);

/* m.q = q  (kernel.pyx property q: also refreshes qh = rfft2(q)); call sites
 * simulate.py:131, operators.py:232; set_q1q2 at simulate.py:167. */
int qgx_set_q(qgx_model *m, const double *q_dev, void *stream);
/* m.qh = qh (also refreshes q = irfft2(qh)). */
int qgx_set_qh(qgx_model *m, const double *qh_dev, void *stream);
/* copy a state field into a caller buffer of the layout given above */
int qgx_get(qgx_model *m, int field, void *out_dev, void *stream);
/* copy a grid constant (host pointer, doubles) */
int qgx_get_table(qgx_model *m, int table, double *out_host);
/* bytes of a field for this model (so callers can size buffers) */
size_t qgx_field_bytes(const qgx_model *m, int field);

/* m._invert(): ph, u, v from qh (simulate.py:132,168; operators.py:233). */
int qgx_invert(qgx_model *m, void *stream);

/* ---- stepping ----------------------------------------------------------------
 * Replaces pyqg Model._step_forward driven by run_with_snapshots
 * (simulate.py:137) including the plugin call of parameterization.py:23-34 and
 * the samplers of stochastic_pyqg.py:30-72. */
/* QGX_SAMPLING_DETERMINISTIC (parameterization.py:27-28 -> predict_mean_snapshot, cgan_regression.py:164-171,
 * cvae_regression.py:138-145, mean_var_model.py:111-115): every step applies the de-meaned mean of `n_mean` generator
 * realisations for the current PV (GZ: the mean net alone, n_mean is not used).  Realisation j (0-based) of global member
 * `member_offset + b` at the t-th deterministic step of the handle draws the Philox stream
 * (seed, member, t + ((uint64_t)(j + 1) << 32)): the high word of the step is 0 on every AR1 / constant draw, so the streams
 * never collide with those.  The sampler state (the latent noise QGX_F_Z, the constant sampler's counter) is neither read
 * nor written; `nsteps` is ignored.  Refused with QGX_ERR_INVALID before anything is launched or changed: n_mean < 1 or
 * > 65536, z_external_dev, an OLS or ANN generator (the reference defines no predict_mean_snapshot for them), a grid the
 * nets do not take for the pseudo-batch launched (qgx_generator_forward_mean). */
enum qgx_sampling { QGX_SAMPLING_AR1 = 0, QGX_SAMPLING_CONSTANT = 1, QGX_SAMPLING_DETERMINISTIC = 2 };

typedef struct qgx_param {
    qgx_generator *gen;      /* NULL: use `forcing_dev` as S (or no forcing if that is NULL too) */
    int32_t  sampling;       /* qgx_sampling                                             */
    int32_t  nsteps;         /* decorrelation steps (AR1: <0 freezes the noise)          */
    double   weight;         /* `model_weight * parameterization` (simulate.py:242)      */
    uint64_t seed;           /* Philox key for on-device latent noise                    */
    uint64_t member_offset;  /* global id of member 0 on this device (multi-GPU shards)  */
    const void *z_external_dev; /* if non-NULL: white noise xi for THIS step, layout of z
                                   (parity tests); only honoured for nsteps_to_run == 1;
                                   refused (QGX_ERR_INVALID) with an OLS or ANN generator */
    const double *forcing_dev;  /* gen == NULL: externally supplied S (B,2,N,N), used as is
                                   (plain pyqg q_parameterization semantics)             */
    int32_t  demean;         /* subtract the per-layer spatial mean of S (parameterization.py:25) */
    int32_t  n_mean;         /* QGX_SAMPLING_DETERMINISTIC: realisations M averaged per step (reference: 100); not read otherwise */
} qgx_param;

/* advance `nsteps_to_run` steps; `p` may be NULL (unparameterized, simulate.py:121).
 * If `refresh_diag` != 0 the last step also stores ph,u,v (as pyqg keeps them).
 * 256 x 256 grids, p == NULL: the steps of a call that neither refresh ph,u,v nor have a diagnostics increment due
 * are executed by ONE persistent launch that occupies every CU of the device (state in registers, row/column exchange
 * in the XCDs' L2).  Such a run is a transaction: it writes only buffers that hold nothing live, and a flag raised inside
 * it (a bounded wait timed out because other work held CUs) is found by the NEXT call that touches the model, which restores
 * the bookkeeping of before the run, switches the kernel off for this model (qgx_run_kernel_state = -1) and replays the
 * steps with three launches each — the run degrades, the state is never undefined.  Issue such calls on one stream at a
 * time (a settle from another stream waits for the replay).
 * Two half-ensembles on two streams (qgx_step_streams): every exit joins both internal streams into `stream`; a call that
 * failed after one half had advanced marks the handle invalid — every later call returns QGX_ERR_STATE with the reason.
 * Option "split_adv" = 1 (default 0; small grids in the two-workgroups-per-member form, generator attached): the half of the
 * step kernel that needs nothing of the forcing runs as a kernel of its own on an internal side stream, forked from and
 * joined into `stream` inside every step; bit-identical, and measured slower on this stack. */
int qgx_step(qgx_model *m, int nsteps_to_run, const qgx_param *p, int refresh_diag, void *stream);
/* (QGX_SAMPLING_DETERMINISTIC never steps in halves: qgx_step_streams returns 1.) */
/* Small grids with a generator attached: an even ensemble may advance as two halves on two internal streams that fork from
 * and join `stream` inside the call (members are independent — the reference runs them as separate processes,
 * scripts/run_parameterized.py:55-63 — and the halves fill the idle phases of each other's launch chain); option "streams" of
 * qgx_set_option: 0 automatic (96 x 96 with 16 ... 64 members, where it measured +9 ... +20 %), 1 never, 2 whenever even.  Returns the number of streams (1 or 2)
 * qgx_step would use for this parameterization. */
int qgx_step_streams(const qgx_model *m, const qgx_param *p);
/* step counter / ablevel (m.tc) and reset of the AB history */
int64_t qgx_step_count(const qgx_model *m);
/* 256 x 256 grids: 1 after the census found the device fit for the single-launch runs of qgx_step, -1 if it did not
 * (or a run raised a flag), 0 before the first unparameterized step or on other grids */
int qgx_run_kernel_state(const qgx_model *m);
int qgx_reset_time(qgx_model *m);
/* Kernel-path switches of a model (no reference counterpart; cross-checks in tests/, A/B timing in bench_tools/):
 * every setting computes the same step, only the fusion / tiling differs.  "genfuse" (0|1: generator output and
 * next-input kernels folded into the small-grid step kernel), "diag_fused" (0|1: one-kernel diagnostics increment),
 * "diag_wide" (-1 auto|0|1: its transforms as (member, transform) workgroups),
 * "lsplit" (-1 auto|0|1: one workgroup per member and layer), "spec_threads" (0 auto|256|512|1024), "team" (0|1:
 * XCD-resident runs at 256 x 256), "team_min" (shortest such run), "large_fused", "large_lazy_q",
 * "large_specialised" (0|1: the large-grid kernel variants), "mean_chunk" (QGX_SAMPLING_DETERMINISTIC: pseudo-members
 * (member x realisation) per launch of the generator, the `chunk` of qgx_generator_forward_mean; 0 = automatic; a value
 * below the member count is refused by the step).  The library reads NO environment variable. */
int qgx_set_option(qgx_model *m, const char *name, int value);

/* Molecular viscosity: the Laplace(nu, PV) q-parameterization of the reference's third kind of online run
 * (--molecular_viscosity, tools/simulate.py:207-236), evaluated inside every step kernel as a term of the spectral
 * tendency:  pv != 0: dqh_k = -nu K^2 qh_k (nu lap q);  pv == 0: dqh_k = nu K^4 ph_k (nu lap zeta, zeta = lap psi).
 * nu_host: n_members doubles, one per member (a viscosity sweep is one ensemble), or NULL to switch the term off; an
 * all-zero array is "on, zero".  Copied into device memory the model owns, behind the work already on `stream` (the call
 * waits for it: the array is free on return).  A property of the handle, like rek: it is present in every later qgx_step
 * — p == NULL (256 x 256: such a model takes three launches per step, not the single-launch run kernel, whose registers
 * have no room for the term; qgx_run_kernel_state stays as it was), forcing_dev, a generator under any sampling, halves
 * on two streams — is untouched by weight and demean, counts as the parameterization's tendency in the diagnostics
 * (paramspec, paramspec_APEflux, paramspec_KEflux, ENSparamspec; the tendency of Dissspec / ENSDissspec), may be set
 * between steps (it takes effect at the next one) and leaves the AB history alone.  With the term off every result is
 * bitwise what it was without this entry point.  Refused before any device call and with the previous setting still in
 * force: a plan_only handle (QGX_ERR_STATE), a non-finite or negative nu (QGX_ERR_INVALID). */
int qgx_set_viscosity(qgx_model *m, const double *nu_host, int pv, void *stream);
/* nu_host (n_members doubles) and *pv as set; off: zeros and *pv = 0.  Returns the number of members the term is on for
 * (n_members, or 0 when it is off — which an all-zero array alone would not tell), or a negative qgx_status. */
int qgx_get_viscosity(const qgx_model *m, double *nu_host, int *pv);

/* The Jansen-Held backscatter closure, pyqg 0.7.2 parameterizations.py::BackscatterBiharmonic(smag_constant, back_constant,
 * eps) — the reference's physical parameterizations (models/physical_parameterizations.py: BackscatterEddy =
 * (sqrt(0.007), 1.2), BackscatterJet = (sqrt(0.005), 0.8), run by tools/simulate.py:243-244) — evaluated on the device from
 * the current qh:  dq = D - C_B R lap lap psi,  D = -lap(lap lap psi dx^2 nu_Smagorinsky(C_S)),  R = sum_k H_k <psi_k D_k> /
 * (sum_k H_k <psi_k lap lap psi_k> + eps), one R per member.  smag_host, back_host: n_members doubles each (a (C_S, C_B)
 * sweep is one ensemble); smag_host == NULL switches the closure off.  A property of the handle: while it is on, every
 * step of qgx_step with p == NULL recomputes S (QGX_F_S) from the state and steps with it (weight 1, no de-mean; 256 x 256:
 * three launches per step, qgx_run_kernel_state stays as it was); it counts as the parameterization's tendency in the
 * diagnostics and composes with qgx_set_viscosity.  A member's result is bitwise the same in any ensemble (fixed-order
 * reductions, no atomics).  With the closure off every result is bitwise what it was without this entry point.  Refused
 * before any launch and with the previous setting in force: a plan_only handle (QGX_ERR_STATE); a non-finite or negative
 * C_S, a non-finite C_B, eps < 0 (QGX_ERR_INVALID); qgx_step with a generator or forcing_dev while the closure is on
 * (pyqg has one q-parameterization slot). */
int qgx_set_backscatter(qgx_model *m, const double *smag_host, const double *back_host, double eps, void *stream);
/* the constants as set (off: zeros).  Returns the number of members the closure is on for (n_members or 0), or a
 * negative qgx_status. */
int qgx_get_backscatter(const qgx_model *m, double *smag_host, double *back_host, double *eps);
/* The closure of the current state into caller buffers: S_dev (n_members,2,N,N) doubles, ratio_dev (n_members) doubles
 * (R) or NULL.  Changes no state; the closure must be on. */
int qgx_backscatter_forcing(qgx_model *m, double *S_dev, double *ratio_dev, void *stream);

/* status reductions of pyqg's _print_status: out_dev[2*b+0] = KE, [2*b+1] = CFL (of ph,u,v as the last step stored
 * them; after steps with refresh_diag == 0 the current state is inverted first) */
int qgx_status_ke_cfl(qgx_model *m, double *out_dev, void *stream);

/* ---- time-averaged spectral diagnostics ------------------------------------------------
 * pyqg model.py::_calc_diagnostics / _increment_diagnostics; consumed by the reference in
 * tools/comparison_tools.py:91-188.  Accumulated inside qgx_step before every step with
 * tc >= start_step and tc % every == 0 (pyqg: t >= tavestart, tc % ceil(taveint/dt) == 0). */
enum qgx_diag {              /* per member; pyqg normalisation 1/M^2 */
    QGX_D_KESPEC = 0,        /* (B,2,N,N/2+1)  wv2 |ph|^2                         */
    QGX_D_ENSSPEC = 1,       /* (B,2,N,N/2+1)  |qh|^2                             */
    QGX_D_ENTSPEC = 2,       /* (B,N,N/2+1)    |del1 qh1 + del2 qh2|^2            */
    QGX_D_APEFLUX = 3,       /* (B,N,N/2+1)                                       */
    QGX_D_KEFLUX = 4,
    QGX_D_APEGENSPEC = 5,
    QGX_D_KEFRICTIONSPEC = 6,
    QGX_D_PARAMSPEC = 7,
    QGX_D_PARAMSPEC_APEFLUX = 8,   /* the APE and KE parts of paramspec (comparison_tools.py:174-176) */
    QGX_D_PARAMSPEC_KEFLUX = 9,
    /* (B,N,N/2+1) each: the filter's dissipation of energy / barotropic enstrophy and the barotropic-enstrophy budget
     * (flux, generation, bottom friction, parameterization) — the remaining keys of comparison_tools.py:222-225,365-368 */
    QGX_D_DISSSPEC = 10,
    QGX_D_ENSDISSSPEC = 11,
    QGX_D_ENSFLUX = 12,
    QGX_D_ENSGENSPEC = 13,
    QGX_D_ENSFRICTIONSPEC = 14,
    QGX_D_ENSPARAMSPEC = 15
};
int qgx_diag_config(qgx_model *m, int64_t start_step, int every);   /* every <= 0 disables */
int qgx_diag_get(qgx_model *m, int diag, double *out_dev, void *stream);   /* time mean */
int64_t qgx_diag_count(const qgx_model *m);
int qgx_diag_reset(qgx_model *m);

/* ---- generator ---------------------------------------------------------------
 * Replaces AndrewCNN inference through apply_function (cnn_tools.py:125-176,
 * 702-735) for CGANRegression.G / CVAERegression.decoder / MeanVarModel nets / OLSModel.net. */
enum qgx_gen_kind { QGX_GEN_GAN = 0, QGX_GEN_VAE = 1, QGX_GEN_GZ = 2, QGX_GEN_OLS = 3 };

typedef struct qgx_cnn_weights {      /* host pointers, float32, PyTorch layouts */
    int32_t n_in, n_out;              /* 4/2; 2, or 4: a flux-form net (see below)   */
    const float *conv_w[8];           /* (cout, cin, k, k)                           */
    const float *conv_b[8];           /* (cout)                                      */
    const float *bn_gamma[7], *bn_beta[7], *bn_mean[7], *bn_var[7];
    float bn_eps;                     /* 1e-5                                        */
} qgx_cnn_weights;

/* nets: GAN / VAE — the generator / decoder (n_in 4), optionally followed by the regression net `net_mean` (n_in 2) of a
 * model trained with regression != 'None' (cgan_regression.py:59-60, cvae_regression.py:49-50): n_nets 1 or 2;
 * GZ — net_mean, net_var (n_in 2): n_nets 2 (mean_var_model.py:82-100);
 * OLS — the deterministic AndrewCNN(2, 2) `net` of OLSModel (ols_model.py:29-31), S = y_std * net(q/x_std) (:68-75): n_nets 1,
 * n_in 2.  It takes no latent noise: qgx_generator_forward ignores z (NULL allowed), qgx_step draws none and writes no z,
 * and refuses z_external_dev; the sampler still decides when the forcing is recomputed (generate_latent_noise returns 0,
 * parameterization.py:23-34).
 * n_out = 4 marks a flux-form net, AndrewCNN(n_in, 2, div=True) (cnn_tools.py:100-123, 139-142, 170-175): conv_w[7] is
 * (4, 32, 3, 3), the last convolution writes the x-fluxes of both layers, then the y-fluxes, and the net's output is
 * (B, 2, N, N) = 10000 * divergence(fluxes), spectral, in float32, with the grid lines of pyqg.QGModel(nx = N) at pyqg's
 * default L = 1e6 as complex64 — NOT the online model's L — evaluated by one LDS-resident FFT kernel behind the last
 * convolution.  Every net of a GAN, VAE or OLS handle is 2 or 4 on its own (the regression net independently of net 0);
 * GZ takes 2 only.  Such a net's output integrates to zero over the domain before any de-mean.
 * Any other n_nets, n_in or n_out is refused (QGX_ERR_INVALID) before any allocation.
 * Grid sizes: the AndrewCNN kernels of such a handle run N = 16, 32, 48, 64, 96 and 128 (every member count).  The
 * other sizes qgx_create admits have no whole number of the kernels' row tiles (8, 12, 24 and every size that divides
 * neither 256 nor 384) or a 5x5-layer patch beyond the LDS (192, 256, 384).  qgx_generator_forward, qgx_cnn_forward and
 * qgx_step refuse them with QGX_ERR_INVALID and a message naming N BEFORE anything is launched or changed: after a refused qgx_step the model (step count, state, latent noise, sampler) is bitwise where it was and
 * the generator handle stays usable (tests/test_gpu_grid_sizes.py records the admitted set;
 * qgx_generator_size_ok asks without running anything, for the options in force: with "chunk" = 16 the patch fits at 192
 * and 256 as well, sizes no test runs the nets at). */
int qgx_generator_create(int kind, const qgx_cnn_weights *nets, int n_nets,
                         const float x_std[2], const float y_std[2], int device,
                         qgx_generator **out);
int qgx_generator_destroy(qgx_generator *g);

/* AndrewCNN nets of any architecture (other hidden_channels, no BatchNorm, no bias): the descriptor qgx_cnn_arch and the entry
 * point that takes it are declared and documented in qgx_arch.h, which this header includes. */
#include "qgx_arch.h"

/* QGX_OK if the kernels of the handle's nets (inet >= 0: of that net alone; -1: of all of them) run B members at N x N
 * under the options in force, else QGX_ERR_INVALID with the message the three entry points above give.  No device call. */
int qgx_generator_size_ok(const qgx_generator *g, int inet, int B, int N);

/* The DeepInversion U-Net generator of CGANRegression(generator='DeepInversion') (cgan_regression.py:50-53): the
 * DeepInversionGenerator(4, 2) of tools/deep_inversion.py:44-94, blocks res_unit / down / up at :104-160, as the forecast
 * sweep runs it (scripts/run_forecasting.py:25, 'CGANRegression-Unet').  Host pointers, float32, PyTorch layouts.
 * A residual unit computes conv(bn(x)) + conv1(bn(x)), conv = LeakyReLU(0.2) -> conv_a 3x3 -> bn2 -> LeakyReLU(0.2) -> conv_b 3x3,
 * conv1 = skip 1x1; state-dict keys <unit>.conv.1 (conv_a), .conv.2 (bn2), .conv.4 (conv_b), .conv1 (skip), .bn (bn). */
typedef struct qgx_unet_res {
    const float *bn_gamma, *bn_beta, *bn_mean, *bn_var;       /* bn (C_in): NULL for the bn='None' units 0 and 10    */
    const float *conv_a_w, *conv_a_b;                         /* (C_out, C_in, 3, 3), (C_out)                        */
    const float *bn2_gamma, *bn2_beta, *bn2_mean, *bn2_var;   /* (C_out): NULL for the bn='None' units              */
    const float *conv_b_w, *conv_b_b;                         /* (C_out, C_out, 3, 3), (C_out)                       */
    const float *skip_w, *skip_b;                             /* (C_out, C_in, 1, 1), (C_out)                        */
} qgx_unet_res;

typedef struct qgx_unet_weights {
    const float *conv32_w, *conv32_b;   /* conv32: (32, 4, 3, 3), (32)                                               */
    /* res32_start (32 -> 32, bn='None'), down64, down128, down256, down512 (each after AvgPool2d(2, 2): 32 -> 64 -> ...
     * -> 512), res512 (512 -> 512), up512, up256, up128, up64 (each on cat((upsampled, skip), dim=1): 512 -> 256 -> ...
     * -> 32), res32_end (32 -> 32, bn='None') */
    qgx_unet_res res[11];
    const float *up_w[4], *up_b[4];     /* up512 .. up64 .upsampling: ConvTranspose2d(C, C/2, 2, 2): (C, C/2, 2, 2), (C/2) */
    const float *conv_end_w, *conv_end_b;   /* conv_end: (2, 32, 1, 1), (2)                                              */
    float bn_eps;                       /* 1e-5                                                                       */
} qgx_unet_weights;

/* A GAN-kind handle whose generator is the U-Net (exact-f32 matrix-core kernels, unet.hip); net_mean: the AndrewCNN(2, 2)
 * regression net of regression != 'None' (cgan_regression.py:59-60) or NULL; it may be flux-form (n_out = 4, div=True) while
 * the U-Net is not.  S = y_std * (U-Net([q/x_std, z]) + net_mean(q/x_std)).
 * The handle serves qgx_generator_forward, qgx_step (gen), qgx_cnn_forward (inet 0: the U-Net, inet 1: net_mean),
 * qgx_generator_range_read and qgx_generator_info (precision 0).  N must be 32, 48, 64, 96 or 128 (QGX_ERR_INVALID before
 * any launch otherwise).  The AndrewCNN-only options and queries (qgx_generator_set_option with anything but precision 0,
 * _wino_info, _wino_info_n, _layer2_kernel, _profile, _profile_read) return QGX_ERR_INVALID on it. */
int qgx_generator_create_unet(const qgx_unet_weights *g, const qgx_cnn_weights *net_mean, const float x_std[2],
                              const float y_std[2], int device, qgx_generator **out);

/* ANNModel (models/ann_model.py): the pointwise MLP of tools/cnn_tools.py:184-210 (ANN), applied at every grid point of every
 * layer of every member to the s x s PV stencil around it (wrapped), one net shared by both layers.  Feature dy*s + dx is
 * float32(q) at offset (dy - s/2, dx - s/2) divided by x_scale (xarray_to_stencil, cnn_tools.py:321-339); the net is
 * Linear(s*s, h0) -> ReLU -> ... -> Linear(h_last, 1) in float32, with scale_invariant y = |x|^2 layers(x / |x|) (degree 2);
 * S = double(float32(y_scale * y)) (ann_model.py:82-93).  A zero stencil under scale_invariant gives NaN, as in torch.
 * Its kind is QGX_GEN_ANN; qgx_generator_create refuses it.  The handle serves qgx_generator_forward (z unused, may be NULL),
 * qgx_step (no latent noise, as OLS: no draw, no write to z, z_external_dev refused), qgx_cnn_forward (inet 0: the raw net on
 * (B, 1, N, N) normalised float images -> (B, 1, N, N)), qgx_generator_info (precision 0) and qgx_generator_range_read, on
 * any N up to 512.  The AndrewCNN-only options and queries return QGX_ERR_INVALID on it, as on the U-Net handle.
 * Shapes are checked before any HIP call: odd stencil_size 1 ... 7, 1 ... 4 hidden layers of width 1 ... 128. */
enum qgx_gen_kind_ann { QGX_GEN_ANN = 4 };

typedef struct qgx_ann_weights {      /* host pointers, float32, PyTorch layouts (state-dict keys layers.{2l}.weight / bias) */
    int32_t stencil_size;             /* s                                                          */
    int32_t n_hidden;                 /* hidden layers                                              */
    int32_t hidden[4];                /* their widths                                               */
    int32_t scale_invariant;          /* != 0: ANN(degree = 2)                                      */
    const float *w[5];                /* linear layer l = 0 .. n_hidden: weight (out, in)           */
    const float *b[5];                /*                                  bias (out)                */
} qgx_ann_weights;

int qgx_generator_create_ann(const qgx_ann_weights *w, float x_scale, float y_scale, int device, qgx_generator **out);
/* S = y_std * G([q/x_std, z]) — with a regression net S = y_std * (G([q/x_std, z]) + net_mean(q/x_std)), summed in
 * float32 — (cgan_regression.py:157-162; cvae_regression.py:131-136; mean_var_model.py:105-109); OLS: S = y_std * net(q/x_std)
 * (ols_model.py:68-75); ANN: S = y_scale * net(stencil(q) / x_scale) (ann_model.py:82-93).  demean != 0 also applies
 * parameterization.py:25.
 * z is float for GAN/VAE, double for GZ, unused (may be NULL) for OLS and ANN. */
int qgx_generator_forward(qgx_generator *g, const double *q_dev, const void *z_dev,
                          double *S_dev, int B, int N, int demean, void *stream);
/* The forcing of predict_mean_snapshot for each of B members (cgan_regression.py:164-171, cvae_regression.py:138-145,
 * mean_var_model.py:111-115): S (B,2,N,N) = y_std * (mean_j G([q/x_std, xi_j]) [+ net_mean(q/x_std)]) over M realisations,
 * the mean accumulated in float64 in realisation order, rounded to float32, summed with the regression net's output and
 * scaled in float32; demean != 0 also applies parameterization.py:25.  xi_j of member b is the Philox stream
 * (seed, member_offset + b, step + ((uint64_t)(j + 1) << 32)), drawn inside the input kernel.  Realisations are evaluated
 * as pseudo-members p = b * R + r of one batched forward, R per launch with B * R <= chunk (0 = automatic: 256; the last
 * launch takes the remainder); the regression net is evaluated once on the B inputs.  Results are bitwise repeatable and
 * depend on `chunk` only through the kernels a pseudo-batch of that size takes.  GZ: S = y_std * net_mean(q/x_std), no
 * draws, net_var is not evaluated, M is not used beyond its check.  OLS / ANN: QGX_ERR_INVALID.
 * Checked before any HIP call (QGX_ERR_INVALID): null pointers, B < 1, M < 1, M > 65536, step >= 2^32, 0 < chunk < B,
 * a grid the nets do not take for the pseudo-batches launched. */
int qgx_generator_forward_mean(qgx_generator *g, const double *q_dev, double *S_dev, int B, int N, int M, int chunk,
                               int demean, uint64_t seed, uint64_t member_offset, uint64_t step, void *stream);
/* raw CNN forward of net `inet`: x (B,n_in,N,N) float -> y (B,2,N,N) float — also for a flux-form net (n_out = 4), whose
 * four fluxes stay in the handle's workspace and whose y is 10000 * their divergence; the ANN: (B,1,N,N) -> (B,1,N,N)
 * (AndrewCNN.forward in eval mode; used by predict_mean_snapshot / offline sampling) */
int qgx_cnn_forward(qgx_generator *g, int inet, const float *x_dev, float *y_dev,
                    int B, int N, void *stream);

/* ---- coarse-graining / re-gridding building blocks ----------------------------------------
 * The reference's operators (tools/operators.py:84-99,117-217,241-268) are compositions of these.
 * A model handle doubles as the FFT plan of its grid: fields are (B,2,N,N) / (B,2,N,N/2+1). */
/* numpy-compatible rfft2 / irfft2 of the model's grid; does not touch the model state
 * (pyqg m.fft / m.ifft, operators.py:244-246). */
int qgx_rfft2(qgx_model *m, const double *x_dev, double *xh_dev, void *stream);
int qgx_irfft2(qgx_model *m, const double *xh_dev, double *x_dev, void *stream);
/* dst (nfields,N,N/2+1) <- scale * filter * [resolved block of src (nfields,n,n/2+1)]: the mode
 * transfer of cut_off (operators.py:123-130) and fft_interpolate (:148-189); zero_src_2h zeroes
 * src[h,0] first, zero_dst_2h zeroes dst[h,0] and dst[:,h] (h = min(n,N)/2); filter_dev is an
 * optional real (N,N/2+1) table on the destination grid (gauss_filter :87-90, model_filter :97-99). */
int qgx_spec_regrid(const double *src_dev, double *dst_dev, int nfields, int n, int N, double scale,
                    int zero_src_2h, int zero_dst_2h, const double *filter_dev, void *stream);
/* out = ik*A + il*B on an N-grid of domain size L (divergence, operators.py:241-247); A or B may be NULL */
int qgx_spec_div(const double *ah_dev, const double *bh_dev, double *out_dev, int nfields, int N,
                 double L, void *stream);
/* out = alpha * a * b + beta * c  (b, c optional): the pointwise products of advect (:258-266) */
int qgx_real_fma(const double *a_dev, const double *b_dev, double *out_dev, size_t n, double alpha,
                 const double *c_dev, double beta, void *stream);

/* sum += y, sumsq += y*y over Monte-Carlo samples (generate_mean_var, cgan_regression.py:139-146;
 * cvae_regression.py:120-126), accumulated in float64 */
int qgx_moments_accumulate(const float *y_dev, double *sum_dev, double *sumsq_dev, size_t n, void *stream);
/* kernel-variant switches for in-process A/B measurement (bench_tools/ab_conv.py): "precision" (0 exact f32 | 3 f16x3),
 * "chunk" (16|32 input channels staged per pass of k_conv), "v3" (-1 auto | 0 | 1 | 2: LDS-operand kernel k_conv3),
 * "last_valu" (0|1), "first_split" (1|2|4 output-channel slices of the first layer), and the tuning options of the
 * f16x3 path.  An unknown name is QGX_ERR_INVALID. */
int qgx_generator_set_option(qgx_generator *g, const char *name, int value);
/* f16x3 range guard (no reference counterpart: the reference evaluates its nets in plain float32).  The default
 * generator arithmetic carries float32 operands as f16 hi/lo pairs, which is float32-class only inside a value window;
 * qgx_generator_create calibrates each net (exact-f32 evaluation of calibration inputs) and picks the activation
 * pre-scale — or makes the exact-f32 kernels the default when the window cannot be met — and every kernel that stores
 * 16-bit activations raises a sticky flag when a value leaves the f16 range.
 * _range_read: synchronises `stream`, returns and clears the flags (bit l = layer l+1 overflowed, bit 31 = non-finite
 * forcing) and the largest |network input| seen since the last read (inputs beyond 65504, or NaN = inf, overflow too).
 * _info: what calibration decided (precision 0 | 3, log2 of the activation pre-scale, fold 0 | 1) and the calibration
 * maxima per layer (10 floats: [0..6] stored activations, [8] layer 1 before its BatchNorm). */
int qgx_generator_range_read(qgx_generator *g, unsigned *flags, float *input_absmax, void *stream);
int qgx_generator_info(const qgx_generator *g, int *precision, int *ascale_log2, int *fold, float *layer_absmax);
/* The 5x5 layer's 1-D Winograd form (conv_wino.hpp; 0.4 x the multiplications of the 25-tap form at 64 x 64): enabled for a
 * generator only if, at qgx_generator_create, its outputs on calibration inputs stayed within 1e-5 of the exact-f32 kernels'
 * (relative to the largest output).  -> whether it is in use, what calibration decided, and the error it measured. */
int qgx_generator_wino_info(const qgx_generator *g, int *enabled, int *chosen_by_calibration, float *calibration_error);
/* ... the same per grid size: the calibration is made at every size the kernels are specialised for (32, 48, 64, 96, 128 — the
 * tile shapes differ between them) and the form is admitted size by size; _wino_info reports the 64 x 64 entry.  Another N:
 * enabled = 0, error = inf.  (No reference counterpart; the arithmetic it guards is cnn_tools.py:79-98,125-176.) */
int qgx_generator_wino_info_n(const qgx_generator *g, int N, int *enabled, int *chosen_by_calibration, float *calibration_error);
/* Which kernel the 5x5 layer of net `inet` takes for B members at N x N under the options in force: 0 exact-f32 MFMA, 1 the
 * 25-tap f16x3 kernel, 2 its split-K form (tiny ensembles), 3 1-D Winograd (k_convw), 4 1-D Winograd with the input transform
 * under the MFMAs (k_convw2).  For measurement code (bench.py's roofline names the kernel it times). */
int qgx_generator_layer2_kernel(const qgx_generator *g, int inet, int B, int N, int *kernel);
/* Measurement hook (bench.py roofline leg; no reference counterpart): bracket every launch (every n-th: option "prof_every")
 * of conv layer `layer` (0..7, -1 = off) of every net with HIP events on the launch stream; _read synchronises those events,
 * returns their summed duration and the launch count, and clears the record. */
int qgx_generator_profile(qgx_generator *g, int layer);
int qgx_generator_profile_read(qgx_generator *g, double *total_ms, int64_t *launches);

/* ---- online metrics ------------------------------------------------------------
 * The exact 1-Wasserstein distance of two empirical distributions, scipy.stats.wasserstein_distance(u, v)
 * (comparison_tools.py:116-195 scores every distributional feature with it): with a the merged sorted sample,
 *     W1 = sum_k |i_k/n_u - j_k/n_v| * (a_{k+1} - a_k),   i_k, j_k = number of u, v values <= a_k.
 * Three steps, all on `stream`: qgx_w1_keys turns each sample into order-preserving unsigned keys (float64 value:
 * uint64 key; float32 identity feature: optionally uint32 key), qgx_w1_sorted sorts both key arrays (LSD radix sort,
 * 8-bit digits: histogram -> scan -> stable scatter) and sums the terms along the merge path.  The result is bitwise
 * the same on every call and for every permutation of either input (fixed partition, fixed reduction order, no float
 * atomics, no inter-workgroup waiting).  Sizes are 64-bit. */
enum qgx_w1_feature {
    QGX_W1_IDENTITY = 0,   /* x                                          (q, u, v)                       */
    QGX_W1_SUMSQ2 = 1,     /* x*x + y*y, in float64                      (KE = u^2 + v^2)                */
    QGX_W1_SQUARE = 2      /* x*x, in float64                            (Ens = curl(u, v)^2)            */
};
enum { QGX_W1_PARTIALS = 1024 };   /* per-block partial sums of qgx_w1_keys: the size of its scratch */

/* bytes of work space qgx_w1_sorted needs for nu and nv keys of key_bits (32 or 64) bits */
int qgx_w1_workspace(size_t nu, size_t nv, int key_bits, size_t *bytes);
/* keys of the feature selected by `feature` over a strided view: R x T rows of P contiguous values each, row (r, t)
 * starting at element r*stride_r + t*stride_t of x (and of y, same strides; y is used by QGX_W1_SUMSQ2 only) — for the
 * last T snapshots of layer z of an (R, T_all, 2, N, N) array pass x + (T_all-T)*stride_t + z*N*N, P = N*N,
 * stride_t = 2*N*N, stride_r = T_all*stride_t.  is_double: x, y are double (1) or float (0).  key_bits 32 only for a
 * float identity feature.  keys_dev: R*T*P keys.  partials_dev: scratch of 2 * QGX_W1_PARTIALS doubles (written in full, its contents before the
 * call are not read).
 * stats_dev (2 doubles, written): [0] = sum of feature^2 in a fixed order, [1] = number of NaN / +-inf feature values.
 * QGX_ERR_INVALID before any device call for an empty view, a bad is_double / feature / key_bits, or null pointers. */
int qgx_w1_keys(const void *x_dev, const void *y_dev, int is_double, int feature, int key_bits, int64_t R, int64_t T,
                int64_t P, int64_t stride_r, int64_t stride_t, void *keys_dev, double *partials_dev, double *stats_dev,
                void *stream);
/* W1 of the two samples whose keys qgx_w1_keys wrote: sorts both key arrays IN PLACE, then merges them; out_dev (one
 * double) <- W1, or NaN when stats_u[1] or stats_v[1] (may be NULL) count a non-finite value.  QGX_ERR_INVALID before any
 * device call for nu == 0, nv == 0, key_bits not 32 / 64, or work_bytes below qgx_w1_workspace(nu, nv, key_bits). */
int qgx_w1_sorted(void *keys_u_dev, size_t nu, const double *stats_u_dev, void *keys_v_dev, size_t nv,
                  const double *stats_v_dev, int key_bits, void *work_dev, size_t work_bytes, double *out_dev,
                  void *stream);
/* out = ik*vh - il*uh = spectral curl(u, v) = ddx(v) - ddy(u) on an N-grid of domain size L (pyqg_parameterization_benchmarks
 * FeatureExtractor 'curl(u,v)'); nfields (N, N/2+1) complex fields each */
int qgx_spec_curl(const double *uh_dev, const double *vh_dev, double *out_dev, int nfields, int N, double L,
                  void *stream);

/* ---- offline metrics -----------------------------------------------------------
 * The reductions behind Parameterization.test_offline (models/parameterization.py:36-168) and subgrid_scores /
 * PDF_histogram (tools/computational_tools.py:5-84) over (R, T, 2, N, N) snapshot arrays: truth T, Monte-Carlo mean M,
 * one sample G, streamfunction psi.  Every entry point returns QGX_ERR_INVALID before any device call for bad sizes,
 * empty views, null pointers or bad flags; indexing is 64-bit; results are bitwise the same on every call and on any
 * stream (fixed partitions, fixed-order merges, no float atomics).  Non-finite input gives NaN sums (spectra, moments)
 * and is counted by qgx_histogram. */
enum { QGX_OFFLINE_PLANES = 22,          /* (l, k) planes per time window of qgx_offline_spectra          */
       QGX_OFFLINE_SPEC_GROUPS = 32,     /* snapshot s is accumulated in group s % 32                      */
       QGX_HIST_MAX_BINS = 4096 };
enum qgx_offline_work { QGX_WORK_SPECTRA = 0, QGX_WORK_MOMENTS = 1, QGX_WORK_HISTOGRAM = 2 };
enum { QGX_HIST_STATS = 1,               /* first: mean and population std of the view (two passes)        */
       QGX_HIST_SCALE_STD = 2 };         /* divide by that std instead of `scale` (needs QGX_HIST_STATS)   */

/* bytes of device work space: SPECTRA the accumulator of qgx_offline_spectra for N (R, T, nbins unused), MOMENTS that of
 * qgx_offline_moments for (R, T, N), HISTOGRAM that of qgx_histogram for nbins */
int qgx_offline_workspace(int which, int64_t R, int64_t T, int64_t N, int nbins, size_t *bytes);
/* Adds S consecutive snapshots (global indices s0 .. s0+S-1, time index s % T) to the accumulator acc_dev
 * (QGX_OFFLINE_SPEC_GROUPS, 2, QGX_OFFLINE_PLANES, N, N/2+1) doubles; accumulate = 0 overwrites it (first call).
 * th, gh, mh, psih: rfft2 of T, G, M, psi, (S, 2, N, N/2+1) complex (psih may be NULL: its planes are 0).  With
 * X = rfft2(x)/N^2, R = T - M, GR = G - M, window w = (t >= t0), plane p of window w:
 *   p = f*2 + z        |X_f,z|^2                 f = T, G, M, R, GR
 *   p = 10 + f*2 + z   Re(conj(Psi_z) X_f,z)
 *   p = 20, 21         Re(conj(R_0) R_1), Re(conj(GR_0) GR_1) */
int qgx_offline_spectra(const double *th_dev, const double *gh_dev, const double *mh_dev, const double *psih_dev,
                        int64_t S, int N, int64_t s0, int64_t T, int64_t t0, int accumulate, double *acc_dev,
                        void *stream);
/* out_dev (2, QGX_OFFLINE_PLANES, N, N/2+1) <- sum over the groups of acc_dev, in group order */
int qgx_offline_spectra_finish(const double *acc_dev, int N, double *out_dev, void *stream);
/* Grouped sums of truth t, mean m, sample g over (R, T, 2, N, N) in two passes; dtypes bit 0 / 1 / 2: t / m / g are
 * double (else float).  out_dev, doubles, quantities q = [(t-m)^2, t^2, (t-t')^2, (m-m')^2, (t-t')(m-m'), (g-m)^2]
 * with t', m' the group means:
 *   spatial  (6, 2, N, N)   over (run, time)
 *   temporal (6, T, 2)      over (run, y, x)
 *   global   (6, 2)         over (run, time, y, x) */
int qgx_offline_moments(const void *t_dev, const void *m_dev, const void *g_dev, int dtypes, int64_t R, int64_t T, int N,
                        void *work_dev, size_t work_bytes, double *out_dev, void *stream);
/* np.histogram(x / scale, bins = nbins, range = (edges[0], edges[nbins])) in float64 over the view layer z, t >= t0 of an
 * (R, T, nlev, P) array; edges_dev: the np.linspace edges (nbins + 1 doubles).  counts_dev: nbins int64.  stats_dev (4
 * doubles): [0] mean, [1] population std (QGX_HIST_STATS only), [2] non-finite values in the view, [3] the scale used.
 * nbins = 0 with QGX_HIST_STATS computes the statistics only ([3]: the scale a count would have used; edges_dev and
 * counts_dev are not touched and may be NULL).  Without QGX_HIST_STATS [0] and [1] are not written. */
int qgx_histogram(const void *x_dev, int is_double, int64_t R, int64_t T, int64_t nlev, int64_t P, int64_t z, int64_t t0,
                  const double *edges_dev, int nbins, int flags, double scale, void *work_dev, size_t work_bytes,
                  int64_t *counts_dev, double *stats_dev, void *stream);

/* ---- flow statistics ---------------------------------------------------------
 * The derived fields omega, KE, Ens, Vabs and the plane sums of KE behind dataset_statistics / dataset_smart_read
 * (tools/comparison_tools.py:197-410): the two entry points are declared and documented in qgx_stats.h, which this header
 * includes. */
#include "qgx_stats.h"

/* ---- training ----------------------------------------------------------------
 * Training of ANNModel's stencil network on the device (models/ann_model.py:34-52 fit, tools/cnn_tools.py:645-700 train):
 * stencil rows, a fused loss / gradient kernel, Adam.  The trainer handle and its entry points are declared and documented
 * in qgx_train.h, which this header includes. */
#include "qgx_train.h"

/* Training of the convolutional nets (AndrewCNN: OLSModel.net and every net built from it): the circular convolution, its
 * data gradient and its weight gradient as stateless layer operations; autograd, BatchNorm and Adam stay with the caller
 * (tools/train_CNN.py).  Declared and documented in qgx_conv_train.h, which this header includes. */
#include "qgx_conv_train.h"

/* The two ends of such a net's training step: the gather of a batch from a planar data set into the engine layout, and the
 * loss head (MSE, or softplus then MSE: MeanVarModel's variance net) with its gradient and its planar outputs.  Declared and
 * documented in qgx_head_train.h, which this header includes. */
#include "qgx_head_train.h"

/* The flux head of a flux-form net (AndrewCNN(div=True)) as a differentiable operation: 10000 divergence(F) in the planar or
 * the engine layout, and its adjoint.  Declared and documented in qgx_flux_train.h, which this header includes. */
#include "qgx_flux_train.h"

/* The latent step of a conditional VAE's training (CVAERegression), between the encoder's last convolution and the decoder's
 * first: the reparameterised sample, the KL divergence with its variance diagnostics, and their gradient.  Declared and
 * documented in qgx_latent_train.h, which this header includes. */
#include "qgx_latent_train.h"

/* The layer of CGANRegression's discriminator (DCGAN_discriminator): Conv2d(cin, cout, 4, stride=2, padding=1, bias=False)
 * with zero padding, its data gradient and its weight gradient as stateless operations; each one's derivative is another of
 * the three, so tools/train_ops.py builds a twice-differentiable layer of them for the gradient penalty.  Declared and
 * documented in qgx_dconv_train.h, which this header includes. */
#include "qgx_dconv_train.h"

/* The layer of the DeepInversion U-Net generator's training (CGANRegression(generator='DeepInversion')): the circular 3 x 3 or
 * 1 x 1 convolution on any grid 2 ... 128 with up to 512 -> 1024 channels, its data gradient and its weight gradient as
 * stateless operations (tools/train_ops.py: unet_conv2d).  Declared and documented in qgx_uconv_train.h, which this header
 * includes. */
#include "qgx_uconv_train.h"

/* ---- latent noise ------------------------------------------------------------
 * z <- a z + b xi with xi ~ N(0,1) from Philox4x32-10 (stochastic_pyqg.py:43-49).  z: (B, n_per_member) float or double,
 * n_per_member a positive multiple of 4; a == 0 overwrites z (its previous contents are not read).  Counter of the four
 * normals at elements 4*quad .. 4*quad+3 of member b: (quad, step mod 2^32, (member_offset + b) mod 2^32, step >> 32),
 * key (seed mod 2^32, seed >> 32).  The global member id enters the counter MODULO 2^32 — here, in qgx_step (qgx_param::
 * member_offset) and in qgx_generator_forward_mean: ids that differ by a multiple of 2^32 draw the same stream, and a shard
 * whose ids pass 2^32 - 1 wraps to 0 (oracle/samplers_ref.py::philox_normal masks in the same way). */
int qgx_noise_normal(void *z_dev, int is_double, int B, int n_per_member, uint64_t seed,
                     uint64_t member_offset, uint64_t step, double a, double b, void *stream);

const char *qgx_last_error(void);
const char *qgx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QGX_H */
