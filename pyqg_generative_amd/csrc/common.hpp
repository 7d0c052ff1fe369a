// Shared host-side declarations of the qgx engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <string>
#include <memory>
#include <tuple>
#include "../../include/qgx.h"

namespace qgx {

void set_error(const char *fmt, ...);

#define QGX_HIP(call)                                                              \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            qgx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                           __FILE__, __LINE__);                                    \
            return QGX_ERR_HIP;                                                    \
        }                                                                          \
    } while (0)

#define QGX_REQUIRE(cond, ...)                                                     \
    do {                                                                           \
        if (!(cond)) {                                                             \
            qgx::set_error(__VA_ARGS__);                                           \
            return QGX_ERR_INVALID;                                                \
        }                                                                          \
    } while (0)

// entry points that touch the model state refuse a plan-only handle (qgx_config::plan_only)
#define QGX_NEEDS_STATE(m, what)                                                            \
    do {                                                                                   \
        if ((m) && (m)->plan_only) {                                                       \
            qgx::set_error("%s: the handle is an FFT plan only (created with plan_only), it has no model state", what); \
            return QGX_ERR_STATE;                                                          \
        }                                                                                  \
        if ((m) && !(m)->broken.empty()) {                                                 \
            qgx::set_error("%s: the model state is invalid: %s", what, (m)->broken.c_str()); \
            return QGX_ERR_STATE;                                                          \
        }                                                                                  \
    } while (0)

constexpr int MAX_RADIX_PASSES = 12;

// Kernel-path switches of a model (qgx_set_option).  They select between equivalent kernels of the product library
// (cross-checks in tests/, A/B timing in bench_tools/); none changes what is computed beyond rounding order.
struct ModelOpts {
    int genfuse = 1;             // small grids: generator output / next-input kernels folded into the step kernel
    int diag_fused = 1;          // small grids: one-kernel diagnostics increment (0: one launch per transform, diag.hip)
    int diag_reg = 1;            // small grids up to 64 x 64: the one-kernel increment with its work fields in registers (k_diag_small_reg):
                                 //   0 off | 1 on, as two workgroups per member while 2 B <= 256 | 2 always one workgroup per member | 3 always two
    int diag_wide = -1;          // small grids: the increment's transforms as (member, transform) workgroups, 3 launches
                                 //   (-1: while 6 B <= 256 | 0 | 1)
    int lsplit = -1;             // small grids: two workgroups per member, one per layer (-1 auto | 0 | 1)
    int spec_threads = 0;        // small grids: threads of the one-workgroup-per-member kernels (0 auto | 256 | 512 | 1024)
    int siblings = -1;           // small grids in layer-split form with a forcing: FOUR workgroups per member — the forcing's transform on a
                                 //   workgroup of its own beside the inversion / advection chain of its layer, joined by a flag in memory
                                 //   (-1: while 4 B <= 256, i.e. all of them resident at once: +2 ... +9 % of the online step | 0 | 1 |
                                 //   2: as 1, always with the cross-XCD publication — the path siblings on different XCDs take)
    int split_adv = 0;           // small grids in layer-split form + generator: the half of the step kernel that needs nothing of the forcing
                                 //   (inversion, advection, its transform) as a kernel of its own on a side stream, under the generator's
                                 //   layers (0 | 1).  Bit-identical and measured SLOWER almost everywhere (the two cross-stream
                                 //   dependencies per step cost more than the two transforms taken out of the chain: DESIGN.md section 3.1c),
                                 //   so it is off unless asked for
    int streams = 0;             // small grids + generator: the two halves of the ensemble on two internal streams (0 auto: 96 x 96, 16..64 even members | 1 never | 2 whenever even)
    int team = 1;                // 256 x 256: XCD-resident runs of unparameterized steps
    int team_min = 2;            //   shortest run handed to that kernel
    int team_fault = 0;          //   A/B library only: raise the run kernel's flag at the end of the next run (test hook)
    int step_fault = 0;          //   A/B library only: half-ensemble (1 | 2) of a two-stream qgx_step refuses its second chunk (test hook)
    int mean_chunk = 0;          // deterministic sampling: pseudo-members (member x realisation) per generator launch (0 auto: 256)
    int large_fused = 1;         // large grids: fused row / column kernels (0: one launch per pass and pointwise phase)
    int large_lazy_q = 1;        // large grids: unparameterized steps keep no real-space q
    int large_specialised = 1;   // large grids: compile-time-N kernels at 128 / 256; diagnostics also 512
};

// Tile-shape tuning aids read from the environment exist in the A/B library only (make ab); the product library
// always runs the measured defaults, so no environment variable can alter a production run.
static inline int tune_env(const char *name, int dflt) {
#ifdef QGX_AB
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// Device-visible description of one model's grid and constants (passed by value).
struct SpecDev {
    int N, NK, LD, B;
    int nrad;
    int rad[MAX_RADIX_PASSES];      // DIF pass radices, product = N
    const double *filtr, *wv2, *a;  // a: 4 tables of N*NK (a00,a01,a10,a11)
    const double *kk, *ll;
    const double2 *tw;              // tw[t] = exp(-2 pi i t / N)
    const int *pos;                 // pos[freq] -> position after the DIF passes
    double U[2], Qy[2];
    double rek, invN2, dt, dx;
    double H[2], Htot;
};

// Work the spectral step kernel does on the generator's behalf (small grids in layer-split form, GAN / VAE / OLS):
//  * y != null: the forcing is still the net's raw output (B,2,N,N) float; the kernel's prologue does what k_finish<FIN_PLAIN>
//    does — S = double(y * y_std) - mean_{y,x} — with the same arithmetic and summation order, and stores S;
//  * X != null: the kernel's epilogue assembles the NEXT step's network input from q^{n+1} and fresh white noise,
//    X = [float(q)/x_std, z], z = b * xi(Philox; seed, member, step) — what k_prep_noise does with a == 0;
//    no_noise (OLS): X = float(q)/x_std alone, (B, xc = 2, N, N) — what k_prep_input does with n_in = 2 (no Philox, no z).
struct GenFuse {
    const float *y = nullptr;
    const float *y1 = nullptr;      // regression net's output, summed with y in float32 before the scaling (k_finish<FIN_SUM>)
    float ys[2] = {1.f, 1.f};
    int demean = 0;
    unsigned *range = nullptr;      // the generator's range-guard words (generator.hpp)
    float *X = nullptr;
    float *z = nullptr;
    float xs[2] = {1.f, 1.f};
    int xc = 4;                     // channels of X per member: 4 ([q, z]) or 2 (OLS: q only)
    int no_noise = 0;               // OLS: no latent channels, z is not written
    float b = 1.f;
    uint64_t seed = 0, member_offset = 0, step = 0;
};

// Arguments of one time step (spectral_small.hip / spectral_large.hip).
struct StepArgs {
    const double2 *qh_in;   // (B,2,N,NK)
    double2 *qh_out;
    double *q;              // (B,2,N,N) in: q^n, out: q^{n+1}
    const double *S;        // (B,2,N,N) or null
    double2 *dqh;           // spectral forcing of this step (pyqg m.dqh)
    double2 *dq_new;        // newest tendency (overwrites the oldest history slot)
    const double2 *dq_p, *dq_pp;
    double2 *ph;            // diagnostics (written when diag != 0)
    double *u, *v;
    double dt1, dt2, dt3;
    double weight;
    int has_S, demean, diag;
    const double *nu = nullptr;     // molecular viscosity per member (qgx_set_viscosity), null = off; spectral_elem.hpp::visc_add
    int nu_pv = 0;                  //   != 0: nu lap q, else nu lap zeta
    GenFuse gf;
    // k_step_small PART 3 (forcing and advection workgroups of a (member, layer) in one launch): one word per (member, layer),
    // set to the launch's epoch by the forcing workgroup once the forcing's spectrum is in memory
    unsigned long long *sib_flag = nullptr;
    unsigned long long sib_epoch = 0;
    int sib_full = 0;           // publish across XCDs even to a sibling on the same one (option siblings = 2: exercises that path)
};

// time-averaged diagnostics (diag.hip; the small-grid increment is one kernel of spectral_small.hip)
struct DiagConst { double del1, del2, rdm2, Udiff, rek, invM2, H0, H1;
                   double dt1, dt2, dt3, invdt;          // AB coefficients of the step about to be taken (Dissspec)
                   const double *nu; int nu_pv; };       // molecular viscosity per member or null (StepArgs::nu): part of dqh
struct DiagAcc { double *KEspec, *Ensspec, *entspec, *APEflux, *KEflux, *APEgenspec, *KEfrictionspec, *paramspec,
                        *paramspec_APEflux, *paramspec_KEflux,
                        *Dissspec, *ENSDissspec, *ENSflux, *ENSgenspec, *ENSfrictionspec, *ENSparamspec; };
constexpr int N_DIAGS = 16;
// The pointers of one increment (diag.hip::diag_increment fills it; passed to the kernels by value).  Spectra are (B,2,N,NK),
// real fields (B,2,N,N).  DiagIn: what a caller brings — the state, the forcing and the tendencies — and all that
// k_diag_small_reg takes (it has no scalar register to spare for kernel arguments it does not read); the rest is written by
// the increment's own stages.
struct DiagIn {
    const double2 *qh; double2 *ph;                                      // state: qh in; ph out
    const double *S; double weight;                                      // forcing (null: none) and its weight
    const double *q;                                                     // state: q in
    const double2 *dq_p, *dq_pp;                                         // T_{n-1}, T_{n-2}
};
struct DiagCall : DiagIn {
    double *u, *v;                                                       // state, out where the path stores them
    double *P, *XI;                                                      // work fields: p = irfft2(psi), xi = irfft2(-K^2 psi)
    double2 *S3, *S4, *S5, *Sh, *S6, *S7;                                // spectra of the product pairs 0, 1, 2, 4, 5 and of the forcing (3)
};

// large grids (spectral_large.hip): complex work fields per member, of N rows at pitch N + large_zpad()
constexpr int ZF = 3;   // zbuf: layers 0,1 and one scratch (S / q pair)
constexpr int DZF = 4;  // dg_z: the fused diagnostics increment
int large_zpad();

// kernel.pyx::_forward_timestep: Euler, AB2, AB3 by start-up level
inline void ab3_coefficients(int level, double dt, double out[3]) {
    if (level == 0) { out[0] = dt; out[1] = 0.0; out[2] = 0.0; }
    else if (level == 1) { out[0] = 1.5 * dt; out[1] = -0.5 * dt; out[2] = 0.0; }
    else { out[0] = 23. / 12. * dt; out[1] = -16. / 12. * dt; out[2] = 5. / 12. * dt; }
}

// The stepping bookkeeping of a model: everything a step changes on the host.  It is saved, restored, compared and copied as
// a whole (the run kernel's undo record, the two half-ensembles of qgx_step), so a field added here is carried everywhere.
struct StepBook {
    int64_t tc = 0, const_counter = 0, dg_count = 0;
    int ablevel = 0, cur_q = 0;            // AB3 start-up level (0 Euler, 1 AB2, 2 AB3); qh[cur_q] is current
    int i_new = 0, i_p = 1, i_pp = 2, i_x = 3;   // roles of dq[]
    bool uv_stale = false;                 // the last step did not store ph, u, v (refresh_diag == 0): status inverts first
    bool q_stale = false;                  // large-N path: q lags qh (unparameterized steps keep no real-space q)
    bool z_double = false, have_noise = false, have_forcing = false;
    uint64_t noise_step = 0;
    const void *x_ready_gen = nullptr;     // the generator whose input the last step kernel assembled (GenFuse::X), or null
    uint64_t x_ready_step = 0;             //   ... for this noise step
    auto tie() const { return std::tie(tc, const_counter, dg_count, ablevel, cur_q, i_new, i_p, i_pp, i_x, uv_stale, q_stale,
                                       z_double, have_noise, have_forcing, noise_step, x_ready_gen, x_ready_step); }
    bool operator==(const StepBook &o) const { return tie() == o.tie(); }
};

}  // namespace qgx

struct qgx_generator;

struct qgx_model {
    qgx_config cfg;
    qgx::SpecDev d;
    qgx::ModelOpts opts;
    int N, NK, B;
    bool small;                     // whole member field fits one CU's LDS
    bool plan_only = false;         // FFT plan of the grid only: tables + work space, no model state (qgx_config::plan_only)
    // tables (device) + host copies for qgx_get_table
    double *t_filtr = nullptr, *t_wv2 = nullptr, *t_a = nullptr, *t_kk = nullptr, *t_ll = nullptr;
    double2 *t_tw = nullptr;
    int *t_pos = nullptr;
    // (behind one pointer: qgx_step copies the model's bookkeeping for its two half-ensembles on every call)
    struct HostTables { std::vector<double> filtr, wv2, a, kk, ll; };
    std::shared_ptr<HostTables> host;
    // a step that failed half-way (one half-ensemble advanced, the other not; a stream operation refused after the fork) leaves
    // device buffers and bookkeeping out of step: every later call on the handle fails loudly with this message
    std::string broken;
    qgx::StepBook bk;               // the stepping bookkeeping (a half-ensemble advances a copy; sib_epoch is not part of it)
    // state (device)
    double *q = nullptr, *u = nullptr, *v = nullptr, *S = nullptr;
    double2 *qh[2] = {nullptr, nullptr};   // ping-pong; qh[bk.cur_q] is current
    double2 *ph = nullptr, *dqh = nullptr; // dqh: spectral forcing of the last step (pyqg m.dqh)
    double2 *dq[4] = {nullptr, nullptr, nullptr, nullptr};   // AB3 tendency history; [3]: large grids, spare slot of the run kernel
    double2 *zbuf = nullptr;               // large-N path: (B,3,N,N) complex work array
    void *team_ctl = nullptr;              // large-N path: census / barrier block of the XCD-resident step kernel
    int team_state = 0;                    //   0 not probed, 1 available, -1 not available
    bool team_pending = false;             //   a run was launched whose flags have not been read back yet
    struct TeamUndo {                      //   the record as it was before the pending run (a run writes ONLY to buffers that hold
        int K = 0;                         //   nothing live, so a run that raised a flag is undone by restoring the record and
        qgx::StepBook before;              //   replayed on the three-launch path)
    } team_undo;
    hipStream_t team_stream = nullptr;     //   the stream the pending run was launched on (its flag is read back there)
    int team_replays = 0;                  //   runs that raised a flag and were replayed
    void *z = nullptr;                     // latent noise (B,2,N,N) float or double
    void *xi = nullptr;                    // scratch white noise for AR1
    // molecular viscosity (qgx_set_viscosity): one nu per member in device memory the model owns; a half-ensemble sees its slice
    double *visc_nu = nullptr;
    bool visc_on = false;
    int visc_pv = 0;
    std::shared_ptr<std::vector<double>> visc_host;
    // Jansen-Held backscatter closure (qgx_set_backscatter, backscatter.hip): C_S then C_B, one each per member, in device
    // memory the model owns; the work fields of the large-grid path (three spectral, three real)
    double *bs_const = nullptr;
    bool bs_on = false;
    double bs_eps = 0.0;
    std::shared_ptr<std::vector<double>> bs_host;
    double2 *bs_spec[3] = {nullptr, nullptr, nullptr};
    double *bs_real[3] = {nullptr, nullptr, nullptr};
    // time-averaged diagnostics (diag.hip)
    int64_t dg_start = 0;
    int dg_every = 0;
    double *dg_R[7] = {};
    double *dg_S[7] = {};
    double *dg_Sdm = nullptr;              // an external forcing less its layer means, where the step de-means it (diag_increment)
    double *dg_acc[qgx::N_DIAGS] = {};
    double2 *dg_z = nullptr;               // large grids: the four work fields of the three-launch increment (spectral_large.hip)
    // the two internal streams of a step in halves (model.hip::qgx_step) and their fork / join events
    // side stream and fork / join events of the two-kernel step (model.hip::step_core); a half-ensemble uses set adv_slot
    unsigned long long *sib_flag = nullptr;      // (B, 2) words of the four-workgroup step, and the epoch of its last launch
    unsigned long long sib_epoch = 0;
    hipStream_t adv_stream[2] = {nullptr, nullptr};
    hipEvent_t adv_event[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    int adv_slot = 0;
    bool is_half = false;                        // a half-ensemble view of a model stepped as two halves on two streams (model.hip::qgx_step)
    hipStream_t sub_stream[2] = {nullptr, nullptr};
    hipEvent_t sub_event[3] = {nullptr, nullptr, nullptr};
};

namespace qgx {
// THE list of the model's device buffers with a leading member axis: f(pointer, bytes per member) for each, null ones
// included.  qgx_step slices its half-ensembles with it and qgx_destroy frees what it yields: a new per-member buffer is
// added here and nowhere else.  The sizes are those of qgx_create, diag_ensure_alloc, diag_increment, large_diag_fused, backscatter_prepare,
// qgx_set_viscosity / _backscatter and step_sib_ensure.  z_elem: bytes of a latent-noise element in use (allocated: double).
template <class F>
void for_each_member_buffer(qgx_model &m, size_t z_elem, F &&f) {
    const size_t N = (size_t)m.N, NK = (size_t)m.NK;
    const size_t real = 2 * N * N * sizeof(double), spec = 2 * N * NK * sizeof(double2);
    const size_t zfield = (N + (size_t)large_zpad()) * N * sizeof(double2);
    f(m.q, real); f(m.u, real); f(m.v, real); f(m.S, real);
    f(m.qh[0], spec); f(m.qh[1], spec); f(m.ph, spec); f(m.dqh, spec);
    for (double2 *&p : m.dq) f(p, spec);
    f(m.z, 2 * N * N * z_elem); f(m.xi, 2 * N * N * z_elem);
    f(m.zbuf, ZF * zfield); f(m.dg_z, DZF * zfield);
    for (double *&p : m.dg_R) f(p, real);
    f(m.dg_Sdm, real);
    for (double *&p : m.dg_S) f(p, spec);                                           // (complex fields kept as doubles)
    for (int i = 0; i < N_DIAGS; ++i) f(m.dg_acc[i], (i < 2 ? 2 : 1) * N * NK * sizeof(double));
    f(m.visc_nu, sizeof(double));
    // two planes, C_S then C_B, of one double per member: backscatter_eval finds the second cfg.n_members further on
    f(m.bs_const, sizeof(double));
    for (double2 *&p : m.bs_spec) f(p, spec);
    for (double *&p : m.bs_real) f(p, real);
    f(m.sib_flag, 4 * sizeof(unsigned long long));      // the flag words and the placement words of a member
}

// model.py::_calc_diagnostics: t >= dt, t >= tavestart, tc % taveints == 0 — is an increment due before step t?
inline bool diag_due(const qgx_model *m, int64_t t) {
    return m->dg_every > 0 && t >= 1 && t >= m->dg_start && t % m->dg_every == 0;
}

// generator entry used by the stepper (generator.hip)
// optional sampler update z <- a z + b xi folded into the generator's input kernel
struct NoiseUpdate {
    const void *xi_ext;      // external draw or nullptr (Philox)
    uint64_t seed, member_offset, step;
    double a, b;
};
// defer != null (GAN / VAE): the output kernel is skipped and *defer describes what the step kernel has to do instead
// (GenFuse::y ...); input_ready: the previous step kernel already assembled the network input (GenFuse::X ...)
int generator_forward(qgx_generator *g, const double *q, const void *z, double *S, int B, int N,
                      int demean, hipStream_t st, const NoiseUpdate *nu, GenFuse *defer = nullptr, bool input_ready = false);
// Deterministic sampling (predict_mean_snapshot for every member): S = y_std * (mean of M realisations of net 0 [+ net_mean]),
// realisation j of member b on the Philox stream (seed, member_offset + b, step + ((j + 1) << 32)); GZ: the mean net alone.
// generator_mean_check: everything generator_forward_mean refuses apart from null pointers, with no HIP call (qgx_step asks
// it before it touches anything)
int generator_forward_mean(qgx_generator *g, const double *q, double *S, int B, int N, int M, int chunk, int demean,
                           uint64_t seed, uint64_t member_offset, uint64_t step, hipStream_t st);
int generator_mean_check(const qgx_generator *g, int B, int N, int M, int chunk, uint64_t step);
// QGX_OK if the handle's nets (inet >= 0: that net alone) run B members at N x N, else QGX_ERR_INVALID naming N; no HIP call
int generator_size_ok(const qgx_generator *g, int B, int N, int inet = -1);
// the generator's input buffer, input scales and range words for the GenFuse::X part (after reserve)
int generator_input_info(qgx_generator *g, int B, int N, GenFuse *gf);
bool small_layer_split(const SpecDev &d, const ModelOpts &o);
// spectral_small.hip
bool small_path_fits(int N);
int small_prepare(const SpecDev &d);
int small_step(const SpecDev &d, const ModelOpts &o, const StepArgs &a, hipStream_t st, int part = 0);
int small_q_to_qh(const SpecDev &d, const ModelOpts &o, const double *q, double2 *qh, hipStream_t st);
int small_qh_to_q(const SpecDev &d, const ModelOpts &o, const double2 *qh, double *q, hipStream_t st);
int small_invert(const SpecDev &d, const ModelOpts &o, const double2 *qh, double2 *ph, double *u, double *v, hipStream_t st);
// one diagnostics increment: in one kernel (k_diag_small) / with its work fields in registers (k_diag_small_reg; _ok: the grid
// has that kernel; halves: two workgroups per member) / its transforms as (member, transform) workgroups, k_diag_accumulate follows
int small_diag_increment(const SpecDev &d, const DiagConst &c, const DiagCall &x, const DiagAcc &a, hipStream_t st);
bool small_diag_increment_reg_ok(const SpecDev &d);
int small_diag_increment_reg(const SpecDev &d, const DiagConst &c, const DiagCall &x, const DiagAcc &a, hipStream_t st, bool halves);
int small_diag_transforms_wide(const SpecDev &d, const DiagConst &c, const DiagCall &x, hipStream_t st);
// spectral_large.hip
int large_prepare(const SpecDev &d);
int large_q_to_qh(qgx_model *m, const double *q, double2 *qh, hipStream_t st);
int large_qh_to_q(qgx_model *m, const double2 *qh, double *q, hipStream_t st);
int large_invert(qgx_model *m, hipStream_t st);
int large_step(qgx_model *m, const StepArgs &a, hipStream_t st);
int large_ensure_q(qgx_model *m, hipStream_t st);
bool large_diag_fused_ok(const qgx_model *m);
int large_diag_fused(qgx_model *m, const DiagConst &c, const DiagCall &x, const DiagAcc &acc, hipStream_t st);
int large_team_available(qgx_model *m, hipStream_t st);
int large_team_check(qgx_model *m, hipStream_t st, unsigned *flag);
int large_team_steps(qgx_model *m, int K, int ablevel0, const double coef[3][3], const double2 *qh_src, double2 *qh_dst,
                     const double2 *p_src, const double2 *pp_src, double2 *p_dst, double2 *pp_dst, hipStream_t st);

// backscatter.hip: kernel attributes / work fields of the closure; S (B,2,N,N) [and R (B)] of the state qh
int backscatter_prepare(qgx_model *m);
int backscatter_eval(qgx_model *m, const double2 *qh, double *S, double *ratio, hipStream_t st);

bool generator_noise_is_double(const qgx_generator *g);
bool generator_takes_noise(const qgx_generator *g);     // false for OLS and ANN: no latent noise at all
bool generator_reads_q(const qgx_generator *g);         // true for ANN: its kernel reads q itself, there is no input to assemble
int diag_increment(qgx_model *m, const double *S, double weight, int demean, hipStream_t st);
int diag_ensure_alloc(qgx_model *m);      // the increment's work fields and accumulators (allocated at first use)
// the generator's activation workspace for the calls that follow (1: the second half of an ensemble stepped in halves)
int generator_select_workspace(qgx_generator *g, int idx);
// unet.hip: the DeepInversion U-Net generator body (exact-f32 matrix-core kernels)
struct UNet;
int unet_create(const qgx_unet_weights *w, UNet **out);
void unet_destroy(UNet *u);
bool unet_size_ok(int N);                       // N = 32, 48, 64, 96, 128
size_t unet_workspace_floats(int B, int N);     // what unet_forward needs as `ws`
// x planar (B, 4, N, N) float -> y planar (B, 2, N, N) float
int unet_forward(const UNet *u, const float *x, float *y, float *ws, int B, int N, hipStream_t st);
// ann.hip: ANNModel's pointwise stencil network
struct Ann;
int ann_check(const qgx_ann_weights *w);         // the shape rules, no HIP call
int ann_create(const qgx_ann_weights *w, Ann **out);
void ann_destroy(Ann *a);
// q (n_img, N, N) double -> raw y (n_img, N, N) float, features float32(q) / x_scale; _x: already normalised float input
int ann_forward_q(const Ann *a, const double *q, float x_scale, float *y, int64_t n_img, int N, hipStream_t st);
int ann_forward_x(const Ann *a, const float *x, float *y, int64_t n_img, int N, hipStream_t st);
int noise_update(void *z, const void *xi_ext, bool is_double, int B, int n_per_member, uint64_t seed,
                 uint64_t member_offset, uint64_t step, double a, double b, hipStream_t st);
int noise_normal(void *z, bool is_double, int B, int n_per_member, uint64_t seed,
                 uint64_t member_offset, uint64_t step, double a, double b, hipStream_t st);
}  // namespace qgx
