// Time-averaged spectral diagnostics of the two-layer model, accumulated on the device.
//
// Restates pyqg 0.7.2 model.py::{_calc_diagnostics,_increment_diagnostics} and the diagnostic
// definitions of model.py / qg_model.py (KEspec, Ensspec, entspec, APEflux, KEflux, APEgenspec,
// KEfrictionspec, paramspec, paramspec_APEflux, paramspec_KEflux, Dissspec, ENSDissspec, ENSflux, ENSgenspec,
// ENSfrictionspec, ENSparamspec — the sixteen keys of comparison_tools.py:222-225), which the reference consumes in
// pyqg_generative/tools/comparison_tools.py:91,106,164-188 (paramspec_* at :174-176),222-247 and plots as
// calc_ispec(m, 0.5*ave_lev(KEspec)) (Google-Colab/online-simulations.ipynb cell 25).
// All spectra carry pyqg's 1/M^2 normalisation.  PARITY UNPINNED (pyqg is not available here):
// checked against oracle/qg_ref.py::_diag_functions only.
#include "common.hpp"
#include "diag_acc.hpp"
#include <cstdlib>

namespace qgx {

// xih_k = -wv2 * ph_k
__global__ void k_diag_xih(SpecDev d, const double2 *ph, double2 *xih) {
    const int sz = d.N * d.NK, b = blockIdx.y;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < 2 * sz; idx += gridDim.x * blockDim.x) {
        const size_t o = (size_t)b * 2 * sz + idx;
        const double w = -d.wv2[idx % sz];
        const double2 p = ph[o];
        xih[o] = make_double2(w * p.x, w * p.y);
    }
}

// real-space products: R3 = [ub*ptpc, vb*ptpc], R4 = [u1*xi1, v1*xi1], R5 = [u2*xi2, v2*xi2], R6 = [u1*q1, v1*q1],
// R7 = [u2*q2, v2*q2]
__global__ void k_diag_products(SpecDev d, DiagConst c, const double *u, const double *v, const double *p,
                                const double *xi, const double *q, double *R3, double *R4, double *R5, double *R6, double *R7) {
    const int rz = d.N * d.N, b = blockIdx.y;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < rz; idx += gridDim.x * blockDim.x) {
        const size_t o = (size_t)b * 2 * rz + idx;
        const double2 uv1 = make_double2(u[o], v[o]), uv2 = make_double2(u[o + rz], v[o + rz]);
        const double p1 = p[o], p2 = p[o + rz], x1 = xi[o], x2 = xi[o + rz], q1 = q[o], q2 = q[o + rz];
        const double2 r3 = diag_product_pair(0, c, 0., uv1, uv2, p1, p2), r4 = diag_product_pair(1, c, 0., uv1, uv2, x1, x2),
                      r5 = diag_product_pair(2, c, 0., uv1, uv2, x1, x2), r6 = diag_product_pair(4, c, 0., uv1, uv2, q1, q2),
                      r7 = diag_product_pair(5, c, 0., uv1, uv2, q1, q2);
        R3[o] = r3.x; R3[o + rz] = r3.y;
        R4[o] = r4.x; R4[o + rz] = r4.y;
        R5[o] = r5.x; R5[o + rz] = r5.y;
        R6[o] = r6.x; R6[o + rz] = r6.y;
        R7[o] = r7.x; R7[o + rz] = r7.y;
    }
}

__global__ void k_diag_accumulate(SpecDev d, DiagConst c, DiagCall x, DiagAcc a) {
    const int N = d.N, NK = d.NK, sz = N * NK, b = blockIdx.y;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < sz; idx += gridDim.x * blockDim.x) {
        const int j = idx / NK, i = idx - j * NK;
        diag_accumulate(d, c, a, b, idx, i, j, sz, [&] { return diag_elem_load(x, (size_t)b * 2 * sz + idx, sz); });
    }
}

__global__ void k_diag_scale_copy(const double *src, double *dst, size_t n, double s) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i] * s;
}
__global__ void k_diag_scale_S(const double *src, double *dst, size_t n, double w) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = w * src[i];
}

// dst = src - mean_{y,x} src for each (member, layer) plane of n values, one workgroup per plane
__global__ void k_diag_demean(const double *src, double *dst, int n) {
    __shared__ double red[256];
    const double *s = src + (size_t)blockIdx.x * n;
    double *o = dst + (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += s[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double mean = red[0] / n;
    for (int i = threadIdx.x; i < n; i += 256) o[i] = s[i] - mean;
}

static dim3 dgrid(const SpecDev &d, int n) { return dim3((unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256), d.B); }

static int dalloc0(double *&p, size_t n) {
    QGX_HIP(hipMalloc((void **)&p, n * sizeof(double)));
    QGX_HIP(hipMemset(p, 0, n * sizeof(double)));
    return QGX_OK;
}

int diag_ensure_alloc(qgx_model *m) {
    const SpecDev &d = m->d;
    const size_t nr = (size_t)d.B * 2 * d.N * d.N, ns2 = (size_t)d.B * 2 * d.N * d.NK * 2, n2d = (size_t)d.B * d.N * d.NK;
    int rc;
    if (!m->dg_R[0]) {
        for (int i = 0; i < 7; ++i) if ((rc = dalloc0(m->dg_R[i], nr))) return rc;
        for (int i = 0; i < 7; ++i) if ((rc = dalloc0(m->dg_S[i], ns2))) return rc;
        for (int i = 0; i < 2; ++i) if ((rc = dalloc0(m->dg_acc[i], ns2 / 2))) return rc;
        for (int i = 2; i < N_DIAGS; ++i) if ((rc = dalloc0(m->dg_acc[i], n2d))) return rc;
    }
    return QGX_OK;
}

static DiagConst diag_const(const qgx_model *m) {
    const SpecDev &d = m->d;
    DiagConst c;
    c.del1 = m->cfg.delta / (m->cfg.delta + 1.); c.del2 = 1. / (m->cfg.delta + 1.);
    c.rdm2 = pow(m->cfg.rd, -2.0); c.Udiff = m->cfg.U1 - m->cfg.U2; c.rek = m->cfg.rek;
    c.invM2 = d.invN2 * d.invN2; c.H0 = d.H[0] / d.Htot; c.H1 = d.H[1] / d.Htot;
    {   // the AB coefficients of the step this increment precedes (model.hip::model_step_once)
        double ab[3];
        ab3_coefficients(m->bk.ablevel, m->cfg.dt, ab);
        c.dt1 = ab[0]; c.dt2 = ab[1]; c.dt3 = ab[2];
        c.invdt = 1.0 / m->cfg.dt;
    }
    c.nu = m->visc_on ? m->visc_nu : nullptr;      // the viscous term is part of the parameterization's tendency
    c.nu_pv = m->visc_pv;
    return c;
}
static DiagAcc diag_acc(const qgx_model *m) {
    DiagAcc a;
    a.KEspec = m->dg_acc[0]; a.Ensspec = m->dg_acc[1]; a.entspec = m->dg_acc[2]; a.APEflux = m->dg_acc[3];
    a.KEflux = m->dg_acc[4]; a.APEgenspec = m->dg_acc[5]; a.KEfrictionspec = m->dg_acc[6]; a.paramspec = m->dg_acc[7];
    a.paramspec_APEflux = m->dg_acc[8]; a.paramspec_KEflux = m->dg_acc[9];
    a.Dissspec = m->dg_acc[10]; a.ENSDissspec = m->dg_acc[11]; a.ENSflux = m->dg_acc[12]; a.ENSgenspec = m->dg_acc[13];
    a.ENSfrictionspec = m->dg_acc[14]; a.ENSparamspec = m->dg_acc[15];
    return a;
}

int diag_increment(qgx_model *m, const double *S, double weight, int demean, hipStream_t st) {
    const SpecDev &d = m->d;
    const size_t nr = (size_t)d.B * 2 * d.N * d.N;
    int rc;
    if ((rc = diag_ensure_alloc(m))) return rc;
    if (S && demean) {
        // an external forcing that the step kernels de-mean (qgx_param::demean: they drop the (0, 0) element of its spectrum)
        // is the parameterization's tendency WITHOUT its layer means here too: pyqg's dqh is the transform of the de-meaned
        // field, and ENSparamspec's (0, 0) element is conj(qh) dqh there, not zero once q has a mean
        if (!m->dg_Sdm && (rc = dalloc0(m->dg_Sdm, nr))) return rc;
        hipLaunchKernelGGL(k_diag_demean, dim3(2 * d.B), dim3(256), 0, st, S, m->dg_Sdm, d.N * d.N);
        S = m->dg_Sdm;
    }
    double *R3 = m->dg_R[2], *R4 = m->dg_R[3], *R5 = m->dg_R[4], *R6 = m->dg_R[5], *R7 = m->dg_R[6];
    double2 *xih = (double2 *)m->dg_S[0];
    const DiagConst c = diag_const(m);
    const DiagAcc a = diag_acc(m);
    DiagCall x;
    x.qh = m->qh[m->bk.cur_q]; x.ph = m->ph; x.u = m->u; x.v = m->v; x.q = m->q;
    x.P = m->dg_R[0]; x.XI = m->dg_R[1];
    x.S3 = (double2 *)m->dg_S[1]; x.S4 = (double2 *)m->dg_S[2]; x.S5 = (double2 *)m->dg_S[3]; x.Sh = (double2 *)m->dg_S[4];
    x.S6 = (double2 *)m->dg_S[5]; x.S7 = (double2 *)m->dg_S[6];
    x.S = S; x.weight = weight;
    x.dq_p = m->dq[m->bk.i_new]; x.dq_pp = m->dq[m->bk.i_p];
    const auto accumulate = [&] {
        hipLaunchKernelGGL(k_diag_accumulate, dgrid(d, d.N * d.NK), dim3(256), 0, st, d, c, x, a);
        return hipGetLastError();
    };
    // the forcing's spectrum where no kernel of the path forms it: Sh = rfft2(weight S) (R3 is free at that point)
    const auto forcing_spectrum = [&](auto fwd) {
        if (!S) return (int)QGX_OK;
        hipLaunchKernelGGL(k_diag_scale_S, dim3(1024), dim3(256), 0, st, S, R3, nr, weight);
        return fwd(R3, x.Sh);
    };
    bool uv_stale = m->bk.uv_stale;       // a path that stores u, v clears it; one that stores psi alone sets or leaves it
    if (m->small && m->opts.diag_fused && (m->opts.diag_wide > 0 || (m->opts.diag_wide < 0 && 6 * d.B <= 256))) {
        // few members: the ten transforms as (member, transform) workgroups — two launches — then the accumulation kernel;
        // a single member's increment is three short kernels instead of a chain of ten transforms on one CU
        if ((rc = small_diag_transforms_wide(d, c, x, st))) return rc;
        QGX_HIP(accumulate());
        uv_stale = false;
    } else if (m->small && m->opts.diag_fused && m->opts.diag_reg && small_diag_increment_reg_ok(d)) {
        // grids up to 64 x 64: the same in ONE kernel whose work fields stay in registers (k_diag_small_reg: a quarter of the
        // bytes); it stores ph but no u, v — they are marked stale and inverted on demand
        // ... as two workgroups per member (chains of 7 and 5 transforms instead of one of 10) while both fit the device at once
        const bool halves = m->opts.diag_reg == 3 || (m->opts.diag_reg == 1 && 2 * d.B <= 256);
        if ((rc = small_diag_increment_reg(d, c, x, a, st, halves))) return rc;
        uv_stale = true;
    } else if (m->small && m->opts.diag_fused) {
        // small grids: the whole increment (inversion, ten packed transforms, products, accumulation) in ONE kernel, a
        // workgroup per member (spectral_small.hip::k_diag_small) instead of a dozen launches
        if ((rc = small_diag_increment(d, c, x, a, st))) return rc;
        uv_stale = false;
    } else if (!m->small && large_diag_fused_ok(m)) {
        // large grids at the specialised sizes: the increment's four packed fields through three fused launches
        // (spectral_large.hip); ph is stored, u and v are not (uv_stale stays as it is: they are inverted on demand)
        if ((rc = forcing_spectrum([&](const double *r, double2 *h) { return large_q_to_qh(m, r, h, st); }))) return rc;
        if ((rc = large_diag_fused(m, c, x, a, st))) return rc;
    } else {
        // one launch per transform.  _invert: ph, u, v of the current state
        rc = m->small ? small_invert(d, m->opts, x.qh, m->ph, m->u, m->v, st) : large_invert(m, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_diag_xih, dgrid(d, 2 * d.N * d.NK), dim3(256), 0, st, d, (const double2 *)m->ph, xih);
        auto inv = [&](const double2 *h, double *r) { return m->small ? small_qh_to_q(d, m->opts, h, r, st) : large_qh_to_q(m, h, r, st); };
        auto fwd = [&](const double *r, double2 *h) { return m->small ? small_q_to_qh(d, m->opts, r, h, st) : large_q_to_qh(m, r, h, st); };
        if ((rc = inv(m->ph, x.P)) || (rc = inv(xih, x.XI))) return rc;
        if (!m->small && (rc = large_ensure_q(m, st))) return rc;          // the lazy unparameterized path keeps no real-space q
        hipLaunchKernelGGL(k_diag_products, dgrid(d, d.N * d.N), dim3(256), 0, st, d, c, (const double *)m->u,
                           (const double *)m->v, (const double *)x.P, (const double *)x.XI, (const double *)m->q, R3, R4, R5, R6, R7);
        if ((rc = fwd(R3, x.S3)) || (rc = fwd(R4, x.S4)) || (rc = fwd(R5, x.S5)) || (rc = fwd(R6, x.S6)) || (rc = fwd(R7, x.S7))) return rc;
        if ((rc = forcing_spectrum(fwd))) return rc;
        QGX_HIP(accumulate());
    }
    m->bk.uv_stale = uv_stale;
    m->bk.dg_count += 1;
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

extern "C" int qgx_diag_config(qgx_model *m, int64_t start_step, int every) {
    QGX_NEEDS_STATE(m, "qgx_diag_config");
    QGX_REQUIRE(m, "qgx_diag_config: null model");
    m->dg_start = start_step;
    m->dg_every = every;
    return QGX_OK;
}

extern "C" int64_t qgx_diag_count(const qgx_model *m) { return m ? m->bk.dg_count : -1; }

extern "C" int qgx_diag_reset(qgx_model *m) {
    QGX_REQUIRE(m, "qgx_diag_reset: null model");
    m->bk.dg_count = 0;
    m->team_undo.before.dg_count = 0;      // (no settle here: a pending run's undo record must not bring the old count back)
    if (m->dg_acc[0]) {
        const size_t ns = (size_t)m->B * 2 * m->N * m->NK, n2 = (size_t)m->B * m->N * m->NK;
        for (int i = 0; i < N_DIAGS; ++i) QGX_HIP(hipMemset(m->dg_acc[i], 0, (i < 2 ? ns : n2) * sizeof(double)));
    }
    return QGX_OK;
}

extern "C" int qgx_diag_get(qgx_model *m, int diag, double *out_dev, void *stream) {
    QGX_NEEDS_STATE(m, "qgx_diag_get");
    QGX_REQUIRE(m && out_dev && diag >= 0 && diag < N_DIAGS, "qgx_diag_get: bad argument");
    QGX_REQUIRE(m->bk.dg_count > 0 && m->dg_acc[0], "qgx_diag_get: no diagnostics accumulated yet");
    const size_t n = (size_t)m->B * (diag < 2 ? 2 : 1) * m->N * m->NK;
    hipLaunchKernelGGL(k_diag_scale_copy, dim3(1024), dim3(256), 0, (hipStream_t)stream,
                       (const double *)m->dg_acc[diag], out_dev, n, 1.0 / (double)m->bk.dg_count);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
