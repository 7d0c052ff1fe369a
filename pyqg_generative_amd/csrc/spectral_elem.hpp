// Per-element formulas of the spectral step, written once: pure functions of values that the LDS-resident kernels
// (spectral_small.hip) and the multi-pass kernels (spectral_large.hip) both call, so that every path computes the
// same expression in the same order — tests assert torch.equal between paths.  No formula here may be regrouped:
// operand order decides which products the compiler contracts into an fma.
//
// Restates pyqg 0.7.2 kernel.pyx::{_invert,_do_advection,_do_friction,_forward_timestep} per spectral element.
#pragma once
#include "common.hpp"

namespace qgx {

__device__ __forceinline__ int neg_mod(int j, int N) { return j == 0 ? 0 : N - j; }

// psi_k = a[k][0] q_1 + a[k][1] q_2
__device__ __forceinline__ double2 invert_layer(double a0, double a1, double2 q0, double2 q1) {
    return make_double2(a0 * q0.x + a1 * q1.x, a0 * q0.y + a1 * q1.y);
}
// the same with the coefficients of element idx taken from the inversion table
__device__ __forceinline__ double2 invert_layer(const SpecDev &d, int k, int idx, double2 q0, double2 q1) {
    const int sz = d.N * d.NK;
    return invert_layer(d.a[(2 * k) * sz + idx], d.a[(2 * k + 1) * sz + idx], q0, q1);
}

// a self-conjugate column (i = 0, N/2) holds (a + conj(a at row -j)) / 2
__device__ __forceinline__ double2 herm_mean(double2 a, double2 am) { return make_double2(0.5 * (a.x + am.x), 0.5 * (a.y - am.y)); }

// uh = -i l ph ; vh = i k ph
__device__ __forceinline__ double2 u_hat(double l, double2 ph) { return make_double2(l * ph.y, -l * ph.x); }
__device__ __forceinline__ double2 v_hat(double k, double2 ph) { return make_double2(-k * ph.y, k * ph.x); }

// the full spectrum of the real pair packed as A + i B, from the half spectra: s (A + i B) at (j, i) and
// s (conj A + i conj B) at the mirror (-j, -i)
__device__ __forceinline__ double2 pack_self(double2 A, double2 B, double s) { return make_double2((A.x - B.y) * s, (A.y + B.x) * s); }
__device__ __forceinline__ double2 pack_mirror(double2 A, double2 B, double s) { return make_double2((A.x + B.y) * s, (B.x - A.y) * s); }

// the reverse: half spectra A = (X + conj C) / 2, B = -i (X - conj C) / 2 from the transformed pair at (j, i) (X) and at
// the mirror (C)
__device__ __forceinline__ void unpack_half(double2 X, double2 C, double2 &A, double2 &B) {
    A = make_double2(0.5 * (X.x + C.x), 0.5 * (X.y - C.y));
    B = make_double2(0.5 * (X.y + C.y), -0.5 * (X.x - C.x));
}

// -(ik uqh + il vqh + ik Qy ph), plus the bottom friction rek K^2 ph in layer 2.  K^2 and rek are read behind the k == 1
// test, which is why they arrive as a pointer and a reference: with rek read up front the two tests merge, and the
// k_step_small instances that loop over the layers come out restructured.
__device__ __forceinline__ double2 tendency_elem(int k, double kx, double ly, double Qy_k, const double &rek, const double *wv2_elem,
                                                 double2 uqh, double2 vqh, double2 ph) {
    const double kq = kx * Qy_k;
    double tx = (kx * uqh.y + ly * vqh.y + kq * ph.y);
    double ty = -(kx * uqh.x + ly * vqh.x + kq * ph.x);
    if (k == 1 && rek != 0.0) {
        const double f = rek * *wv2_elem;
        tx += f * ph.x;
        ty += f * ph.y;
    }
    return make_double2(tx, ty);
}

// Molecular viscosity, the Laplace(nu, PV) q-parameterization of pyqg_generative/tools/simulate.py:207-225, per spectral
// element: dqh_k = c src with  PV: c = -nu K^2, src = qh_k (nu lap q);  else: c = nu K^4, src = ph_k (nu lap zeta,
// zeta = lap psi, lap = (ik)^2 + (il)^2 = -K^2).  The coefficient is a chain of single products, so there is nothing for
// the compiler to contract differently from kernel to kernel.
__device__ __forceinline__ double visc_coef(double nu, int pv, double wv2) { return pv ? -(nu * wv2) : (nu * wv2) * wv2; }
// the term itself (diagnostics: the parameterization's tendency, pyqg's dqh)
__device__ __forceinline__ double2 visc_elem(double nu, int pv, double wv2, double2 qh_k, double2 ph_k) {
    const double c = visc_coef(nu, pv, wv2);
    const double2 s = pv ? qh_k : ph_k;
    return make_double2(c * s.x, c * s.y);
}
// the tendency with the term added (after tendency_elem and after the forcing): one explicit fused multiply-add per
// component, the same rounding in every kernel whatever surrounds the call
__device__ __forceinline__ double2 visc_add(double2 t, double nu, int pv, double wv2, double2 qh_k, double2 ph_k) {
    const double c = visc_coef(nu, pv, wv2);
    const double2 s = pv ? qh_k : ph_k;
    return make_double2(__builtin_fma(c, s.x, t.x), __builtin_fma(c, s.y, t.y));
}

// third-order Adams-Bashforth step of one element with the exponential filter f
__device__ __forceinline__ double2 ab3_filter(double f, double2 qk, double2 t, double2 p, double2 pp, double dt1, double dt2, double dt3) {
    return make_double2(f * (qk.x + dt1 * t.x + dt2 * p.x + dt3 * pp.x), f * (qk.y + dt1 * t.y + dt2 * p.y + dt3 * pp.y));
}

}  // namespace qgx
