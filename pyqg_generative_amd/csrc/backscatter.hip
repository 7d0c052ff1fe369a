// The Jansen-Held backscatter closure as a q-parameterization evaluated on the device for whole ensembles.
//
// Restates pyqg 0.7.2 parameterizations.py::{Smagorinsky.__call__(m, just_viscosity=True), BackscatterBiharmonic.__call__}
// (the reference's physical parameterizations: pyqg_generative/models/physical_parameterizations.py, run by
// tools/simulate.py:243-244 as model_weight * eval(name)()), behind _invert, per member with its own (C_S, C_B):
//
//   Sxx = ifft(ik uh), Sxy = ifft(il uh + ik vh) / 2, Syy = -Sxx        (uh = -il ph, vh = ik ph)
//   nu  = (C_S dx)^2 sqrt(2 (Sxx^2 + Syy^2 + 2 Sxy^2))
//   llp = ifft(K^4 ph),  g = llp dx^2 nu,  D = ifft(K^2 fft(g))
//   R   = sum_k H_k <psi_k D_k> / (sum_k H_k <psi_k llp_k> + eps)       both means by Parseval on the half spectrum
//   dqh = K^2 fft(g) - C_B R K^4 ph,  S = ifft(dqh)
//
// Five complex N x N transforms of packed pairs per member: (Sxx_1 + i Sxy_1), (Sxx_2 + i Sxy_2), (llp_1 + i llp_2)
// inverse, (g_1 + i g_2) forward, (S_1 + i S_2) inverse.  Small grids: one LDS-resident kernel, one workgroup per member;
// nu waits for llp in the member's slice of the OUTPUT array (every thread re-reads what it wrote itself).  Other grids:
// the model's batched transforms around three small kernels.  R is a fixed-order workgroup reduction with no atomics, by
// a workgroup of always 1024 threads: a member's result does not depend on the ensemble it is in.
#include "common.hpp"
#include "fft_lds.hpp"
#include "spectral_elem.hpp"
#include "spectral_pack.hpp"

namespace qgx {

struct BsArgs {
    const double2 *qh;              // (B,2,N,NK) current state
    const double *smag, *back;      // (B) C_S, C_B
    double eps;
    double *S;                      // (B,2,N,N) out
    double *ratio;                  // (B) out, or null
};

constexpr int BS_THREADS = 1024;

// ---- per-element formulas, shared by both paths
// Sxx^ = ik uh = k l ph ;  Sxy^ = (il uh + ik vh) / 2 = (l^2 - k^2) ph / 2
__device__ __forceinline__ double2 bs_sxx_hat(double kx, double ly, double2 ph) { const double c = kx * ly; return make_double2(c * ph.x, c * ph.y); }
__device__ __forceinline__ double2 bs_sxy_hat(double kx, double ly, double2 ph) {
    const double c = 0.5 * (ly * ly - kx * kx);
    return make_double2(c * ph.x, c * ph.y);
}
// (lap lap psi)^ = K^4 ph
__device__ __forceinline__ double2 bs_llp_hat(double wv2, double2 ph) { const double c = wv2 * wv2; return make_double2(c * ph.x, c * ph.y); }
// Smagorinsky viscosity with Syy = -Sxx, cs2 = (C_S dx)^2
__device__ __forceinline__ double bs_nu(double cs2, double sxx, double sxy) {
    return cs2 * sqrt(2.0 * (sxx * sxx + sxx * sxx + 2.0 * (sxy * sxy)));
}
// D^ = K^2 g^
__device__ __forceinline__ double2 bs_diss_hat(double wv2, double2 gh) { return make_double2(wv2 * gh.x, wv2 * gh.y); }
// this element's share of sum_k H_k sum_full Re(ph_k conj(X_k)), w = 1 on the self-conjugate columns, else 2
__device__ __forceinline__ double bs_share(double w, double H0, double H1, double2 p0, double2 x0, double2 p1, double2 x1) {
    return w * (H0 * (p0.x * x0.x + p0.y * x0.y) + H1 * (p1.x * x1.x + p1.y * x1.y));
}
__device__ __forceinline__ double2 bs_assemble(double2 Dh, double cbR, double2 Lh) { return make_double2(Dh.x - cbR * Lh.x, Dh.y - cbR * Lh.y); }

// sums of (num, den) over the workgroup in a fixed order: per-thread partial sums, wave shuffles, waves in order.
// Returns the energy ratio R to every thread.
__device__ __forceinline__ double bs_ratio(const SpecDev &d, double num, double den, double eps) {
    __shared__ double s_num[BS_THREADS / 64], s_den[BS_THREADS / 64];
    __shared__ double s_R;
    for (int o = 32; o > 0; o >>= 1) {
        num += __shfl_down(num, o);
        den += __shfl_down(den, o);
    }
    if ((threadIdx.x & 63) == 0) { s_num[threadIdx.x >> 6] = num; s_den[threadIdx.x >> 6] = den; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tn = 0.0, td = 0.0;
        for (int w = 0; w < BS_THREADS / 64; ++w) { tn += s_num[w]; td += s_den[w]; }
        const double s = d.invN2 * d.invN2;             // mean_xy(a b) = sum_full(ah conj(bh)) / N^4
        s_R = (tn * s) / (td * s + eps);
    }
    __syncthreads();
    return s_R;
}

// ------------------------------------------------------------------ small grids: the whole closure in one kernel
template <int NN>
__global__ __launch_bounds__(BS_THREADS) void k_backscatter_small(SpecDev d, BsArgs a) {
    double2 *Z = reinterpret_cast<double2 *>(qgx_smem);
    int *pos_lds;
    Grid g = make_grid(d, Z, pos_lds);
    if (NN) { g.N = NN; g.NK = NN / 2 + 1; g.LD = NN + 1; }
    const int N = NN ? NN : d.N, NK = NN ? NN / 2 + 1 : d.NK, LD = NN ? NN + 1 : d.LD, b = blockIdx.x;
    const size_t so = (size_t)b * 2 * N * NK, ro = (size_t)b * 2 * N * N;
    const int sz = N * NK, rz = N * N;
    const double2 *qh0 = a.qh + so, *qh1 = qh0 + sz;
    double *Sb = a.S + ro;
    const double cs = a.smag[b] * d.dx, cs2 = cs * cs, dx2 = d.dx * d.dx;
    __syncthreads();
    // ---- strain of layer k as the pair (Sxx_k + i Sxy_k); nu_k into the output array
    for (int k = 0; k < 2; ++k) {
        for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
            const int j = idx / NK, i = idx - j * NK;
            const double kx = d.kk[i];
            const double2 ph = invert_layer(d, k, idx, qh0[idx], qh1[idx]);
            double2 A = bs_sxx_hat(kx, d.ll[j], ph), Bv = bs_sxy_hat(kx, d.ll[j], ph);
            if (i == 0 || 2 * i == N) {
                const int jm = neg_mod(j, N), idm = jm * NK + i;
                const double2 pm = invert_layer(d, k, idm, qh0[idm], qh1[idm]);
                A = herm_mean(A, bs_sxx_hat(kx, d.ll[jm], pm));
                Bv = herm_mean(Bv, bs_sxy_hat(kx, d.ll[jm], pm));
            }
            pack_store(Z, g, j, i, A, Bv, d.invN2);
        }
        __syncthreads();
        fft2d_inv_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
        for (int idx = threadIdx.x; idx < rz; idx += BS_THREADS) {
            const int y = idx / N, x = idx - y * N;
            const double2 s = Z[y * LD + x];
            Sb[k * rz + idx] = bs_nu(cs2, s.x, s.y);
        }
        __syncthreads();
    }
    // ---- (llp_1 + i llp_2), then g = llp dx^2 nu in place
    for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
        const int j = idx / NK, i = idx - j * NK;
        const double w2 = d.wv2[idx];
        double2 A = bs_llp_hat(w2, invert_layer(d, 0, idx, qh0[idx], qh1[idx]));
        double2 Bv = bs_llp_hat(w2, invert_layer(d, 1, idx, qh0[idx], qh1[idx]));
        if (i == 0 || 2 * i == N) {
            const int idm = neg_mod(j, N) * NK + i;
            const double wm = d.wv2[idm];
            A = herm_mean(A, bs_llp_hat(wm, invert_layer(d, 0, idm, qh0[idm], qh1[idm])));
            Bv = herm_mean(Bv, bs_llp_hat(wm, invert_layer(d, 1, idm, qh0[idm], qh1[idm])));
        }
        pack_store(Z, g, j, i, A, Bv, d.invN2);
    }
    __syncthreads();
    fft2d_inv_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
    for (int idx = threadIdx.x; idx < rz; idx += BS_THREADS) {       // (the element -> thread map nu was stored under)
        const int y = idx / N, x = idx - y * N;
        const double2 w = Z[y * LD + x];
        Z[y * LD + x] = make_double2(w.x * dx2 * Sb[idx], w.y * dx2 * Sb[rz + idx]);
    }
    __syncthreads();
    fft2d_fwd_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
    // ---- the two sums of R over the half spectrum (D^ = K^2 g^ read out of the transformed field, which stays as it is)
    double num = 0.0, den = 0.0;
    for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
        const int j = idx / NK, i = idx - j * NK;
        const double w2 = d.wv2[idx];
        double2 g0, g1;
        unpack_pair(Z, g, j, i, g0, g1);
        const double2 p0 = invert_layer(d, 0, idx, qh0[idx], qh1[idx]), p1 = invert_layer(d, 1, idx, qh0[idx], qh1[idx]);
        const double w = (i == 0 || 2 * i == N) ? 1.0 : 2.0;
        num += bs_share(w, d.H[0], d.H[1], p0, bs_diss_hat(w2, g0), p1, bs_diss_hat(w2, g1));
        den += bs_share(w, d.H[0], d.H[1], p0, bs_llp_hat(w2, p0), p1, bs_llp_hat(w2, p1));
    }
    const double R = bs_ratio(d, num, den, a.eps);       // (its barriers stand between the reads above and the writes below)
    if (a.ratio && threadIdx.x == 0) a.ratio[b] = R;
    const double cbR = a.back[b] * R;
    // ---- dqh = D^ - C_B R K^4 ph as the pair (S_1 + i S_2), IN PLACE: the thread of element (j, i) reads and writes the
    // field at (j, i) and at its mirror (-j, -i) only.  On a self-conjugate column both are elements of the half spectrum:
    // the thread of the smaller row does both, the other one nothing
    for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
        const int j = idx / NK, i = idx - j * NK;
        const bool selfc = i == 0 || 2 * i == N;
        const int jm = neg_mod(j, N);
        if (selfc && jm < j) continue;
        const double w2 = d.wv2[idx];
        double2 g0, g1;
        unpack_pair(Z, g, j, i, g0, g1);
        double2 s0 = bs_assemble(bs_diss_hat(w2, g0), cbR, bs_llp_hat(w2, invert_layer(d, 0, idx, qh0[idx], qh1[idx])));
        double2 s1 = bs_assemble(bs_diss_hat(w2, g1), cbR, bs_llp_hat(w2, invert_layer(d, 1, idx, qh0[idx], qh1[idx])));
        if (!selfc) { pack_store(Z, g, j, i, s0, s1, d.invN2); continue; }
        const int idm = jm * NK + i;
        const double wm = d.wv2[idm];
        double2 m0, m1;
        unpack_pair(Z, g, jm, i, m0, m1);
        const double2 t0 = bs_assemble(bs_diss_hat(wm, m0), cbR, bs_llp_hat(wm, invert_layer(d, 0, idm, qh0[idm], qh1[idm])));
        const double2 t1 = bs_assemble(bs_diss_hat(wm, m1), cbR, bs_llp_hat(wm, invert_layer(d, 1, idm, qh0[idm], qh1[idm])));
        pack_store(Z, g, j, i, herm_mean(s0, t0), herm_mean(s1, t1), d.invN2);
        if (jm != j) pack_store(Z, g, jm, i, herm_mean(t0, s0), herm_mean(t1, s1), d.invN2);
    }
    __syncthreads();
    fft2d_inv_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
    for (int idx = threadIdx.x; idx < rz; idx += BS_THREADS) {
        const int y = idx / N, x = idx - y * N;
        const double2 w = Z[y * LD + x];
        Sb[idx] = w.x;
        Sb[rz + idx] = w.y;
    }
}

// ------------------------------------------------------------------ other grids: three kernels around the batched transforms
// half spectra of Sxx, Sxy and lap lap psi of both layers; grid (chunks, B)
__global__ void k_bs_spectra(SpecDev d, const double2 *qh, double2 *Sxxh, double2 *Sxyh, double2 *Llph) {
    const int sz = d.N * d.NK, b = blockIdx.y;
    const size_t so = (size_t)b * 2 * sz;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < sz; idx += gridDim.x * blockDim.x) {
        const int j = idx / d.NK, i = idx - j * d.NK;
        const double kx = d.kk[i], ly = d.ll[j], w2 = d.wv2[idx];
        const double2 q0 = qh[so + idx], q1 = qh[so + sz + idx];
        for (int k = 0; k < 2; ++k) {
            const double2 ph = invert_layer(d, k, idx, q0, q1);
            const size_t o = so + (size_t)k * sz + idx;
            Sxxh[o] = bs_sxx_hat(kx, ly, ph);
            Sxyh[o] = bs_sxy_hat(kx, ly, ph);
            Llph[o] = bs_llp_hat(w2, ph);
        }
    }
}

// g = llp dx^2 nu over (B,2,N,N), written over Sxx; grid (chunks, B)
__global__ void k_bs_g(SpecDev d, const double *smag, double *Sxx_g, const double *Sxy, const double *Llp) {
    const int n = 2 * d.N * d.N, b = blockIdx.y;
    const size_t ro = (size_t)b * n;
    const double cs = smag[b] * d.dx, cs2 = cs * cs, dx2 = d.dx * d.dx;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x)
        Sxx_g[ro + idx] = Llp[ro + idx] * dx2 * bs_nu(cs2, Sxx_g[ro + idx], Sxy[ro + idx]);
}

// one workgroup per member: R, then dqh = K^2 g^ - C_B R K^4 ph (gh and dqh may not alias)
__global__ __launch_bounds__(BS_THREADS) void k_bs_ratio_assemble(SpecDev d, BsArgs a, const double2 *gh, double2 *dqh) {
    const int sz = d.N * d.NK, NK = d.NK, N = d.N, b = blockIdx.x;
    const size_t so = (size_t)b * 2 * sz;
    const double2 *qh0 = a.qh + so, *qh1 = qh0 + sz;
    double num = 0.0, den = 0.0;
    for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
        const int i = idx % NK;
        const double w2 = d.wv2[idx];
        const double2 p0 = invert_layer(d, 0, idx, qh0[idx], qh1[idx]), p1 = invert_layer(d, 1, idx, qh0[idx], qh1[idx]);
        const double w = (i == 0 || 2 * i == N) ? 1.0 : 2.0;
        num += bs_share(w, d.H[0], d.H[1], p0, bs_diss_hat(w2, gh[so + idx]), p1, bs_diss_hat(w2, gh[so + sz + idx]));
        den += bs_share(w, d.H[0], d.H[1], p0, bs_llp_hat(w2, p0), p1, bs_llp_hat(w2, p1));
    }
    const double R = bs_ratio(d, num, den, a.eps);
    if (a.ratio && threadIdx.x == 0) a.ratio[b] = R;
    const double cbR = a.back[b] * R;
    for (int idx = threadIdx.x; idx < sz; idx += BS_THREADS) {
        const double w2 = d.wv2[idx];
        const double2 p0 = invert_layer(d, 0, idx, qh0[idx], qh1[idx]), p1 = invert_layer(d, 1, idx, qh0[idx], qh1[idx]);
        dqh[so + idx] = bs_assemble(bs_diss_hat(w2, gh[so + idx]), cbR, bs_llp_hat(w2, p0));
        dqh[so + sz + idx] = bs_assemble(bs_diss_hat(w2, gh[so + sz + idx]), cbR, bs_llp_hat(w2, p1));
    }
}

// ------------------------------------------------------------------ host
static size_t bs_small_lds_bytes(const SpecDev &d) {      // field + digit-reversal table + twiddle table (make_grid)
    size_t bytes = (size_t)d.N * d.LD * sizeof(double2) + (size_t)((d.N + 3) & ~3) * sizeof(int) + (size_t)d.N * sizeof(double2);
    return (bytes + 15) & ~(size_t)15;
}

#define QGX_BS_DISPATCH_N(N_, CALL)             \
    switch (N_) {                               \
        case 32: { constexpr int NN = 32; CALL; } break; \
        case 48: { constexpr int NN = 48; CALL; } break; \
        case 64: { constexpr int NN = 64; CALL; } break; \
        case 96: { constexpr int NN = 96; CALL; } break; \
        default: { constexpr int NN = 0; CALL; } break;  \
    }

// the large-grid work fields (three spectral, three real), allocated when the closure is first switched on
int backscatter_prepare(qgx_model *m) {
    if (m->small) {
        const int bytes = (int)bs_small_lds_bytes(m->d);
        QGX_BS_DISPATCH_N(m->N, QGX_HIP(hipFuncSetAttribute((const void *)k_backscatter_small<NN>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)))
        return QGX_OK;
    }
    const size_t nr = (size_t)m->B * 2 * m->N * m->N, ns = (size_t)m->B * 2 * m->N * m->NK;
    for (int i = 0; i < 3; ++i) {
        if (!m->bs_spec[i]) QGX_HIP(hipMalloc((void **)&m->bs_spec[i], ns * sizeof(double2)));
        if (!m->bs_real[i]) QGX_HIP(hipMalloc((void **)&m->bs_real[i], nr * sizeof(double)));
    }
    return QGX_OK;
}

// S (B,2,N,N) and, if asked for, R (B) of the state qh; changes nothing else
int backscatter_eval(qgx_model *m, const double2 *qh, double *S, double *ratio, hipStream_t st) {
    const SpecDev &d = m->d;
    BsArgs a;
    a.qh = qh; a.smag = m->bs_const; a.back = m->bs_const + m->cfg.n_members; a.eps = m->bs_eps; a.S = S; a.ratio = ratio;
    if (m->small) {
        QGX_BS_DISPATCH_N(d.N, hipLaunchKernelGGL(k_backscatter_small<NN>, dim3(d.B), dim3(BS_THREADS), bs_small_lds_bytes(d), st, d, a))
        QGX_HIP(hipGetLastError());
        return QGX_OK;
    }
    const int sz = d.N * d.NK, nr = 2 * d.N * d.N;
    const dim3 gs((unsigned)((sz + 255) / 256 > 1024 ? 1024 : (sz + 255) / 256), d.B);
    const dim3 gr((unsigned)((nr + 255) / 256 > 1024 ? 1024 : (nr + 255) / 256), d.B);
    double2 *Sxxh = m->bs_spec[0], *Sxyh = m->bs_spec[1], *Llph = m->bs_spec[2];
    double *Sxx = m->bs_real[0], *Sxy = m->bs_real[1], *Llp = m->bs_real[2];
    int rc;
    hipLaunchKernelGGL(k_bs_spectra, gs, dim3(256), 0, st, d, qh, Sxxh, Sxyh, Llph);
    if ((rc = large_qh_to_q(m, Sxxh, Sxx, st)) || (rc = large_qh_to_q(m, Sxyh, Sxy, st)) || (rc = large_qh_to_q(m, Llph, Llp, st))) return rc;
    hipLaunchKernelGGL(k_bs_g, gr, dim3(256), 0, st, d, a.smag, Sxx, (const double *)Sxy, (const double *)Llp);
    if ((rc = large_q_to_qh(m, Sxx, Sxyh, st))) return rc;                     // g^ (the strain spectra are spent)
    hipLaunchKernelGGL(k_bs_ratio_assemble, dim3(d.B), dim3(BS_THREADS), 0, st, d, a, (const double2 *)Sxyh, Sxxh);
    if ((rc = large_qh_to_q(m, Sxxh, S, st))) return rc;
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
#undef QGX_BS_DISPATCH_N

}  // namespace qgx
