// Packed-pair helpers of the LDS-resident kernels (spectral_small.hip, backscatter.hip): two real fields travel through
// one complex N x N transform as A + i B; the functions here add the addressing of the digit-reversed LDS field to the
// per-element arithmetic of spectral_elem.hpp.
#pragma once
#include "common.hpp"
#include "spectral_elem.hpp"

namespace qgx {

struct Grid {
    int N, NK, LD, nrad;
    const int *rad;     // registers/param space
    const int *pos;     // LDS copy
    const double2 *tw;
};

// half-spectra (A,B) of the real parts packed as A + iB, read out of the DIF-ordered field
__device__ __forceinline__ void unpack_pair(const double2 *Z, const Grid &g, int j, int i,
                                            double2 &A, double2 &Bv) {
    const int jm = neg_mod(j, g.N), im = neg_mod(i, g.N);
    unpack_half(Z[g.pos[j] * g.LD + g.pos[i]], Z[g.pos[jm] * g.LD + g.pos[im]], A, Bv);
}

// store the Hermitian extension of (Ah + i Bh) at (j,i) [and its mirror], DIT-input order.
// For the self-conjugate columns the caller passes already symmetrised values.
__device__ __forceinline__ void pack_store(double2 *Z, const Grid &g, int j, int i, double2 Ah,
                                           double2 Bh, double scale) {
    Z[g.pos[j] * g.LD + g.pos[i]] = pack_self(Ah, Bh, scale);
    if (i != 0 && 2 * i != g.N) Z[g.pos[neg_mod(j, g.N)] * g.LD + g.pos[g.N - i]] = pack_mirror(Ah, Bh, scale);
}

// Build the packed spectrum of (u_k + i v_k) from qh; optionally store ph_k.
__device__ __forceinline__ void build_uv(double2 *Z, const Grid &g, const SpecDev &d, int k,
                                         const double2 *qh0, const double2 *qh1, double2 *ph_out) {
    const int N = g.N, NK = g.NK;
    for (int idx = threadIdx.x; idx < N * NK; idx += blockDim.x) {
        const int j = idx / NK, i = idx - j * NK;
        const double2 ph = invert_layer(d, k, idx, qh0[idx], qh1[idx]);
        if (ph_out) ph_out[idx] = ph;
        const double kx = d.kk[i], ly = d.ll[j];
        double2 uh = u_hat(ly, ph), vh = v_hat(kx, ph);
        if (i == 0 || 2 * i == N) {
            const int jm = neg_mod(j, N);
            const int idm = jm * NK + i;
            const double2 pm = invert_layer(d, k, idm, qh0[idm], qh1[idm]);
            uh = herm_mean(uh, u_hat(d.ll[jm], pm));
            vh = herm_mean(vh, v_hat(kx, pm));
        }
        pack_store(Z, g, j, i, uh, vh, d.invN2);
    }
}

// Build the packed spectrum of (A + i B) from two half spectra in global memory (Bh == nullptr: B = 0).
__device__ __forceinline__ void build_pair(double2 *Z, const Grid &g, const double2 *Ah,
                                           const double2 *Bh, double scale) {
    const int N = g.N, NK = g.NK;
    for (int idx = threadIdx.x; idx < N * NK; idx += blockDim.x) {
        const int j = idx / NK, i = idx - j * NK;
        double2 a = Ah[idx], b = Bh ? Bh[idx] : make_double2(0., 0.);
        if (i == 0 || 2 * i == N) {
            const int idm = neg_mod(j, N) * NK + i;
            a = herm_mean(a, Ah[idm]);
            b = herm_mean(b, Bh ? Bh[idm] : make_double2(0., 0.));
        }
        pack_store(Z, g, j, i, a, b, scale);
    }
}

__device__ __forceinline__ Grid make_grid(const SpecDev &d, double2 *Z, int *&pos_lds) {
    Grid g;
    g.N = d.N; g.NK = d.NK; g.LD = d.LD; g.nrad = d.nrad; g.rad = d.rad; g.tw = d.tw;
    pos_lds = reinterpret_cast<int *>(Z + d.N * d.LD);
    // twiddle table in LDS too: read from global memory, every butterfly of a transform's first pass waits for an
    // L1 / L2 round trip (the large-grid kernels measured 60-70 % wait that way)
    double2 *tw_lds = reinterpret_cast<double2 *>(pos_lds + ((d.N + 3) & ~3));
    for (int t = threadIdx.x; t < d.N; t += blockDim.x) { pos_lds[t] = d.pos[t]; tw_lds[t] = d.tw[t]; }
    g.pos = pos_lds;
    g.tw = tw_lds;
    return g;
}

extern __shared__ __attribute__((aligned(16))) char qgx_smem[];

}  // namespace qgx
