// The spectral divergence behind a flux-form AndrewCNN, y = 10000 irfftn(ik rfftn(fx) + il rfftn(fy)), and its adjoint, as
// device functions: fluxdiv.hip (the generator's planar kernel) and fluxdiv_train.hip (the training step's kernels in the engine
// layout, and the backward in both) instantiate them, so that a net is trained on the forward that its inference computes.
// The header comment of fluxdiv.hip derives the Hermitian multipliers Hx, Hy that both functions use.
//
//   fluxdiv_body      one workgroup per (member, layer): z = fx + i fy, forward FFT, the pair multiply, inverse FFT, scale
//   fluxdiv_adjoint   one workgroup per (member, direction): z = g1 + i g2 (the operator is real: it acts on the real and
//                     the imaginary part separately, so the two layers share one transform and no pair is separated), forward
//                     FFT, the pointwise multiply by conj(Hx) or conj(Hy) on the full plane, inverse FFT, scale
//
// LAYOUT (include/qgx_flux_train.h): QGX_FLUX_PLANAR F (B, 4, N, N), y (B, 2, N, N); QGX_FLUX_ENGINE (B, N, N, 8) records
// [fx1, fx2, fy1, fy2, 0, 0, 0, 0] and [y1, y2, 0, ...]: only the first 16 bytes of an F record and the first 8 of a dy
// record are read, and every byte of an output record is written exactly once, the pad channels as zero.
#pragma once
#include "common.hpp"
#include "fft_lds_f32.hpp"

namespace qgx {

constexpr int fluxdiv_threads(int N) { return N >= 64 ? 1024 : 256; }
constexpr size_t fluxdiv_lds_bytes(int N) { return (size_t)N * (N + 1) * sizeof(float2) + N * sizeof(float2) + N * sizeof(int); }

// tw[j] = exp(-2 pi i j / N), pos[j] = where the forward transform leaves frequency j (no barrier)
template <int N>
__device__ __forceinline__ void fluxdiv_tables(float2 *tw, int *pos) {
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        double s, co;
        sincospi(-2.0 * j / N, &s, &co);                         // rounded ONCE from float64
        tw[j] = make_float2((float)co, (float)s);
        pos[j] = fft32::freq_pos(j, N);
    }
}

template <int N, int LAYOUT>
__device__ __forceinline__ void fluxdiv_body(const float *__restrict__ F, float *__restrict__ y, unsigned char *smem) {
    constexpr int LD = N + 1, H = N / 2;
    float2 *Z = reinterpret_cast<float2 *>(smem);                // [N][LD]
    float2 *tw = Z + N * LD;                                     // exp(-2 pi i j / N), j < N
    int *pos = reinterpret_cast<int *>(tw + N);                  // where the forward transform leaves frequency j
    const int b = blockIdx.x >> 1, c = blockIdx.x & 1;
    if constexpr (LAYOUT == QGX_FLUX_PLANAR) {
        const float *fx = F + ((size_t)b * 4 + c) * N * N, *fy = fx + 2 * (size_t)N * N;
        for (int i = threadIdx.x; i < N * N / 4; i += blockDim.x) {  // N % 4 == 0: a quad stays in its row
            const float4 a = reinterpret_cast<const float4 *>(fx)[i], d = reinterpret_cast<const float4 *>(fy)[i];
            const int r = 4 * i / N, col = 4 * i - r * N;
            float2 *z = Z + r * LD + col;
            z[0] = make_float2(a.x, d.x); z[1] = make_float2(a.y, d.y); z[2] = make_float2(a.z, d.z); z[3] = make_float2(a.w, d.w);
        }
    } else {
        const float4 *rec = reinterpret_cast<const float4 *>(F) + (size_t)b * N * N * 2;     // two float4 per pixel record
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const float4 a = rec[(size_t)i * 2];
            const int r = i / N, col = i - r * N;
            Z[r * LD + col] = c ? make_float2(a.y, a.w) : make_float2(a.x, a.z);
        }
    }
    fluxdiv_tables<N>(tw, pos);
    __syncthreads();
    fft32::fft2d_fwd<N>(Z, tw);
    // every conjugate pair {(l,k), (-l,-k)} once: k = 0 .. N/2, and on the two self-paired columns l <= -l (mod N) only
    const double dk = 6.283185307179586 / 1e6;
    for (int w = threadIdx.x; w < N * (H + 1); w += blockDim.x) {
        const int l = w / (H + 1), k = w - l * (H + 1);
        const int lm = l ? N - l : 0, km = k ? N - k : 0;
        if ((k == 0 || k == H) && l > lm) continue;
        float2 *pa = Z + pos[l] * LD + pos[k], *pb = Z + pos[lm] * LD + pos[km];
        const float2 A = *pa, Bc = make_float2(pb->x, -pb->y);
        // X = (A + conj B) / 2, Y = (A - conj B) / (2 i): the spectra of fx and fy at (l, k)
        const float2 X = make_float2(0.5f * (A.x + Bc.x), 0.5f * (A.y + Bc.y));
        const float2 Y = make_float2(0.5f * (A.y - Bc.y), -0.5f * (A.x - Bc.x));
        const float wk = k == H ? 0.f : (float)(dk * (double)k);
        const float wl = l != H ? (float)(dk * (double)(l < H ? l : l - N)) : ((k == 0 || k == H) ? 0.f : (float)(dk * (double)(-H)));
        const float2 t = make_float2(X.x * wk + Y.x * wl, X.y * wk + Y.y * wl);
        const float2 D = make_float2(-t.y, t.x);                 // i t
        *pa = D;
        *pb = make_float2(D.x, -D.y);                            // (a self-paired bin: D = 0 there, both multipliers vanish)
    }
    __syncthreads();
    fft32::fft2d_inv<N>(Z, tw);
    constexpr float inv = 1.0f / (float)(N * N);
    if constexpr (LAYOUT == QGX_FLUX_PLANAR) {
        float *out = y + ((size_t)b * 2 + c) * N * N;
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const int r = i / N, col = i - r * N;
            out[i] = 10000.f * (Z[r * LD + col].x * inv);
        }
    } else {
        // layer 0 writes channel 0 and the pad channels 4 ... 7, layer 1 channel 1 and the pad channels 2, 3
        float *out = y + (size_t)b * N * N * 8;
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const int r = i / N, col = i - r * N;
            float *rec = out + (size_t)i * 8;
            rec[c] = 10000.f * (Z[r * LD + col].x * inv);
            if (c) *reinterpret_cast<float2 *>(rec + 2) = make_float2(0.f, 0.f);
            else *reinterpret_cast<float4 *>(rec + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// dF = D^T dy: workgroup (member b, direction d) computes 10000 ifft2(conj(H_d) fft2(g1 + i g2)); its real part is the
// gradient of layer 1's flux in direction d, its imaginary part layer 2's
template <int N, int LAYOUT>
__device__ __forceinline__ void fluxdiv_adjoint(const float *__restrict__ dy, float *__restrict__ dF, unsigned char *smem) {
    constexpr int LD = N + 1, H = N / 2;
    float2 *Z = reinterpret_cast<float2 *>(smem);
    float2 *tw = Z + N * LD;
    int *pos = reinterpret_cast<int *>(tw + N);
    const int b = blockIdx.x >> 1, d = blockIdx.x & 1;
    if constexpr (LAYOUT == QGX_FLUX_PLANAR) {
        const float *g1 = dy + (size_t)b * 2 * N * N, *g2 = g1 + (size_t)N * N;
        for (int i = threadIdx.x; i < N * N / 4; i += blockDim.x) {
            const float4 a = reinterpret_cast<const float4 *>(g1)[i], e = reinterpret_cast<const float4 *>(g2)[i];
            const int r = 4 * i / N, col = 4 * i - r * N;
            float2 *z = Z + r * LD + col;
            z[0] = make_float2(a.x, e.x); z[1] = make_float2(a.y, e.y); z[2] = make_float2(a.z, e.z); z[3] = make_float2(a.w, e.w);
        }
    } else {
        const float *rec = dy + (size_t)b * N * N * 8;
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const int r = i / N, col = i - r * N;
            Z[r * LD + col] = *reinterpret_cast<const float2 *>(rec + (size_t)i * 8);
        }
    }
    fluxdiv_tables<N>(tw, pos);
    __syncthreads();
    fft32::fft2d_fwd<N>(Z, tw);
    // conj(H) G = -i w G on the full plane, w the real wavenumber of H = i w (fluxdiv_body's expressions; on the Nyquist row
    // Hy carries sign(k), which the pair loop there gets from the conjugate partner)
    const double dk = 6.283185307179586 / 1e6;
    for (int w = threadIdx.x; w < N * N; w += blockDim.x) {
        const int l = w / N, k = w - l * N;
        float wn;
        if (d == 0) {
            wn = k == H ? 0.f : (float)(dk * (double)(k < H ? k : k - N));
        } else {
            wn = l != H ? (float)(dk * (double)(l < H ? l : l - N))
                        : ((k == 0 || k == H) ? 0.f : (k < H ? (float)(dk * (double)(-H)) : -(float)(dk * (double)(-H))));
        }
        float2 *p = Z + pos[l] * LD + pos[k];
        const float2 G = *p;
        *p = make_float2(G.y * wn, -(G.x * wn));                 // -i w G
    }
    __syncthreads();
    fft32::fft2d_inv<N>(Z, tw);
    constexpr float inv = 1.0f / (float)(N * N);
    if constexpr (LAYOUT == QGX_FLUX_PLANAR) {
        float *o1 = dF + ((size_t)b * 4 + 2 * d) * N * N, *o2 = o1 + (size_t)N * N;
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const int r = i / N, col = i - r * N;
            const float2 v = Z[r * LD + col];
            o1[i] = 10000.f * (v.x * inv);
            o2[i] = 10000.f * (v.y * inv);
        }
    } else {
        // direction x writes channels 0, 1 and the pad channels 4 ... 7, direction y channels 2, 3
        float *out = dF + (size_t)b * N * N * 8;
        for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
            const int r = i / N, col = i - r * N;
            const float2 v = Z[r * LD + col];
            float *rec = out + (size_t)i * 8;
            *reinterpret_cast<float2 *>(rec + 2 * d) = make_float2(10000.f * (v.x * inv), 10000.f * (v.y * inv));
            if (d == 0) *reinterpret_cast<float4 *>(rec + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

}  // namespace qgx
