// In-LDS mixed-radix complex FFT passes in float32 for gfx950: the flow graphs of fft_lds.hpp (forward = decimation in
// frequency, natural order in -> digit-reversed order out; inverse = the transposed graph, digit-reversed in -> natural
// out; consecutive lanes take consecutive LINES, rows padded to N + 1 elements), restated for float2 with radices 2, 3, 4, 8
// and 16 and compile-time plans only.  fft_lds.hpp stays float64: the spectral step's arithmetic is not touched by this file.
// Used by fluxdiv.hip (the float32 spectral divergence behind a flux-form AndrewCNN).
#pragma once
#include <hip/hip_runtime.h>

namespace qgx {
namespace fft32 {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// multiply by -i (forward) / +i (inverse)
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }
__device__ __forceinline__ float2 mul_pi(float2 a) { return make_float2(-a.y, a.x); }

template <int R, bool FWD>
__device__ __forceinline__ void small_dft(float2 (&v)[R]) {
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 3) {
        const float c = -0.5f, s = 0.86602540378443864676f;   // cos, sin of 2 pi / 3
        const float2 t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
        const float2 m = make_float2(v[0].x + c * t.x, v[0].y + c * t.y);
        const float2 isd = make_float2(-s * d.y, s * d.x);       // i s d
        v[0] = cadd(v[0], t);
        if (FWD) { v[1] = csub(m, isd); v[2] = cadd(m, isd); }
        else     { v[1] = cadd(m, isd); v[2] = csub(m, isd); }
    } else if constexpr (R == 4) {
        const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]);
        const float2 s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
        const float2 r = FWD ? mul_mi(d13) : mul_pi(d13);
        v[0] = cadd(s02, s13);
        v[1] = cadd(d02, r);
        v[2] = csub(s02, s13);
        v[3] = csub(d02, r);
    } else if constexpr (R == 8) {
        // two interleaved radix-4 transforms (even / odd inputs) + one radix-2 stage with W8^k
        float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
        small_dft<4, FWD>(e);
        small_dft<4, FWD>(o);
        const float h = 0.70710678118654752440f;
        float2 t1, t2, t3;
        if (FWD) {
            t1 = make_float2(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));
            t2 = mul_mi(o[2]);
            t3 = make_float2(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));
        } else {
            t1 = make_float2(h * (o[1].x - o[1].y), h * (o[1].y + o[1].x));
            t2 = mul_pi(o[2]);
            t3 = make_float2(-h * (o[3].x + o[3].y), h * (o[3].x - o[3].y));
        }
        v[0] = cadd(e[0], o[0]); v[4] = csub(e[0], o[0]);
        v[1] = cadd(e[1], t1);   v[5] = csub(e[1], t1);
        v[2] = cadd(e[2], t2);   v[6] = csub(e[2], t2);
        v[3] = cadd(e[3], t3);   v[7] = csub(e[3], t3);
    } else {   // R == 16 = 4 x 4, decimation in time over the four interleaved length-4 sequences x[4m + r]
        static_assert(R == 16, "radix");
        float2 f0[4] = {v[0], v[4], v[8], v[12]}, f1[4] = {v[1], v[5], v[9], v[13]};
        float2 f2[4] = {v[2], v[6], v[10], v[14]}, f3[4] = {v[3], v[7], v[11], v[15]};
        small_dft<4, FWD>(f0);
        small_dft<4, FWD>(f1);
        small_dft<4, FWD>(f2);
        small_dft<4, FWD>(f3);
        const float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
        const float sg = FWD ? -1.0f : 1.0f;
        // W16^j = (cos(pi j / 8), sg sin(pi j / 8))
        f1[1] = cmul(f1[1], make_float2(c1, sg * s1));
        f1[2] = cmul(f1[2], make_float2(h, sg * h));
        f1[3] = cmul(f1[3], make_float2(s1, sg * c1));
        f2[1] = cmul(f2[1], make_float2(h, sg * h));
        f2[2] = FWD ? mul_mi(f2[2]) : mul_pi(f2[2]);
        f2[3] = cmul(f2[3], make_float2(-h, sg * h));
        f3[1] = cmul(f3[1], make_float2(s1, sg * c1));
        f3[2] = cmul(f3[2], make_float2(-h, sg * h));
        f3[3] = cmul(f3[3], make_float2(-c1, -sg * s1));
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            float2 g[4] = {f0[k1], f1[k1], f2[k1], f3[k1]};
            small_dft<4, FWD>(g);
            v[k1] = g[0]; v[k1 + 4] = g[1]; v[k1 + 8] = g[2]; v[k1 + 12] = g[3];
        }
    }
}

// One pass of radix R with current block size n over `nl` lines of length N at Z + line * ls + e * es; tw[j] = exp(-2 pi i j / N)
template <int R, bool FWD>
__device__ __forceinline__ void fft_pass(float2 *Z, int nl, int ls, int es, int n, int N, const float2 *tw) {
    const int sub = n / R;
    const int per_line = N / R;
    const int total = nl * per_line;
    const int tstride = N / n;
    for (int w = threadIdx.x; w < total; w += blockDim.x) {
        const int bb = w / nl;
        const int line = w - bb * nl;
        const int blk = bb / sub;
        const int b = bb - blk * sub;
        float2 *base = Z + line * ls + (blk * n + b) * es;
        const int step = sub * es;
        float2 v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = base[m * step];
        if constexpr (FWD) {
            small_dft<R, true>(v);
            if (sub > 1) {
#pragma unroll
                for (int m = 1; m < R; ++m) v[m] = cmul(v[m], tw[m * b * tstride]);
            }
        } else {
            if (sub > 1) {
#pragma unroll
                for (int m = 1; m < R; ++m) v[m] = cmulc(v[m], tw[m * b * tstride]);
            }
            small_dft<R, false>(v);
        }
#pragma unroll
        for (int m = 0; m < R; ++m) base[m * step] = v[m];
    }
}

// the plan: 16 while it divides, then 8, 4, 2, 3 (128 = 16 x 8, 96 = 16 x 2 x 3, 64 = 16 x 4, 48 = 16 x 3, 32 = 16 x 2)
constexpr int pick_radix(int n) { return n % 16 == 0 ? 16 : (n % 8 == 0 ? 8 : (n % 4 == 0 ? 4 : (n % 2 == 0 ? 2 : 3))); }

template <int N, int n>
__device__ __forceinline__ void fft_lines_fwd(float2 *Z, int nl, int ls, int es, const float2 *tw) {
    if constexpr (n > 1) {
        constexpr int R = pick_radix(n);
        fft_pass<R, true>(Z, nl, ls, es, n, N, tw);
        __syncthreads();
        fft_lines_fwd<N, n / R>(Z, nl, ls, es, tw);
    }
}
template <int N, int n>
__device__ __forceinline__ void fft_lines_inv(float2 *Z, int nl, int ls, int es, const float2 *tw) {
    if constexpr (n > 1) {
        constexpr int R = pick_radix(n);
        fft_lines_inv<N, n / R>(Z, nl, ls, es, tw);
        fft_pass<R, false>(Z, nl, ls, es, n, N, tw);
        __syncthreads();
    }
}
// where the forward transform of length n leaves frequency k: pass 1 sends the frequencies k = m (mod R) to sub-block m
constexpr int freq_pos(int k, int n) {
    int p = 0;
    while (n > 1) {
        const int R = pick_radix(n);
        n /= R;
        p += (k % R) * n;
        k /= R;
    }
    return p;
}

// 2-D transforms of an N x N field with row stride N + 1 (callers barrier BEFORE; each ends with a barrier)
template <int N>
__device__ __forceinline__ void fft2d_fwd(float2 *Z, const float2 *tw) {
    fft_lines_fwd<N, N>(Z, N, N + 1, 1, tw);   // along x, lines = rows
    fft_lines_fwd<N, N>(Z, N, 1, N + 1, tw);   // along y, lines = columns
}
template <int N>
__device__ __forceinline__ void fft2d_inv(float2 *Z, const float2 *tw) {
    fft_lines_inv<N, N>(Z, N, 1, N + 1, tw);
    fft_lines_inv<N, N>(Z, N, N + 1, 1, tw);
}

}  // namespace fft32
}  // namespace qgx
