// Generator forward: the 8-layer circular-padded CNN as implicit-GEMM convolutions on the
// exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), fused bias + ReLU + eval-mode BatchNorm.
//
// Replaces AndrewCNN.forward evaluated through apply_function
// (pyqg_generative/tools/cnn_tools.py:79-98 make_block = Conv2d('same', circular) -> ReLU ->
// BatchNorm2d; :125-176 channels [n_in,128,64,32,32,32,32,32,n_out], kernels [5,5,3,3,3,3,3,3];
// :702-735 eval mode, no grad).  The handle, the model wrappers around the nets and the C ABI that is not
// AndrewCNN-specific are in generator.hip; generator.hpp holds the handle and the functions between the two files.
//
// Data layout: activations NHWC float32 (B, N, N, C) so that the GEMM K index
// (tap, input channel) is contiguous per pixel; the first layer reads a small planar
// (B, n_in, N, N) input and the last writes planar (B, n_out, N, N).
// One workgroup (4 waves) owns R full-width image rows (M = R*N pixels, all output
// channels); the input patch of (R+K-1) rows is staged once per input-channel chunk
// into LDS with a padded pixel stride, horizontal wrap-around is resolved when the
// A fragment address is formed, vertical wrap-around when the patch is staged.
// MFMA 32x32x2 f32: A[i = lane&31][k = lane>>5] = pixel x K, B[k][j = lane&31] = K x cout.
// Lane half h consumes K indices 8g+4h .. 8g+4h+3 of every group of 8 with one 16-byte
// read of A (LDS) and of B (packed weights, L2 resident) feeding 4 consecutive MFMAs.
#include "generator.hpp"
#include <unordered_map>
#include <cmath>
#include <utility>
#include <functional>

namespace qgx {

#include "conv_types.hpp"

struct ConvArgs {
    const float *in;       // NHWC (B,N,N,CIN) or planar (B,CIN,N,N)
    float *out;            // NHWC (B,N,N,COUT) or planar (B,COUT_REAL,N,N)
    const float *w;        // packed [kgroup][COUTP][8]
    const float *bias, *scale, *shift;   // [COUTP]
    int N, R, cout_real;
    int out_channels;      // k_conv_last: channels of a member in `out` (a flux-form net writes its four in two launches of two)
    size_t npix_total;     // B*N*N (stride of one split-K partial plane)
    float ascale;          // OUTH: power-of-two pre-scale of the stored 16-bit activations
    unsigned *range;       // OUTH: f16x3 range guard flag word (conv_half.hpp::range_guard)
};

#include "conv_half.hpp"
#include "conv_pair.hpp"
#include "conv_wino.hpp"
// conv_wino2.hip (a translation unit of its own: built without the SLP vectoriser): the same layer with the input transform
// under the MFMAs, bit-identical to k_convw, for the tile shapes where it is faster; *done = false: take k_convw
int launch_convw2(int N, int TW, int R, const ConvWArgs &a, int total_tiles, hipStream_t st, bool *done);
bool convw2_takes(int N, int TW, int R);     // the tile shapes k_convw2 is built for
// One path per layer and size: the kernel variants that were measured slower than the ones above (a generic run-time-N
// 16-bit kernel and its plain-f16 mode, resident weights, 16x16x32 MFMAs, full-line chunks, a channel-planar layer 1) are
// not carried; their measurements are in DESIGN.md 3.2b-d.  The A/B library (`make ab` -> libqgx_ab.so) is this code plus
// the fault-injection hooks of model.hip / common.hpp and qgx_debug_read_act.

// OUTH = 0: f32 NHWC output.  OUTH = 2 (first layer only): the MFMA roles are swapped (lane = pixel)
// and the epilogue writes the packed f16 hi-lo activation layout of conv_half.hpp.
template <int CIN, int COUT, int KS, int CC, int MT, bool PLANAR_IN, bool FINAL, int CSPLIT = 1, bool PARTIAL = false, int OUTH = 0>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
    static_assert(OUTH == 0 || (OUTH == 2 && PLANAR_IN && !FINAL && !PARTIAL), "16-bit output: first layer only");
    constexpr int NTF = (COUT + 31) / 32;        // all output-channel tiles of the layer
    constexpr int NT = NTF / CSPLIT;             // tiles owned by this workgroup (blockIdx.y picks the slice)
    constexpr int COUTP = NTF * 32;
    const int nt0 = CSPLIT > 1 ? blockIdx.y * NT : 0;
    constexpr int P = KS / 2;
    constexpr int T = KS * KS;
    constexpr int STRIDE = PLANAR_IN ? CIN : CC + 4;   // floats per patch pixel
    float *patch = reinterpret_cast<float *>(conv_smem);

    const int N = a.N, R = a.R;
    const int tiles_per_img = N / R;
    const int b = blockIdx.x / tiles_per_img;
    const int y0 = (blockIdx.x - b * tiles_per_img) * R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int ntiles = R * N / 32;
    const int PR = R + KS - 1;

    int py[MT], px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int tile = wave + 4 * mt;
        if (tile >= ntiles) tile = 0;              // duplicate work on a valid tile, never stored
        const int p = tile * 32 + li;
        py[mt] = p / N;
        px[mt] = p - py[mt] * N;
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    if constexpr (PLANAR_IN) {
        // ---- stage the whole (tiny) input patch: patch[(pr*N + x)*CIN + c]
        for (int it = threadIdx.x; it < PR * CIN * N; it += 256) {
            const int x = it % N;
            const int c = (it / N) % CIN;
            const int pr = it / (N * CIN);
            int gy = y0 - P + pr;
            gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
            patch[(pr * N + x) * CIN + c] = a.in[(((size_t)b * CIN + c) * N + gy) * N + x];
        }
        __syncthreads();
        constexpr int NG = (T * CIN + 7) / 8;
        const float4 *wp = reinterpret_cast<const float4 *>(a.w) + (size_t)li * 2 + h;
        for (int g = 0; g < NG; ++g) {
            float4 A[MT], Bf[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) Bf[nt] = wp[((size_t)g * COUTP + (nt0 + nt) * 32) * 2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if constexpr (CIN == 4) {
                    int tap = 2 * g + h;
                    if (tap >= T) tap = 0;             // zero weights there
                    const int ky = tap / KS, kx = tap - ky * KS;
                    int col = px[mt] + kx - P;
                    col = col < 0 ? col + N : (col >= N ? col - N : col);
                    A[mt] = *reinterpret_cast<const float4 *>(&patch[((py[mt] + ky) * N + col) * 4]);
                } else {   // CIN == 2: two taps per lane half
                    float2 v[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        int tap = 4 * g + 2 * h + e;
                        if (tap >= T) tap = 0;
                        const int ky = tap / KS, kx = tap - ky * KS;
                        int col = px[mt] + kx - P;
                        col = col < 0 ? col + N : (col >= N ? col - N : col);
                        v[e] = *reinterpret_cast<const float2 *>(&patch[((py[mt] + ky) * N + col) * 2]);
                    }
                    A[mt] = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = OUTH ? __builtin_amdgcn_mfma_f32_32x32x2f32(
                                                 (&Bf[nt].x)[e], (&A[mt].x)[e], acc[mt][nt], 0, 0, 0)
                                           : __builtin_amdgcn_mfma_f32_32x32x2f32(
                                                 (&A[mt].x)[e], (&Bf[nt].x)[e], acc[mt][nt], 0, 0, 0);
        }
    } else {
        constexpr int G8 = CC / 8;
        constexpr int C4 = CC / 4;
        const float4 *wp = reinterpret_cast<const float4 *>(a.w) + (size_t)li * 2 + h;
        // split-K (small ensembles): blockIdx.y owns a contiguous range of input-channel chunks and
        // stores raw partial sums; k_conv_reduce adds them in a fixed order and applies the epilogue
        int cbeg = 0, cend = CIN;
        if constexpr (PARTIAL) {
            const int per = CIN / (int)gridDim.y;
            cbeg = blockIdx.y * per;
            cend = cbeg + per;
            wp += (size_t)(cbeg / CC) * T * G8 * COUTP * 2;
        }
        for (int c0 = cbeg; c0 < cend; c0 += CC) {
            __syncthreads();
            // ---- stage patch chunk: (PR rows) x N x CC channels, pixel stride CC+4 floats
            for (int it = threadIdx.x; it < PR * N * C4; it += 256) {
                const int c4 = it % C4;
                const int x = (it / C4) % N;
                const int pr = it / (C4 * N);
                int gy = y0 - P + pr;
                gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
                const float4 vv = *reinterpret_cast<const float4 *>(
                    &a.in[(((size_t)b * N + gy) * N + x) * CIN + c0 + c4 * 4]);
                *reinterpret_cast<float4 *>(&patch[(pr * N + x) * STRIDE + c4 * 4]) = vv;
            }
            __syncthreads();
            // ---- K loop over (tap, 8-channel group), software pipelined: the A fragment (LDS) and the
            // B fragment (packed weights, L2) of step i+1 are requested before the MFMAs of step i.
            int ky = 0, kx = 0;
            int aoff[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                int col = px[mt] - P;
                col = col < 0 ? col + N : col;
                aoff[mt] = (py[mt] * N + col) * STRIDE + 4 * h;
            }
            float4 An[MT], Bn[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) Bn[nt] = wp[(size_t)(nt0 + nt) * 64];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff[mt]]);
            for (int tap = 0; tap < T; ++tap) {
                const bool last_tap = tap == T - 1;
                int nkx = kx + 1, nky = ky;
                if (nkx == KS) { nkx = 0; ++nky; }
                int aoff_n[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    int col = px[mt] + nkx - P;
                    col = col < 0 ? col + N : (col >= N ? col - N : col);
                    aoff_n[mt] = last_tap ? aoff[mt] : ((py[mt] + nky) * N + col) * STRIDE + 4 * h;
                }
                const float4 *wp_n = last_tap ? wp : wp + (size_t)G8 * COUTP * 2;
#pragma unroll
                for (int g8 = 0; g8 < G8; ++g8) {
                    float4 A[MT], Bf[NT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) A[mt] = An[mt];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) Bf[nt] = Bn[nt];
                    if (g8 + 1 < G8) {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) Bn[nt] = wp[((size_t)(g8 + 1) * COUTP + (nt0 + nt) * 32) * 2];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff[mt] + (g8 + 1) * 8]);
                    } else {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) Bn[nt] = wp_n[(size_t)(nt0 + nt) * 64];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff_n[mt]]);
                    }
                    // keep the prefetch ABOVE this step's MFMAs (hipcc otherwise sinks the loads to their use)
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                    (&A[mt].x)[e], (&Bf[nt].x)[e], acc[mt][nt], 0, 0, 0);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) aoff[mt] = aoff_n[mt];
                wp = wp_n;
                kx = nkx; ky = nky;
            }
            wp += (size_t)G8 * COUTP * 2;      // the last tap did not advance
        }
    }

    // ---- epilogue: bias (+ ReLU + BatchNorm affine), store
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int tile = wave + 4 * mt;
        if (tile >= ntiles) continue;
        if constexpr (OUTH != 0) {
            char *pix = reinterpret_cast<char *>(a.out) +
                        ((size_t)b * N * N + (size_t)y0 * N + tile * 32 + li) * (COUT * 4);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                store_tile_t<false>(acc[mt][nt], (nt0 + nt) * 32, h, pix, a.bias, a.scale, a.shift, 1.0f, a.ascale, a.range, 1u);
            continue;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = (nt0 + nt) * 32 + li;
            const float bias = a.bias[co];
            if constexpr (FINAL) {
                if (co < a.cout_real) {
                    float *o = a.out + ((size_t)b * a.cout_real + co) * N * N + (size_t)y0 * N;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        o[p] = acc[mt][nt][r] + bias;
                    }
                }
            } else if constexpr (PARTIAL) {
                float *o = a.out + ((size_t)blockIdx.y * a.npix_total + (size_t)b * N * N + (size_t)y0 * N) * COUT + co;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    o[(size_t)p * COUT] = acc[mt][nt][r];
                }
            } else {
                const float sc = a.scale[co], sh = a.shift[co];
                float *o = a.out + ((size_t)b * N * N + (size_t)y0 * N) * COUT + co;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float vv = acc[mt][nt][r] + bias;
                    vv = fmaxf(vv, 0.f);
                    o[(size_t)p * COUT] = vv * sc + sh;
                }
            }
        }
    }
}

// ---- hidden layers, LDS-only operands with register-prefetched staging ---------------------------
// Both MFMA operands come from LDS: the input patch (double buffered per 16-channel chunk) and the
// weight slice of TPS taps (double buffered).  The global loads that fetch the NEXT weight slice and
// the next chunk's patch are issued at the start of a stage into registers and written to the idle
// LDS buffers at its end, so the K loop contains no vector-memory instruction and nothing ever waits
// on HBM/L2 latency except the stage boundary.  The workgroup is persistent over its tiles, so the
// prefetch also runs across tile boundaries; one barrier per stage.
template <int CIN, int COUT, int KS, int CC, int MT, int TPS, int PPT, int NW = 4>
__global__ __launch_bounds__(NW * 64) void k_conv3(ConvArgs a, int total_tiles) {
    constexpr int NTHR = NW * 64;
    constexpr int NT = (COUT + 31) / 32;
    constexpr int COUTP = NT * 32;
    constexpr int P = KS / 2;
    constexpr int T = KS * KS;
    constexpr int G8 = CC / 8;
    constexpr int C4 = CC / 4;
    constexpr int NCH = CIN / CC;
    constexpr int STRIDE = CC + 4;
    constexpr int NSL = T / TPS;                        // weight slices per chunk
    constexpr int WSL = TPS * G8 * 2 * COUTP * 4;       // floats per slice, layout [tap][g8][h][cout][4]
    constexpr int WF4 = WSL / 4;
    constexpr int WPT = (WF4 + NTHR - 1) / NTHR;
    static_assert(T % TPS == 0, "taps per slice must divide the tap count");
    const int N = a.N, R = a.R;
    const int PR = R + KS - 1;
    const int patch_floats = PR * N * STRIDE;
    // LDS addresses are always formed arithmetically from the shared symbol: selecting between pointers
    // kept in an array makes hipcc lose the address space and emit flat_load (vmcnt+lgkmcnt, full drains)
    float *const lds0 = reinterpret_cast<float *>(conv_smem);
    float *const wlds0 = lds0 + 2 * patch_floats;
    const int tiles_per_img = N / R;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int n_my = blockIdx.x < (unsigned)total_tiles ? (total_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int ntiles = R * N / 32;
    const int PF4 = PR * N * C4;                        // float4 per patch chunk
    const int PSH = (PF4 + NSL - 1) / NSL;              // patch float4 fetched per stage

    // The staging code below is written inline (no helper lambdas taking array references): hipcc
    // keeps the prefetch registers in VGPRs only when every index is a compile-time constant in the
    // kernel body; through a by-reference helper they went to scratch and each load was drained.
#define QGX_PATCH_LOAD(TI, CH, LO, HI, V)                                                                   \
    {                                                                                                       \
        const int tile_ = blockIdx.x + (TI) * gridDim.x;                                                    \
        const int b_ = tile_ / tiles_per_img;                                                               \
        const int y0_ = (tile_ - b_ * tiles_per_img) * R;                                                   \
        _Pragma("unroll") for (int u = 0; u < PPT; ++u) {                                                   \
            int it_ = (LO) + u * NTHR + threadIdx.x;                                                         \
            it_ = it_ < (HI) ? it_ : (HI) - 1; /* clamped: branch-free, the store is predicated instead */  \
            const int c4_ = it_ % C4, pl_ = it_ / C4;                                                       \
            const int pr_ = pl_ / N, x_ = pl_ - pr_ * N;                                                    \
            int gy_ = y0_ - P + pr_;                                                                        \
            gy_ = gy_ < 0 ? gy_ + N : (gy_ >= N ? gy_ - N : gy_);                                           \
            V[u] = *reinterpret_cast<const f32x4 *>(                                                        \
                &a.in[(((size_t)b_ * N + gy_) * N + x_) * CIN + (CH) * CC + c4_ * 4]);                      \
        }                                                                                                   \
    }
#define QGX_PATCH_STORE(BUF, LO, HI, V)                                                                     \
    {                                                                                                       \
        _Pragma("unroll") for (int u = 0; u < PPT; ++u) {                                                   \
            const int it_ = (LO) + u * NTHR + threadIdx.x;                                                   \
            if (it_ < (HI)) {                                                                               \
                const int c4_ = it_ % C4, pl_ = it_ / C4;                                                   \
                *reinterpret_cast<f32x4 *>(&(BUF)[pl_ * STRIDE + c4_ * 4]) = V[u];                          \
            }                                                                                               \
        }                                                                                                   \
    }
#define QGX_W_LOAD(CH, SL, V)                                                                               \
    {                                                                                                       \
        const f32x4 *src_ = reinterpret_cast<const f32x4 *>(a.w) + ((size_t)(CH) * NSL + (SL)) * WF4;       \
        _Pragma("unroll") for (int u = 0; u < WPT; ++u) {                                                   \
            const int it_ = u * NTHR + threadIdx.x;                                                          \
            V[u] = src_[it_ < WF4 ? it_ : WF4 - 1];                                                         \
        }                                                                                                   \
    }
#define QGX_W_STORE(BUF, V)                                                                                 \
    {                                                                                                       \
        _Pragma("unroll") for (int u = 0; u < WPT; ++u) {                                                   \
            const int it_ = u * NTHR + threadIdx.x;                                                          \
            if (it_ < WF4) reinterpret_cast<f32x4 *>(BUF)[it_] = V[u];                                      \
        }                                                                                                   \
    }

    if (n_my == 0) return;
    // ---- prologue: first chunk's patch and first weight slice, synchronously
    {
        f32x4 pv[PPT];
        for (int lo = 0; lo < PF4; lo += PPT * NTHR) {
            const int hi = lo + PPT * NTHR < PF4 ? lo + PPT * NTHR : PF4;
            QGX_PATCH_LOAD(0, 0, lo, hi, pv)
            QGX_PATCH_STORE(lds0, lo, hi, pv)
        }
        f32x4 wv[WPT];
        QGX_W_LOAD(0, 0, wv)
        QGX_W_STORE(wlds0, wv)
    }
    __syncthreads();

    int py[MT], px[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int tile = wave + NW * mt;
        if (tile >= ntiles) tile = wave % ntiles;
        const int p = tile * 32 + li;
        py[mt] = p / N;
        px[mt] = p - py[mt] * N;
    }
    f32x16 acc[MT][NT];
    int cur_p = 0, cur_w = 0;
    for (int ti = 0; ti < n_my; ++ti) {
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch == 0) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
            }
            // the chunk after this one (possibly the first chunk of the next tile)
            const int nch = ch + 1 < NCH ? ch + 1 : 0;
            const int nti = ch + 1 < NCH ? ti : ti + 1;
            const bool have_next_chunk = nti < n_my;
            for (int sl = 0; sl < NSL; ++sl) {
                // ---- prefetch into registers (consumed after the K loop of this stage)
                f32x4 wv[WPT], pv[PPT];
                const bool last_stage = !have_next_chunk && sl == NSL - 1;
                // (always issued, from a valid dummy source on the very last stage: no branch around loads)
                {
                    const int wch = sl + 1 < NSL ? ch : (have_next_chunk ? nch : ch);
                    const int wsl = sl + 1 < NSL ? sl + 1 : (have_next_chunk ? 0 : sl);
                    QGX_W_LOAD(wch, wsl, wv)
                }
                const int plo = sl * PSH, phi = (sl + 1) * PSH < PF4 ? (sl + 1) * PSH : PF4;
                QGX_PATCH_LOAD(have_next_chunk ? nti : ti, have_next_chunk ? nch : ch, plo, phi, pv)

                // ---- K loop over the TPS taps of this slice; operands from LDS, pipelined one step ahead
                const float *patch = lds0 + cur_p * patch_floats;
                const float *wl = wlds0 + cur_w * WSL + h * COUTP * 4 + li * 4;
                const int tap0 = sl * TPS;
                int ky = tap0 / KS, kx = tap0 - ky * KS;
                int aoff[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    int col = px[mt] + kx - P;
                    col = col < 0 ? col + N : (col >= N ? col - N : col);
                    aoff[mt] = ((py[mt] + ky) * N + col) * STRIDE + 4 * h;
                }
                float4 An[MT], Bn[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) Bn[nt] = *reinterpret_cast<const float4 *>(wl + nt * 128);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff[mt]]);
                for (int tl = 0; tl < TPS; ++tl) {
                    const bool last_tap = tl == TPS - 1;
                    int nkx = kx + 1, nky = ky;
                    if (nkx == KS) { nkx = 0; ++nky; }
                    int aoff_n[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        int col = px[mt] + nkx - P;
                        col = col < 0 ? col + N : (col >= N ? col - N : col);
                        aoff_n[mt] = last_tap ? aoff[mt] : ((py[mt] + nky) * N + col) * STRIDE + 4 * h;
                    }
                    const float *wl_t = wl + (size_t)tl * G8 * 2 * COUTP * 4;
                    const float *wl_n = last_tap ? wl_t : wl_t + (size_t)G8 * 2 * COUTP * 4;
#pragma unroll
                    for (int g8 = 0; g8 < G8; ++g8) {
                        float4 A[MT], Bf[NT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) A[mt] = An[mt];
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) Bf[nt] = Bn[nt];
                        if (g8 + 1 < G8) {
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt)
                                Bn[nt] = *reinterpret_cast<const float4 *>(wl_t + (size_t)(g8 + 1) * 2 * COUTP * 4 + nt * 128);
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt)
                                An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff[mt] + (g8 + 1) * 8]);
                        } else {
#pragma unroll
                            for (int nt = 0; nt < NT; ++nt) Bn[nt] = *reinterpret_cast<const float4 *>(wl_n + nt * 128);
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt)
                                An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff_n[mt]]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                                for (int nt = 0; nt < NT; ++nt)
                                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                        (&A[mt].x)[e], (&Bf[nt].x)[e], acc[mt][nt], 0, 0, 0);
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) aoff[mt] = aoff_n[mt];
                    kx = nkx; ky = nky;
                }

                // ---- retire the prefetch into the idle LDS buffers
                if (!last_stage) QGX_W_STORE(wlds0 + (cur_w ^ 1) * WSL, wv)
                if (have_next_chunk) QGX_PATCH_STORE(lds0 + (cur_p ^ 1) * patch_floats, plo, phi, pv)

                if (sl == NSL - 1 && ch == NCH - 1) {
                    // ---- epilogue of this tile: bias + ReLU + BatchNorm affine, NHWC store
                    const int tile_g = blockIdx.x + ti * gridDim.x;
                    const int b = tile_g / tiles_per_img;
                    const int y0 = (tile_g - b * tiles_per_img) * R;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const int tile = wave + NW * mt;
                        if (tile >= ntiles) continue;
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const int co = nt * 32 + li;
                            const float bias = a.bias[co], sc = a.scale[co], sh = a.shift[co];
                            float *o = a.out + ((size_t)b * N * N + (size_t)y0 * N) * COUT + co;
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                                float vv = fmaxf(acc[mt][nt][r] + bias, 0.f);
                                o[(size_t)p * COUT] = vv * sc + sh;
                            }
                        }
                    }
                }
                __syncthreads();
                cur_w ^= 1;
            }
            cur_p ^= 1;
        }
    }
}
#undef QGX_PATCH_LOAD
#undef QGX_PATCH_STORE
#undef QGX_W_LOAD
#undef QGX_W_STORE

// out[p][c] = BN(ReLU(sum_s partial[s][p][c] + bias[c])): deterministic split-K combine (fixed order)
template <int COUT>
__global__ void k_conv_reduce(const float *partial, int nsplit, size_t npix_total, const float *bias,
                              const float *scale, const float *shift, float *out) {
    const size_t n4 = npix_total * COUT / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)((i * 4) % COUT);
        float4 v = reinterpret_cast<const float4 *>(partial)[i];
        for (int s2 = 1; s2 < nsplit; ++s2) {
            const float4 w = reinterpret_cast<const float4 *>(partial)[(size_t)s2 * n4 + i];
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
        float4 o;
        o.x = fmaxf(v.x + bias[c + 0], 0.f) * scale[c + 0] + shift[c + 0];
        o.y = fmaxf(v.y + bias[c + 1], 0.f) * scale[c + 1] + shift[c + 1];
        o.z = fmaxf(v.z + bias[c + 2], 0.f) * scale[c + 2] + shift[c + 2];
        o.w = fmaxf(v.w + bias[c + 3], 0.f) * scale[c + 3] + shift[c + 3];
        reinterpret_cast<float4 *>(out)[i] = o;
    }
}

// ---- last layer (32 -> n_out <= 2, 3x3): VALU kernel ---------------------------------------------
// Two output channels would fill 2 of 32 MFMA columns; on the vector ALUs the 288x2 dot products per
// pixel run at full useful rate: one thread per pixel, weights broadcast from scalar registers.

// PARTS = 4 (single-row tiles of 64 pixels, i.e. one or two members at 64 x 64): the four waves split the input
// channels of the same 64 pixels and combine through LDS — a 4x shorter dependent FMA chain per thread
template <int CIN, int KS, int PARTS = 1>
__global__ __launch_bounds__(256) void k_conv_last(ConvArgs a, LastWeights lw) {
    constexpr int P = KS / 2, STRIDE = CIN + 4, C4 = CIN / 4;
    float *patch = reinterpret_cast<float *>(conv_smem);
    const int N = a.N, R = a.R;
    const int tiles_per_img = N / R;
    const int b = blockIdx.x / tiles_per_img;
    const int y0 = (blockIdx.x - b * tiles_per_img) * R;
    const int PR = R + KS - 1;
    for (int it = threadIdx.x; it < PR * N * C4; it += 256) {
        const int c4 = it % C4, pl = it / C4;
        const int pr = pl / N, x = pl - pr * N;
        int gy = y0 - P + pr;
        gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
        *reinterpret_cast<float4 *>(&patch[pl * STRIDE + c4 * 4]) =
            *reinterpret_cast<const float4 *>(&a.in[(((size_t)b * N + gy) * N + x) * CIN + c4 * 4]);
    }
    __syncthreads();
    const float *w = lw.w;
    const int part = PARTS > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;   // wave-uniform
    constexpr int CPP = C4 / PARTS;                    // float4 channel groups per part
    float *red = patch + PR * N * STRIDE;              // PARTS > 1: [part][pixel][2]
    for (int p = PARTS > 1 ? (threadIdx.x & 63) : threadIdx.x; p < R * N; p += PARTS > 1 ? 64 : 256) {
        const int py = p / N, px = p - py * N;
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                int col = px + kx - P;
                col = col < 0 ? col + N : (col >= N ? col - N : col);
                const float *src = &patch[((py + ky) * N + col) * STRIDE + part * CPP * 4];
                const float *wt = w + ((ky * KS + kx) * CIN + part * CPP * 4) * 2;
#pragma unroll
                for (int c4 = 0; c4 < CPP; ++c4) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + c4 * 4);
                    acc0 = fmaf(v.x, wt[(c4 * 4 + 0) * 2], acc0); acc1 = fmaf(v.x, wt[(c4 * 4 + 0) * 2 + 1], acc1);
                    acc0 = fmaf(v.y, wt[(c4 * 4 + 1) * 2], acc0); acc1 = fmaf(v.y, wt[(c4 * 4 + 1) * 2 + 1], acc1);
                    acc0 = fmaf(v.z, wt[(c4 * 4 + 2) * 2], acc0); acc1 = fmaf(v.z, wt[(c4 * 4 + 2) * 2 + 1], acc1);
                    acc0 = fmaf(v.w, wt[(c4 * 4 + 3) * 2], acc0); acc1 = fmaf(v.w, wt[(c4 * 4 + 3) * 2 + 1], acc1);
                }
            }
        if constexpr (PARTS > 1) {
            red[(part * 64 + p) * 2] = acc0;
            red[(part * 64 + p) * 2 + 1] = acc1;
        } else {
            float *o = a.out + (size_t)b * a.out_channels * N * N + (size_t)y0 * N + p;
            o[0] = acc0 + a.bias[0];
            if (a.cout_real > 1) o[(size_t)N * N] = acc1 + a.bias[1];
        }
    }
    if constexpr (PARTS > 1) {
        __syncthreads();
        const int p = threadIdx.x >> 1, c = threadIdx.x & 1;
        if (p < R * N && c < a.cout_real) {
            float v = a.bias[c];
#pragma unroll
            for (int q = 0; q < PARTS; ++q) v += red[(q * 64 + p) * 2 + c];   // fixed order
            a.out[((size_t)b * a.out_channels + c) * N * N + (size_t)y0 * N + p] = v;
        }
    }
}

// out[0] = max |a - b|, out[1] = max |b| (float bits; calibration of the Winograd layer against the exact-f32 path)
__global__ void k_absdiff_max(const float *a, const float *b, size_t n, unsigned *out) {
    float d = 0.f, m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        d = fmaxf(d, abs_or_inf(a[i] - b[i]));
        m = fmaxf(m, abs_or_inf(b[i]));
    }
    for (int o = 32; o > 0; o >>= 1) { d = fmaxf(d, __shfl_down(d, o)); m = fmaxf(m, __shfl_down(m, o)); }
    if ((threadIdx.x & 63) == 0) { atomicMax(out, __float_as_uint(d)); atomicMax(out + 1, __float_as_uint(m)); }
}

// ---- host side ---------------------------------------------------------------------------
// hipFuncSetAttribute takes microseconds of host time; the single-member step is a chain of 5-15 us kernels whose
// launches the host has to keep ahead of: the dynamic-LDS cap of a kernel is raised once per kernel, device and host
// thread, not once per launch (rocprofv3: 14 launches / 116 us of kernels per step were taking 128 us of wall time)
int ensure_dynamic_lds(const void *kern, int bytes) {
    static thread_local std::unordered_map<const void *, int> seen[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto &m = seen[dev & 15];
    const auto it = m.find(kern);
    if (it != m.end() && it->second >= bytes) return QGX_OK;
    QGX_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    m[kern] = bytes;
    return QGX_OK;
}

static const int KSZ[8] = {5, 5, 3, 3, 3, 3, 3, 3};
static const int HID[7] = {128, 64, 32, 32, 32, 32, 32};

static int upf(float *&dst, const std::vector<float> &h) {
    QGX_HIP(hipMalloc((void **)&dst, h.size() * sizeof(float)));
    QGX_HIP(hipMemcpy(dst, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return QGX_OK;
}

// packed weights [k-group][coutp][8] for channel-chunk size cc (planar first layer: cc = cin)
static int pack_weights(const LayerHost &L, int li, const qgx_cnn_weights *w, bool planar_in, int cc, float *&dst) {
    const int cin = L.cin, cout = L.cout, ks = L.ks, T = ks * ks;
    const int ngroups = planar_in ? (T * cin + 7) / 8 : (cin / cc) * T * (cc / 8);
    std::vector<float> pw((size_t)ngroups * L.coutp * 8, 0.f);
    const float *W = w->conv_w[li];
    for (int g = 0; g < ngroups; ++g)
        for (int co = 0; co < cout; ++co)
            for (int e = 0; e < 8; ++e) {
                int tap, c;
                if (planar_in) {
                    const int kidx = 8 * g + e;
                    if (kidx >= T * cin) continue;
                    tap = kidx / cin; c = kidx % cin;
                } else {
                    const int g8n = cc / 8;
                    const int g8 = g % g8n, tt = (g / g8n) % T, chunk = g / (g8n * T);
                    tap = tt; c = chunk * cc + g8 * 8 + e;
                }
                const int ky = tap / ks, kx = tap % ks;
                pw[((size_t)g * L.coutp + co) * 8 + e] = W[(((size_t)co * cin + c) * ks + ky) * ks + kx];
            }
    return upf(dst, pw);
}

// conv_half.hpp weight layout [chunk][tap][part][h][cout][8] f16 (hi | lo), pre-scaled by 2^s with max|w| 2^s in [2^13, 2^14)
static int pack_half(LayerHost &L, int li, const qgx_cnn_weights *w, const float *cin_scale = nullptr) {
    const int cin = L.cin, cout = L.cout, T = L.ks * L.ks;
    const int coutp = ((cout + 31) / 32) * 32;         // the 32 -> 2 last layer is padded with zero rows
    const int nch = cin / 16;
    const float *W = w->conv_w[li];
    float mx = 0.f;
    for (int co = 0; co < cout; ++co)
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < T; ++t)
                mx = fmaxf(mx, fabsf(W[((size_t)co * cin + c) * T + t] * (cin_scale ? cin_scale[c] : 1.f)));
    int e = 0;
    if (mx > 0.f) { (void)frexpf(mx, &e); }             // mx = m 2^e, m in [0.5, 1)
    int sexp = 14 - e;
    sexp = sexp < -20 ? -20 : (sexp > 40 ? 40 : sexp);
    const float sc = ldexpf(1.f, sexp);
    std::vector<_Float16> pw((size_t)nch * T * 4 * coutp * 8, (_Float16)0.f);
    for (int ch = 0; ch < nch; ++ch)
        for (int t = 0; t < T; ++t)
            for (int j = 0; j < 2; ++j)
                for (int hh = 0; hh < 2; ++hh)
                    for (int co = 0; co < cout; ++co)
                        for (int e8 = 0; e8 < 8; ++e8) {
                            const int c = ch * 16 + hh * 8 + e8;
                            const float x = W[((size_t)co * cin + c) * T + t] * (cin_scale ? cin_scale[c] : 1.f) * sc;
                            const _Float16 xh = (_Float16)x;
                            const _Float16 v = j == 0 ? xh : (_Float16)(x - (float)xh);
                            pw[(((((size_t)ch * T + t) * 2 + j) * 2 + hh) * coutp + co) * 8 + e8] = v;
                        }
    void *&dst = cin_scale ? L.whF : L.wh;
    QGX_HIP(hipMalloc(&dst, pw.size() * sizeof(_Float16)));
    QGX_HIP(hipMemcpy(dst, pw.data(), pw.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    (cin_scale ? L.whF_unscale : L.wh_unscale) = ldexpf(1.f, -sexp);
    return QGX_OK;
}

// conv_wino.hpp weight layout [chunk][ky][p][part][h][cout][8] f16: U_p,ky(o, c) = sum_kx G[p][kx] w(o, c, ky, kx) of the
// Toom-Cook algorithm F(4, 5) with the points 0, +-1, +-2, +-1/2, infinity, evaluated in float64, pre-scaled per position by
// 2^s_p with max|U_p| 2^s_p in [2^13, 2^14), split into f16 hi / lo
static const double WINO_G[8][5] = {{-1, 0, 0, 0, 0},
                                    {-2. / 9, -2. / 9, -2. / 9, -2. / 9, -2. / 9},
                                    {-2. / 9, 2. / 9, -2. / 9, 2. / 9, -2. / 9},
                                    {1. / 90, 2. / 90, 4. / 90, 8. / 90, 16. / 90},
                                    {1. / 90, -2. / 90, 4. / 90, -8. / 90, 16. / 90},
                                    {32. / 45, 16. / 45, 8. / 45, 4. / 45, 2. / 45},
                                    {32. / 45, -16. / 45, 8. / 45, -4. / 45, 2. / 45},
                                    {0, 0, 0, 0, 1}};
[[maybe_unused]] static const float WINO_AT[4][8] = {{1, 1, 1, 1, 1, 1, 1, 0},
                                    {0, 1, -1, 2, -2, .5f, -.5f, 0},
                                    {0, 1, 1, 4, 4, .25f, .25f, 0},
                                    {0, 1, -1, 8, -8, .125f, -.125f, 1}};
static int pack_wino(LayerHost &L, int li, const qgx_cnn_weights *w, const float *cin_scale, int which) {
    const int cin = L.cin, cout = L.cout;
    if (cin != 128 || cout != 64 || L.ks != 5) return QGX_OK;
    const int nch = cin / 16;
    const float *W = w->conv_w[li];
    std::vector<double> U((size_t)8 * 5 * cout * cin);
    double mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < 8; ++p)
        for (int ky = 0; ky < 5; ++ky)
            for (int co = 0; co < cout; ++co)
                for (int c = 0; c < cin; ++c) {
                    double u = 0.0;
                    for (int kx = 0; kx < 5; ++kx)
                        u += WINO_G[p][kx] * (double)W[((size_t)co * cin + c) * 25 + ky * 5 + kx];
                    u *= cin_scale ? (double)cin_scale[c] : 1.0;
                    U[(((size_t)p * 5 + ky) * cout + co) * cin + c] = u;
                    mx[p] = fmax(mx[p], fabs(u));
                }
    std::vector<_Float16> pw((size_t)nch * 5 * 8 * 4 * cout * 8, (_Float16)0.f);
    for (int p = 0; p < 8; ++p) {
        int e = 0;
        if (mx[p] > 0.) (void)frexp(mx[p], &e);
        int sexp = 14 - e;
        sexp = sexp < -20 ? -20 : (sexp > 40 ? 40 : sexp);
        const double sc = ldexp(1.0, sexp);
        L.ww_unscale[which][p] = ldexpf(1.f, -sexp);
        for (int ch = 0; ch < nch; ++ch)
            for (int ky = 0; ky < 5; ++ky)
                for (int j = 0; j < 2; ++j)
                    for (int hh = 0; hh < 2; ++hh)
                        for (int co = 0; co < cout; ++co)
                            for (int e8 = 0; e8 < 8; ++e8) {
                                const int c = ch * 16 + hh * 8 + e8;
                                const float x = (float)(U[(((size_t)p * 5 + ky) * cout + co) * cin + c] * sc);
                                const _Float16 xh = (_Float16)x;
                                pw[((((((size_t)ch * 5 + ky) * 8 + p) * 2 + j) * 2 + hh) * cout + co) * 8 + e8] =
                                    j == 0 ? xh : (_Float16)(x - (float)xh);
                            }
    }
    QGX_HIP(hipMalloc(&L.ww[which], pw.size() * sizeof(_Float16)));
    QGX_HIP(hipMemcpy(L.ww[which], pw.data(), pw.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    return QGX_OK;
}

// first layer, f16x3 (k_convh_first): [step][part][h][cout][8], element j of lane half h in step s is
// (tap, channel) = (TPS s + TPF h + j / n_in, j % n_in); tap slots >= 25 hold zeros
static int pack_half_first(LayerHost &L, const qgx_cnn_weights *w) {
    const int nin = L.cin, cout = L.cout, T = 25;
    const int TPF = 8 / nin, TPS = 2 * TPF, nstep = (T + TPS - 1) / TPS;
    const float *W = w->conv_w[0];
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)cout * nin * T; ++i) mx = fmaxf(mx, fabsf(W[i]));
    int e = 0;
    if (mx > 0.f) (void)frexpf(mx, &e);
    int sexp = 14 - e;
    sexp = sexp < -20 ? -20 : (sexp > 40 ? 40 : sexp);
    const float sc = ldexpf(1.f, sexp);
    std::vector<_Float16> pw((size_t)nstep * 4 * cout * 8, (_Float16)0.f);
    for (int s = 0; s < nstep; ++s)
        for (int part = 0; part < 2; ++part)
            for (int hh = 0; hh < 2; ++hh)
                for (int co = 0; co < cout; ++co)
                    for (int j = 0; j < 8; ++j) {
                        const int tap = TPS * s + TPF * hh + j / nin, c = j % nin;
                        if (tap >= T) continue;
                        const float x = W[((size_t)co * nin + c) * T + tap] * sc;
                        const _Float16 xh = (_Float16)x;
                        pw[((((size_t)s * 2 + part) * 2 + hh) * cout + co) * 8 + j] = part == 0 ? xh : (_Float16)(x - (float)xh);
                    }
    QGX_HIP(hipMalloc(&L.whf, pw.size() * sizeof(_Float16)));
    QGX_HIP(hipMemcpy(L.whf, pw.data(), pw.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    L.whf_unscale = ldexpf(1.f, -sexp);
    return QGX_OK;
}

static int pack_layer(LayerHost &L, int li, const qgx_cnn_weights *w, bool planar_in) {
    const int cout = L.cout;
    L.coutp = ((cout + 31) / 32) * 32;
    int rc;
    if (planar_in) {
        if ((rc = pack_weights(L, li, w, true, L.cin, L.w))) return rc;
        if ((rc = pack_half_first(L, w))) return rc;
        {
            std::vector<float> o1(L.coutp, 1.f), z0(L.coutp, 0.f);
            if ((rc = upf(L.ones, o1)) || (rc = upf(L.zeros, z0))) return rc;
        }
    } else {
        if ((rc = pack_weights(L, li, w, false, 16, L.w))) return rc;
        if ((rc = pack_weights(L, li, w, false, 32, L.w32))) return rc;
        {      // LDS-operand layout for k_conv3
            const int cc = 16, cin = L.cin, ks = L.ks, T = ks * ks, g8n = cc / 8, nch = cin / cc;
            std::vector<float> pw((size_t)nch * T * g8n * 2 * L.coutp * 4, 0.f);
            for (int ch = 0; ch < nch; ++ch)
                for (int t = 0; t < T; ++t)
                    for (int g8 = 0; g8 < g8n; ++g8)
                        for (int hh = 0; hh < 2; ++hh)
                            for (int co = 0; co < cout; ++co)
                                for (int e = 0; e < 4; ++e) {
                                    const int c = ch * cc + g8 * 8 + hh * 4 + e;
                                    pw[(((((size_t)ch * T + t) * g8n + g8) * 2 + hh) * L.coutp + co) * 4 + e] =
                                        w->conv_w[li][((size_t)co * cin + c) * T + t];
                                }
            if ((rc = upf(L.wl16, pw))) return rc;
        }
        if (li < 7) {
            if ((rc = pack_half(L, li, w))) return rc;
            if (li == 1) {
                // fold layer 1's BatchNorm (alpha, beta' of its 128 output channels) into this layer
                const int cin = L.cin, T = L.ks * L.ks;
                std::vector<float> al(cin), be(cin), bf(L.coutp, 0.f);
                for (int c = 0; c < cin; ++c) {
                    const float invstd = 1.0f / sqrtf(w->bn_var[0][c] + w->bn_eps);
                    al[c] = w->bn_gamma[0][c] * invstd;
                    be[c] = w->bn_beta[0][c] - w->bn_mean[0][c] * al[c];
                }
                for (int co = 0; co < cout; ++co) {
                    double acc = w->conv_b[li][co];
                    for (int c = 0; c < cin; ++c)
                        for (int t = 0; t < T; ++t) acc += (double)w->conv_w[li][((size_t)co * cin + c) * T + t] * be[c];
                    bf[co] = (float)acc;
                }
                if ((rc = pack_half(L, li, w, al.data())) || (rc = upf(L.biasF, bf))) return rc;
                if ((rc = pack_wino(L, li, w, nullptr, 0)) || (rc = pack_wino(L, li, w, al.data(), 1))) return rc;
            }
        } else if ((rc = pack_half(L, li, w))) return rc;      // fused (layer 7, layer 8) pair
    }
    if (li == 7) {      // [tap][c][2] for the VALU last-layer kernel
        const int cin = L.cin, ks = L.ks;
        memset(L.wv_host, 0, sizeof(L.wv_host));
        for (int co = 0; co < cout && co < 4; ++co)
            for (int c = 0; c < cin; ++c)
                for (int t = 0; t < ks * ks; ++t)
                    L.wv_host[co / 2].w[((size_t)t * cin + c) * 2 + (co & 1)] = w->conv_w[li][((size_t)co * cin + c) * ks * ks + t];
    }
    std::vector<float> bias(L.coutp, 0.f), sc(L.coutp, 1.f), sh(L.coutp, 0.f);
    for (int co = 0; co < cout; ++co) {
        bias[co] = w->conv_b[li][co];
        if (li < 7) {
            // eval-mode BatchNorm as PyTorch evaluates it: alpha = gamma * invstd, y = x*alpha + (beta - mean*alpha)
            const float invstd = 1.0f / sqrtf(w->bn_var[li][co] + w->bn_eps);
            const float alpha = w->bn_gamma[li][co] * invstd;
            sc[co] = alpha;
            sh[co] = w->bn_beta[li][co] - w->bn_mean[li][co] * alpha;
        }
    }
    if ((rc = upf(L.bias, bias)) || (rc = upf(L.scale, sc)) || (rc = upf(L.shift, sh))) return rc;
    return QGX_OK;
}

int cnn_pack_net(NetHost &net, const qgx_cnn_weights *w) {
    net.n_in = w->n_in; net.n_out = w->n_out;
    if (net.flux()) { if (const int rc = fluxdiv_prepare()) return rc; }
    for (int li = 0; li < 8; ++li) {
        LayerHost &L = net.L[li];
        L.cin = li == 0 ? w->n_in : HID[li - 1];
        L.cout = li == 7 ? w->n_out : HID[li];
        L.ks = KSZ[li];
        if (const int rc = pack_layer(L, li, w, li == 0)) return rc;
    }
    return QGX_OK;
}
void cnn_free_net(NetHost &net) {
    for (LayerHost &L : net.L) L.free_device();
}

// Very small ensembles at 64 x 64 (a single member above all: BASELINE configs[1]) are chains of launch latencies; with 4-row
// tiles a member is 16 workgroups, with 2-row tiles 32 with half the K loop each (bit-identical: the tile shape does not enter
// the summation order).  Measured at one member: the 5x5 layer's split-K kernel + combine 23.6 -> 19.9 us, layer 3 12.1 -> 10.9.
static bool small_tiles(const qgx_generator *g, int B, int N) { return g->opt_small_tiles && N == 64 && B * 16 <= 64; }

int choose_rows(int N) {
    if (N <= 256 && 256 % N == 0) return 256 / N;     // 8 M-tiles
    if (N <= 384 && 384 % N == 0) return 384 / N;     // 12 M-tiles
    return 0;
}

template <int CIN, int COUT, int KS, int CC, bool PLANAR_IN, bool FINAL, int CSPLIT = 1, int OUTH = 0>
static int launch_conv(qgx_generator *g, int layer, const LayerHost &L, const float *in, float *out, int B,
                       int N, int cout_real, hipStream_t st) {
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    const int R = choose_rows(N);
    QGX_REQUIRE(R > 0 && N % R == 0, "generator: unsupported grid size N=%d", N);
    const int ntiles = R * N / 32;
    ConvArgs a = {};
    a.in = in; a.out = out; a.w = (!PLANAR_IN && CC == 32) ? L.w32 : L.w; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.N = N; a.R = R; a.cout_real = cout_real; a.npix_total = (size_t)B * N * N; a.ascale = g->opt_ascale;
    a.range = g->range_dev;
    constexpr int STRIDE = PLANAR_IN ? CIN : CC + 4;
    const size_t lds = (size_t)(R + KS - 1) * N * STRIDE * sizeof(float);
    QGX_REQUIRE(lds <= 160 * 1024, "generator: LDS patch %zu B too large for N=%d", lds, N);
    dim3 grid(B * (N / R), CSPLIT), block(256);
    if (ntiles <= 8) return launch_conv_kernel(k_conv<CIN, COUT, KS, CC, 2, PLANAR_IN, FINAL, CSPLIT, false, OUTH>, grid, block, lds, st, a);
    return launch_conv_kernel(k_conv<CIN, COUT, KS, CC, 3, PLANAR_IN, FINAL, CSPLIT, false, OUTH>, grid, block, lds, st, a);
}

// the exact-f32 first layer (n_in = 4 or 2 planar channels -> 128, 5x5): its output-channel tiles over `split` = 1, 2 or 4
// workgroups ("first_split"); outh = 2 (with split = 2): it stores the f16x3 activation layout for the 16-bit layers behind it
static int launch_conv_first(qgx_generator *g, const LayerHost &L, int n_in, int split, int outh, const float *in, float *out,
                             int B, int N, hipStream_t st) {
#define QGX_L1(SPLIT, OUTH)                                                                              \
    (n_in == 4 ? launch_conv<4, 128, 5, 4, true, false, SPLIT, OUTH>(g, 0, L, in, out, B, N, 128, st)    \
               : launch_conv<2, 128, 5, 2, true, false, SPLIT, OUTH>(g, 0, L, in, out, B, N, 128, st))
    if (outh == 2) return QGX_L1(2, 2);
    return split == 2 ? QGX_L1(2, 0) : (split == 4 ? QGX_L1(4, 0) : QGX_L1(1, 0));
#undef QGX_L1
}

// ---- small ensembles (few tiles): 4 M-tiles per workgroup (one per wave) and split-K over the
// 32-channel chunks, so that a single member still spreads over >= 128 workgroups -----------------
// rows per workgroup of the small-ensemble path: at most 4 M-tiles of 32 pixels (one per wave), as many as fit
static int rows_small(int N) {
    int best = 0;
    for (int R = 1; R <= N; ++R) {
        if (N % R || (R * N) % 32) continue;
        if (R * N / 32 > 4) break;
        best = R;
    }
    return best;
}
static bool small_ensemble(int B, int N) {
    const int R = choose_rows(N);
    return R > 0 && B * (N / R) <= 192 && rows_small(N) > 0 && rows_small(N) < R;   // crossover ~ B=13 at 64x64
}

template <int CIN, int COUT, int KS, int CC = 32>
static int launch_conv_small(qgx_generator *g, int layer, const LayerHost &L, const float *in, float *out, int B,
                             int N, hipStream_t st) {
    const int R = rows_small(N);                   // <= 4 M-tiles of 32 pixels
    const int nsplit = CIN >= 64 ? CIN / CC : 1;
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    const size_t npix = (size_t)B * N * N;
    if (nsplit > 1) { if (const int rc = generator_reserve_part(g, npix * COUT * nsplit)) return rc; }
    float *const part = g->work().part;
    ConvArgs a = {};
    a.in = in; a.out = nsplit > 1 ? part : out; a.w = CC == 32 ? L.w32 : L.w; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.N = N; a.R = R; a.cout_real = COUT; a.npix_total = npix;
    const size_t lds = (size_t)(R + KS - 1) * N * (CC + 4) * sizeof(float);
    dim3 grid(B * (N / R), nsplit), block(256);
    if (nsplit == 1) return launch_conv_kernel(k_conv<CIN, COUT, KS, CC, 1, false, false, 1, false>, grid, block, lds, st, a);
    if (const int rc = launch_conv_kernel(k_conv<CIN, COUT, KS, CC, 1, false, false, 1, true>, grid, block, lds, st, a)) return rc;
    const size_t n4 = npix * COUT / 4;
    return launch_conv_kernel(k_conv_reduce<COUT>, dim3((unsigned)((n4 + 255) / 256 > 1024 ? 1024 : (n4 + 255) / 256)), dim3(256), 0, st,
                              part, nsplit, npix, L.bias, L.scale, L.shift, out);
}

// ---- k_conv3 launcher -------------------------------------------------------------------------
template <int CIN, int COUT, int KS, int TPS, int CC = 16, int NW = 4>
static int launch_conv3(qgx_generator *g, int layer, const LayerHost &L, const float *in, float *out, int B,
                        int N, hipStream_t st, bool &done) {
    done = false;
    static_assert(CC == 16, "k_conv3's weights are packed for 16-channel chunks (LayerHost::wl16)");
    constexpr int T = KS * KS, NSL = T / TPS, NTc = (COUT + 31) / 32;
    constexpr size_t WSLB = (size_t)TPS * (CC / 8) * 2 * NTc * 32 * 4 * sizeof(float);
    // rows per tile: as k_conv (8 or 12 M-tiles; twice that with 8 waves), LDS = 2 patches + 2 weight slices
    int R = choose_rows(N);
    if (R == 0 || N % R) return QGX_OK;
    if (NW == 8) { if (N % (2 * R)) return QGX_OK; R *= 2; }
    const int ntiles = R * N / 32;
    const int PR = R + KS - 1;
    const size_t lds = (size_t)2 * PR * N * (CC + 4) * sizeof(float) + 2 * WSLB;
    if (lds > 160 * 1024 - 256) return QGX_OK;
    const int PF4 = PR * N * (CC / 4);
    const int ppt = (((PF4 + NSL - 1) / NSL) + NW * 64 - 1) / (NW * 64);
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    ConvArgs a = {};
    a.in = in; a.out = out; a.w = L.wl16; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.N = N; a.R = R; a.cout_real = COUT;
    const int total_tiles = B * (N / R);
    const int grid = persistent_grid(lds * 2 <= 160 * 1024 ? 512 : 256, total_tiles);
    void (*kern)(ConvArgs, int) = nullptr;
#define QGX_L3(MTV, PPTV) { kern = k_conv3<CIN, COUT, KS, CC, MTV, TPS, PPTV, NW>; }
    const int mtv = (ntiles + NW - 1) / NW <= 1 ? 1 : ((ntiles + NW - 1) / NW == 2 ? 2 : 3);
    if (mtv == 1) {
        if (ppt <= 2) QGX_L3(1, 2) else if (ppt <= 4) QGX_L3(1, 4) else return QGX_OK;
    } else if (ppt <= 2) { if (mtv == 2) QGX_L3(2, 2) else QGX_L3(3, 2) }
    else if (ppt <= 4) { if (mtv == 2) QGX_L3(2, 4) else QGX_L3(3, 4) }
    else if (ppt <= 8) { if (mtv == 2) QGX_L3(2, 8) else QGX_L3(3, 8) }
    else return QGX_OK;
#undef QGX_L3
    if (const int rc = launch_conv_kernel(kern, dim3(grid), dim3(NW * 64), lds, st, a, total_tiles)) return rc;
    done = true;
    return QGX_OK;
}

// hidden layers: k_conv3 (LDS-only operands, prefetched staging) where it measured faster (CIN <= 64 at
// 64x64: -8..-13 %; the 128->64 5x5 layer ties), else the one-shot k_conv.  "v3" option: -1 auto, 0 off,
// 1 = 4 waves, weight slice per tap row; 2 = 4 waves, slice per chunk; 6 / 7 = the same with 8 waves and
// double-height tiles.  Auto: 8 waves (slice per tap row for CIN = 32, per chunk for CIN = 64), falling
// back to 4 waves and then to k_conv when the LDS budget does not fit.
template <int CIN, int COUT, int KS>
static int conv_hidden(qgx_generator *g, int layer, const LayerHost &L, const float *in, float *out, int B,
                       int N, hipStream_t st) {
    if (g->opt_small && small_ensemble(B, N)) {
        // wide layers: split K per 16-channel chunk (8 / 4 partial sums) so that a single member still spreads
        // over >= 128 workgroups; the same split for every small ensemble, so that results do not depend
        // on the member count within this kernel family
        return launch_conv_small<CIN, COUT, KS, CIN >= 64 ? 16 : 32>(g, layer, L, in, out, B, N, st);
    }
    bool done = false;
    int rc = QGX_OK;
    const int v3 = g->opt_v3;
    if (v3 < 0) {
        if (CIN <= 64) {
            rc = CIN == 64 ? launch_conv3<CIN, COUT, KS, KS * KS, 16, 8>(g, layer, L, in, out, B, N, st, done)
                           : launch_conv3<CIN, COUT, KS, KS, 16, 8>(g, layer, L, in, out, B, N, st, done);
            if (!rc && !done) rc = launch_conv3<CIN, COUT, KS, KS>(g, layer, L, in, out, B, N, st, done);
        }
    } else if (v3 == 1) rc = launch_conv3<CIN, COUT, KS, KS>(g, layer, L, in, out, B, N, st, done);
    else if (v3 == 2) rc = launch_conv3<CIN, COUT, KS, KS * KS>(g, layer, L, in, out, B, N, st, done);
    else if (v3 == 6) rc = launch_conv3<CIN, COUT, KS, KS, 16, 8>(g, layer, L, in, out, B, N, st, done);
    else if (v3 == 7) rc = launch_conv3<CIN, COUT, KS, KS * KS, 16, 8>(g, layer, L, in, out, B, N, st, done);
    if (rc || done) return rc;
    if (g->opt_cc == 32) return launch_conv<CIN, COUT, KS, 32, false, false>(g, layer, L, in, out, B, N, COUT, st);
    return launch_conv<CIN, COUT, KS, 16, false, false>(g, layer, L, in, out, B, N, COUT, st);
}

// rows per workgroup of the VALU last layer
static int last_rows(const qgx_generator *g, int B, int N) {
    int R = choose_rows(N);
    if (g->opt_small && R > 0 && B * (N / R) <= 192) R = 1;      // small ensembles: one row per workgroup
    else if (R > 2 && N % 2 == 0) R = 2;                         // 37-55 KB of LDS: 2-4 workgroups per CU hide the
                                                                 // load -> barrier -> compute -> store chain (-10..-20 %)
    if (g->opt_last_rows > 0 && N % g->opt_last_rows == 0) R = g->opt_last_rows;
    return R;
}
static size_t last_lds_bytes(int R, int N) {
    const bool split = R * N == 64;                        // one wave of pixels: the waves split the channels
    return (size_t)(R + 2) * N * 36 * sizeof(float) + (split ? 4 * 64 * 2 * sizeof(float) : 0);
}

static int launch_conv_last(qgx_generator *g, const LayerHost &L, const float *in, float *out, int B, int N,
                            int n_out, hipStream_t st) {
    const int R = last_rows(g, B, N);
    QGX_REQUIRE(R > 0 && N % R == 0, "generator: unsupported grid size N=%d", N);
    ProfScope prof;
    if (const int prc = prof.begin(g, 7, st)) return prc;
    const bool split = R * N == 64;
    const size_t lds = last_lds_bytes(R, N);
    QGX_REQUIRE(lds <= 160 * 1024, "generator: LDS patch %zu B too large for N=%d", lds, N);
    // two accumulators per thread, and two channels of weights are 2.3 KB of kernel arguments (the limit is 4 KB): the four
    // flux channels of a flux-form net are two launches, each writing its channel pair of the (B, 4, N, N) output
    for (int c0 = 0; c0 < n_out; c0 += 2) {
        ConvArgs a = {};
        a.in = in; a.out = out + (size_t)c0 * N * N; a.w = nullptr; a.bias = L.bias + c0; a.scale = L.scale; a.shift = L.shift;
        a.N = N; a.R = R; a.cout_real = n_out - c0 < 2 ? n_out - c0 : 2; a.out_channels = n_out;
        if (const int rc = launch_conv_kernel(split ? k_conv_last<32, 3, 4> : k_conv_last<32, 3>, dim3(B * (N / R)), dim3(256), lds, st,
                                              a, L.wv_host[c0 / 2])) return rc;
    }
    return QGX_OK;
}

// ---- 16-bit matrix-core path (conv_half.hpp) ------------------------------------------------------
// rows per tile of k_convh2 (4 waves x MT M-tiles of 32 pixels), 0 when the grid size has no specialisation
static int rows_h2(int N) {
    switch (N) {
        case 32: return 8;
        case 48: return 8;
        case 64: return 4;
        case 96: return 4;
        case 128: return 2;
        default: return 0;
    }
}
// with the split-K variant for single members the 16-bit path wins at every ensemble size on the grids
// k_convh2 is specialised for, so it is always taken there ("half_min_tiles" = 1; raise it to send small
// ensembles to the exact-f32 split-K kernels)
static bool half_path_ok(const qgx_generator *g, int B, int N) {
    // f16x3 on the grids k_convh2 is specialised for (each a whole number of its row tiles), exact f32 everywhere else
    const int R = rows_h2(N);
    if (g->opt_precision != 3 || R <= 0) return false;
    return B * (N / R) >= g->opt_half_min_tiles;
}

// the fields every f16x3 hidden-layer launcher fills alike
static ConvHArgs convh_args(const qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, bool outf32, int N, int R) {
    ConvHArgs a = {};
    a.in = in; a.out = out; a.w = L.wh; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.unscale = L.wh_unscale / g->opt_ascale; a.ascale = outf32 ? 1.f : g->opt_ascale;
    a.range = g->range_dev; a.range_bit = 1u << layer;
    a.N = N; a.R = R;
    a.stamps = layer == g->stamp_layer ? g->stamps : nullptr;
    return a;
}

// f16x3 hidden layers at the grid sizes with a compile-time specialisation (k_convh2; 2 workgroups per CU
// where the LDS budget allows)
template <int CIN, int COUT, int KS, bool OUTF32, int NN, int MT>
static int launch_convh2_n(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B,
                           hipStream_t st) {
    constexpr int TPS = KS == 5 ? 5 : 9;
    constexpr int R = 4 * MT * 32 / NN, PR = R + KS - 1, PW = NN + 2 * (KS / 2);
    constexpr bool WDB = KS == 3;                                // double-buffered weight slice (3x3 layers)
    constexpr size_t lds = (size_t)PR * PW * 80 + (size_t)(WDB ? 2 : 1) * TPS * 4 * COUT * 16 + 3 * COUT * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS");
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    ConvHArgs a = convh_args(g, layer, L, in, out, OUTF32, NN, R);
    a.prio_alt = KS == 5 ? g->opt_prio_alt : (g->opt_prio_alt == 3 ? 3 : 0);      // measured: -2 % on the 5x5 layer, nothing on the 3x3 layers (3: by phase)
    const int total_tiles = B * (NN / R);
    const int grid = persistent_grid(g->opt_h2_grid > 0 ? g->opt_h2_grid : (lds * 2 <= 160 * 1024 ? 512 : 256), total_tiles);
    constexpr bool TWO = lds * 2 <= 160 * 1024 && MT == 2;        // two workgroups per CU: <= 256 registers
    auto kern = g->opt_pair && KS == 3 ? k_convh2<CIN, COUT, KS, NN, MT, TPS, OUTF32, WDB, TWO, KS == 3>
                                        : k_convh2<CIN, COUT, KS, NN, MT, TPS, OUTF32, WDB, TWO, false>;
    return launch_conv_kernel(kern, dim3(grid), dim3(256), lds, st, a, total_tiles);
}

// single members: split K over the 16-channel chunks (k_convh2<PART> + k_convh_reduce), so that the wide
// layers spread over >= 64 workgroups
template <int CIN, int COUT, int KS, bool OUTF32, int NN, int MT>
static int launch_convh2_part_n(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B,
                                hipStream_t st) {
    constexpr int TPS = KS == 5 ? 5 : 9, NCH = CIN / 16;
    constexpr int R = 4 * MT * 32 / NN, PR = R + KS - 1, PW = NN + 2 * (KS / 2);
    constexpr bool WDB = KS == 3;
    constexpr size_t lds = (size_t)PR * PW * 80 + (size_t)(WDB ? 2 : 1) * TPS * 4 * COUT * 16 + 3 * COUT * sizeof(float);
    constexpr int nsplit = NCH >= 8 ? 8 : NCH;
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    const size_t npix = (size_t)B * NN * NN;
    if (const int rc = generator_reserve_part(g, npix * COUT * nsplit)) return rc;
    float *const part = g->work().part;
    ConvHArgs a = convh_args(g, layer, L, in, part, OUTF32, NN, R);
    a.npix_total = npix; a.stamps = nullptr;
    const int total_tiles = B * (NN / R);
    constexpr bool TWO = lds * 2 <= 160 * 1024 && MT == 2;
    if (const int rc = launch_conv_kernel(k_convh2<CIN, COUT, KS, NN, MT, TPS, OUTF32, WDB, TWO, false, true>, dim3(total_tiles, nsplit),
                                          dim3(256), lds, st, a, total_tiles)) return rc;
    const size_t n = npix * (COUT / 8);
    return launch_conv_kernel(k_convh_reduce<COUT, OUTF32>, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, st,
                              part, nsplit, npix, L.bias, L.scale, L.shift, a.unscale, a.ascale, out, a.range, a.range_bit);
}

template <int CIN, int COUT, int KS, bool OUTF32>
static int launch_convh2_part(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B, int N,
                              hipStream_t st, bool &done) {
    done = true;
    switch (N) {
        case 32: return launch_convh2_part_n<CIN, COUT, KS, OUTF32, 32, 2>(g, layer, L, in, out, B, st);
        case 48: return launch_convh2_part_n<CIN, COUT, KS, OUTF32, 48, 3>(g, layer, L, in, out, B, st);
        // (half-height tiles for the smallest ensembles: 32 instead of 16 workgroups per member and split — small_tiles())
        case 64: return small_tiles(g, B, 64) && B == 1      // (at 4 members the 5x5 layer's 8 splits x 128 tiles are slower)
                            ? launch_convh2_part_n<CIN, COUT, KS, OUTF32, 64, 1>(g, layer, L, in, out, B, st)
                                              : launch_convh2_part_n<CIN, COUT, KS, OUTF32, 64, 2>(g, layer, L, in, out, B, st);
        case 96: return launch_convh2_part_n<CIN, COUT, KS, OUTF32, 96, 3>(g, layer, L, in, out, B, st);
        case 128: return launch_convh2_part_n<CIN, COUT, KS, OUTF32, 128, 2>(g, layer, L, in, out, B, st);
        default: done = false; return QGX_OK;
    }
}

// the 5x5 layer as ONE 8-wave workgroup per CU (R = 8 rows at 64 x 64: row halo 1.5x instead of 2x, half the
// weight traffic, double-buffered weight slice, 7 + 3 prefetch registers per thread)
template <int NN, int MT, int TW = NN>
static int launch_convh2_w8(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B, hipStream_t st) {
    constexpr int CIN = 128, COUT = 64, KS = 5, TPS = 5, NW = 8;
    constexpr int R = NW * MT * 32 / TW, PR = R + KS - 1, PW = TW + 4;
    constexpr size_t lds = (size_t)PR * PW * 80 + (size_t)2 * TPS * 4 * COUT * 16 + 3 * COUT * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS");
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    ConvHArgs a = convh_args(g, layer, L, in, out, false, NN, R);
    const int total_tiles = B * (NN / R) * (NN / TW);
    return launch_conv_kernel(k_convh2<CIN, COUT, KS, NN, MT, TPS, false, true, false, false, false, NW, TW>,
                              dim3(persistent_grid(256, total_tiles)), dim3(NW * 64), lds, st, a, total_tiles);
}

// the 3x3 layers in the same 8-wave shape (64 x 64)
template <int CIN, bool OUTF32, int NN = 64, int TW = NN, int NW = 8>
static int launch_convh2_w8_3x3(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B, hipStream_t st) {
    constexpr int COUT = 32, KS = 3, MT = 2, TPS = 9;
    constexpr int R = NW * MT * 32 / TW, PR = R + KS - 1, PW = TW + 2;
    constexpr size_t lds = (size_t)PR * PW * 80 + (size_t)2 * TPS * 4 * COUT * 16 + 3 * COUT * sizeof(float);
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    ConvHArgs a = convh_args(g, layer, L, in, out, OUTF32, NN, R);
    const int total_tiles = B * (NN / R) * (NN / TW);
    return launch_conv_kernel(k_convh2<CIN, COUT, KS, NN, MT, TPS, OUTF32, true, false, true, false, NW, TW>,
                              dim3(persistent_grid(256, total_tiles)), dim3(NW * 64), lds, st, a, total_tiles);
}

template <int CIN, int COUT, int KS, bool OUTF32>
static int launch_convh2(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B, int N,
                         hipStream_t st, bool &done) {
    done = true;
    if constexpr (KS == 3 && COUT == 32) {
        if ((g->opt_h2_w8 & 2) && g->opt_pair && N == 64 && B * 8 >= 256) return launch_convh2_w8_3x3<CIN, OUTF32>(g, layer, L, in, out, B, st);
        // 96 = 3 x 32: tiles of 16 rows x 32 columns give the 3x3 layers the two-M-tiles-per-wave 8-wave shape too
        if ((g->opt_h2_w8 & 2) && g->opt_pair && g->opt_h2_x96 && N == 96 && B * 18 >= 256) {
            // 16 x 32 tiles on 8 waves (18 per member) or 12 x 32 tiles on 6 waves (24 per member): by rounds x cost per tile, as the
            // Winograd layer's shapes (launch_convw); a 6-wave tile costs 0.85 of an 8-wave one (measured: 32 members 32.4 -> 30.4 us
            // per 32 -> 32 layer, 16 members 23.0 -> 21.1, 64 members 52.1 / 52.2)
            const int r16 = (B * 18 + 255) / 256, r12 = (B * 24 + 255) / 256;
            const bool rows12 = g->opt_h2_rows96 == 12 || (g->opt_h2_rows96 == 0 && 0.85 * r12 < 1.0 * r16);
            return rows12 ? launch_convh2_w8_3x3<CIN, OUTF32, 96, 32, 6>(g, layer, L, in, out, B, st)
                          : launch_convh2_w8_3x3<CIN, OUTF32, 96, 32>(g, layer, L, in, out, B, st);
        }
    }
    if constexpr (KS == 5 && CIN == 128) {
        // one 8-wave workgroup per CU once its double-height tiles fill the CUs: -5.5 % at 64 x 64, -3.5 % at
        // 32 x 32; the three-tile-per-wave shapes of 96 / 48 spill at 256 registers (+40 %), 128 ties
        if (g->opt_h2_w8) {
            if (N == 64 && B * 8 >= 256)
                return g->opt_h2_tw32 ? launch_convh2_w8<64, 2, 32>(g, layer, L, in, out, B, st) : launch_convh2_w8<64, 2>(g, layer, L, in, out, B, st);
            if (N == 32 && B * 2 >= 256) return launch_convh2_w8<32, 2>(g, layer, L, in, out, B, st);
            // 96 = 3 x 32: tiles of 16 rows x 32 columns keep the two-M-tiles-per-wave shape
            if (N == 96 && B * 18 >= g->opt_h2_w8_min96) return launch_convh2_w8<96, 2, 32>(g, layer, L, in, out, B, st);
        }
    }
    switch (N) {
        case 32: return launch_convh2_n<CIN, COUT, KS, OUTF32, 32, 2>(g, layer, L, in, out, B, st);
        case 48: return launch_convh2_n<CIN, COUT, KS, OUTF32, 48, 3>(g, layer, L, in, out, B, st);
        case 64: return small_tiles(g, B, 64) ? launch_convh2_n<CIN, COUT, KS, OUTF32, 64, 1>(g, layer, L, in, out, B, st)
                                              : launch_convh2_n<CIN, COUT, KS, OUTF32, 64, 2>(g, layer, L, in, out, B, st);
        case 96: return launch_convh2_n<CIN, COUT, KS, OUTF32, 96, 3>(g, layer, L, in, out, B, st);
        case 128: return launch_convh2_n<CIN, COUT, KS, OUTF32, 128, 2>(g, layer, L, in, out, B, st);
        default: done = false; return QGX_OK;
    }
}

// a 3x3 layer of the f16x3 path: half_path_ok admits only the grids k_convh2 is specialised for
template <int CIN, int COUT, bool OUTF32>
static int conv3x3_half(qgx_generator *g, int layer, const LayerHost &L, const void *in, void *out, int B, int N,
                        hipStream_t st) {
    bool done = false;
    if (const int rc = launch_convh2<CIN, COUT, 3, OUTF32>(g, layer, L, in, out, B, N, st, done)) return rc;
    QGX_REQUIRE(done, "generator: no f16x3 kernel for N=%d (half_path_ok admits only the specialised grids)", N);
    return QGX_OK;
}

// two fused 3x3 layers (k_convh_pair) on R-row strips of an NN x NN grid
template <int CINA, bool LAST, bool BOUTF32, int NN = 64, int R = 8>
static int launch_convh_pair(qgx_generator *g, int layerA, const LayerHost &LA, const LayerHost &LB, const void *in,
                             void *out, int B, int N, int n_out, hipStream_t st) {
    constexpr int PW = NN + 2;
    QGX_REQUIRE(N == NN, "generator: fused layer pairs compiled for N=%d", NN);
    constexpr size_t reg0 = (size_t)(R + 2) * PW * 144 > (size_t)(R + 4) * PW * 80 ? (size_t)(R + 2) * PW * 144 : (size_t)(R + 4) * PW * 80;
    constexpr size_t lds = reg0 + 3 * (9 * 4 * 32 * 16) + 2 * 96 * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS");
    ProfScope prof;
    if (const int prc = prof.begin(g, layerA, st)) return prc;
    ConvPairArgs a = {};
    a.in = in; a.out = out; a.wA = LA.wh; a.wB = LB.wh;
    a.biasA = LA.bias; a.scaleA = LA.scale; a.shiftA = LA.shift;
    a.biasB = LB.bias; a.scaleB = LB.scale; a.shiftB = LB.shift;
    a.unscaleA = LA.wh_unscale / g->opt_ascale; a.unscaleB = LB.wh_unscale / g->opt_ascale; a.ascale = g->opt_ascale;
    a.range = g->range_dev; a.range_bit = 1u << layerA;
    a.n_out = n_out;
    a.stamps = layerA == g->stamp_layer ? g->stamps : nullptr;
    const int total_tiles = B * (N / R);
    return launch_conv_kernel(k_convh_pair<CINA, NN, LAST, BOUTF32, R>, dim3(persistent_grid(256, total_tiles)), dim3(512), lds, st, a, total_tiles);
}

template <int NIN>
static int launch_convh_first(qgx_generator *g, const LayerHost &L, const float *in, void *out, int B, int N,
                              hipStream_t st, bool wino_next = false) {
    int R = choose_rows(N);
    QGX_REQUIRE(R > 0 && N % R == 0 && N % 4 == 0, "generator: unsupported grid size N=%d", N);
    // one 8-wave workgroup per CU with double-height tiles where two M-tiles per wave result (64 x 64, 32 x 32) and
    // the ensemble fills the CUs: of two co-resident 4-wave workgroups the older wins every issue arbitration and
    // the younger finishes 30 % later (global-clock stamps), and the 57 KB weight set is staged once per CU
    const bool w8 = g->opt_h2_w8 && R * N / 32 == 8 && N % (2 * R) == 0 && B * (N / (2 * R)) >= 256;
    if (w8) R *= 2;
    const bool half_rows = !w8 && small_tiles(g, B, N) && R % 2 == 0;      // one M-tile per wave (small_tiles())
    if (half_rows) R /= 2;
    const int nw = w8 ? 8 : 4;
    const int PR = R + 4, ntiles = R * N / 32;
    constexpr int nstep = NIN == 4 ? 7 : 4;
    const size_t lds = (size_t)nstep * 4 * 128 * 16 + (size_t)2 * PR * N * NIN * 4 + 3 * 128 * sizeof(float);
    const int ppt = (PR * NIN * (N / 4) + nw * 64 - 1) / (nw * 64);
    QGX_REQUIRE(lds <= 160 * 1024 - 256 && ppt <= 3 && (ntiles == 2 * nw || ntiles == 3 * nw || (half_rows && ntiles == nw)),
                "generator: 16-bit first layer unsupported for N=%d", N);
    ProfScope prof;
    if (const int prc = prof.begin(g, 0, st)) return prc;
    ConvHFirstArgs a = {};
    a.stamps = g->stamp_layer == 0 ? g->stamps : nullptr;
    a.in = in; a.out = out; a.w = L.whf; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.unscale = L.whf_unscale; a.ascale = g->opt_ascale; a.N = N; a.R = R;
    a.guard_mul = wino_next ? 16.f : 1.f;
    a.range = g->range_dev; a.range_bit = 1u;
    const int total_tiles = B * (N / R);
    const int grid = persistent_grid(lds * 2 <= 160 * 1024 ? 512 : 256, total_tiles);
    void (*kern)(ConvHFirstArgs, int) = nullptr;
#define QGX_LF(MTV, PPTV, NWV) { kern = k_convh_first<NIN, MTV, PPTV, NWV>; }
    if (half_rows) { if (ppt <= 2) QGX_LF(1, 2, 4) else QGX_LF(1, 3, 4) }
    else if (w8) { if (ppt <= 2) QGX_LF(2, 2, 8) else QGX_LF(2, 3, 8) }
    else if (ntiles == 8) { if (ppt <= 2) QGX_LF(2, 2, 4) else QGX_LF(2, 3, 4) }
    else { if (ppt <= 2) QGX_LF(3, 2, 4) else QGX_LF(3, 3, 4) }
#undef QGX_LF
    return launch_conv_kernel(kern, dim3(grid), dim3(nw * 64), lds, st, a, total_tiles);
}

// layer 2 as a 1-D Winograd convolution (conv_wino.hpp); use2: as k_convw2 where that kernel is built for the tile shape
template <int NN, int TW, int R>
static int launch_convw_n(qgx_generator *g, int layer, const LayerHost &L, int which, bool use2, const void *in, void *out, int B,
                          hipStream_t st) {
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    ConvWArgs a = {};
    a.in = in; a.out = out; a.w = L.ww[which]; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    for (int p = 0; p < 8; ++p) a.pscale[p] = L.ww_unscale[which][p] / g->opt_ascale;
    a.ascale = g->opt_ascale;
    a.range = g->range_dev; a.range_bit = 1u << layer;
    const int total_tiles = B * (NN / R) * (NN / TW);
    constexpr size_t lds = convw_lds_bytes(NN, TW, R);
    static_assert(lds <= 160 * 1024 - 256, "k_convw: LDS");
    if (use2) {
        bool done2 = false;
        const int rc2 = launch_convw2(NN, TW, R, a, total_tiles, st, &done2);
        if (rc2 || done2) return rc2;
    }
    return launch_conv_kernel(k_convw<NN, TW, R>, dim3(persistent_grid(256, total_tiles)), dim3(512), lds, st, a, total_tiles);
}
// tiles of 512 pixels: 8 x 64 (64 x 64, 128 x 128), 16 x 32 (96 x 96, 32 x 32); 16 x 16 at 48 x 48
static int wino_tiles(int B, int N) {
    switch (N) {
        case 32: return B * 2;
        case 48: return B * 9;
        case 64: return B * 8;
        case 96: return B * 18;
        case 128: return B * 32;
        default: return 0;
    }
}
static int wino_size_index(int N) {
    switch (N) { case 32: return 0; case 48: return 1; case 64: return 2; case 96: return 3; case 128: return 4; default: return -1; }
}
static bool wino_applies(const qgx_generator *g, const LayerHost &L, int which, int B, int N) {
    const int tiles = wino_tiles(B, N), si = wino_size_index(N);
    const bool on = g->opt_wino == 1 || (g->opt_wino == 2 && si >= 0 && g->auto_wino_n[si]);
    return on && L.ww[which] && tiles > 0 && tiles >= g->opt_wino_min_tiles;
}
// The Winograd layer's tile rows for B members at N x N: the full shape of wino_tiles() or, at every size but 48 x 48, a
// smaller one.  256 persistent workgroups take ceil(tiles / 256) rounds, so the shape is chosen by rounds x cost per tile:
// the small shape pays while the large one leaves CUs idle.  Measured (layer time in us):
//   64 x 64, 8-row tiles (8 per member) or 4-row tiles (16 per member, half the work each at a 2 x instead of 1.5 x row
//     halo), 8 / 4 rows: 8 members 65 / 44, 16: 69 / 50, 24: 74 / 87, 31: 80 / 92, 48: 139 / 134 -> 0.66 per tile
//   32 x 32, 16 x 32 tiles (2 per member) or 8 x 32 (4 per member): 32 / 64 members 63 -> 42 / 68 -> 49 us, 96 / 128 members
//     stay (73 / 85, 83 / 95)
//   128 x 128, 8 x 64 tiles (32 per member) or 4 x 64 (64 per member), as at 64 x 64: 2 / 4 members 67 -> 45 / 72 -> 53 us,
//     6 / 8 members stay (78 / 89, 86 / 97), 12 members 155 -> 143
//   96 x 96, 16 x 32 tiles (18 per member) or 12 x 32 (24 per member, 0.75 x the work each at a 1.33 x instead of 1.25 x row
//     halo): at 32 members 3 x 1.0 against 3 x 0.79 (measured 215 -> 171 us), at 24 members 2 x 1.0 against 3 x 0.79
//     (149 / 160 us), at 128 9 x 1.0 against 12 x 0.79 (690 / 749 us)
static int wino_rows(const qgx_generator *g, int B, int N) {
    if (N == 48) return 16;
    if (N == 96) {
        const int r16 = (B * 18 + 255) / 256, r12 = (B * 24 + 255) / 256;
        return g->opt_wino_rows96 == 12 || (g->opt_wino_rows96 == 0 && 0.79 * r12 < 1.0 * r16) ? 12 : 16;
    }
    const int full = N == 32 ? 16 : 8, tiles = wino_tiles(B, N);      // the half-height shape has twice the tiles
    const int rf = (tiles + 255) / 256, rh = (2 * tiles + 255) / 256;
    return g->opt_wino_rows64 == 4 || (g->opt_wino_rows64 == 0 && 0.66 * rh < 1.0 * rf) ? full / 2 : full;
}

// ---- the plan for layer 2 (the 128 -> 64, 5x5 layer) -----------------------------------------------------------------
// Everything about it that is decided BEFORE layer 1 is launched — layer 1's BatchNorm, its output layout and its range
// guard depend on it — and decided here only: cnn_forward_half and launch_convw carry the plan out,
// qgx_generator_layer2_kernel reports it.
struct Layer2Plan {
    bool fold = false;      // layer 1 stores its ReLU output (identity BatchNorm in the epilogue; 50 % exact zeros with the
                            //   shipped weights) and layer 2 uses the weights / bias with that BatchNorm folded in
    bool tiny = false;      // single members / tiny ensembles (fewer than "part_max_tiles" tiles): split K on the two wide layers,
                            //   and no 8-row pair kernel for (7, 8) (8 tiles of 512 pixels would leave 248 CUs idle)
    bool wino = false;      // the Winograd form runs (then layer 1's range guard covers its input transform too) ...
    int which = 0;          //   ... with these weights of LayerHost::ww: 0 plain, 1 folded
    int tw = 0, rows = 0;   //   ... on tiles of rows x tw pixels
    bool wino2 = false;     //   ... as k_convw2
    int kernel = 0;         // 0 exact-f32 MFMA, 1 the 25-tap f16x3 kernel, 2 its split-K form, 3 k_convw, 4 k_convw2
};
static Layer2Plan plan_layer2(const qgx_generator *g, const NetHost &net, int B, int N) {
    Layer2Plan p;
    const bool x3 = g->opt_precision == 3;
    p.fold = x3 && g->opt_first_h && g->opt_fold && net.L[1].whF;
    p.which = p.fold ? 1 : 0;
    const int r2 = rows_h2(N);
    if (!x3 || r2 <= 0) return p;
    p.tiny = B * (N / r2) < g->opt_part_max_tiles;
    p.wino = !p.tiny && g->opt_first_h && wino_applies(g, net.L[1], p.which, B, N);
    p.kernel = p.tiny ? 2 : 1;
    if (!p.wino) return p;
    p.rows = wino_rows(g, B, N);
    p.tw = N == 48 ? 16 : (N == 64 || N == 128 ? 64 : 32);
    p.wino2 = g->opt_wino2 && convw2_takes(N, p.tw, p.rows);
    p.kernel = p.wino2 ? 4 : 3;
    return p;
}

static int launch_convw(qgx_generator *g, int layer, const LayerHost &L, const Layer2Plan &p, const void *in, void *out, int B,
                        int N, hipStream_t st) {
#define QGX_LW(NN, TW, R) \
    if (N == NN && p.tw == TW && p.rows == R) return launch_convw_n<NN, TW, R>(g, layer, L, p.which, p.wino2, in, out, B, st);
    QGX_LW(32, 32, 8) QGX_LW(32, 32, 16) QGX_LW(48, 16, 16) QGX_LW(64, 64, 4) QGX_LW(64, 64, 8)
    QGX_LW(96, 32, 12) QGX_LW(96, 32, 16) QGX_LW(128, 64, 4) QGX_LW(128, 64, 8)
#undef QGX_LW
    QGX_REQUIRE(false, "generator: layer 1 was stored for the Winograd layer, which did not run (N=%d)", N);
}

// Layers 5-8 of the 16-bit path.  `pairs` bit 0: layers (5, 6), bit 1: layers (7, 8) as ONE launch of the pair kernel on R-row
// strips of an NN x NN grid (the intermediate activation stays in LDS), else as two kernels.  `cur` holds layer 4's output,
// `oth` takes a layer's output; which buffer ends up with which layer is what qgx_debug_read_act relies on.
template <int NN, int R>
static int layers_5_to_8(qgx_generator *g, const NetHost &net, int pairs, float *cur, float *oth, float *yc, int Bc, int N,
                         hipStream_t st) {
    int rc;
    if (pairs & 1) {
        if ((rc = launch_convh_pair<32, false, false, NN, R>(g, 4, net.L[4], net.L[5], cur, oth, Bc, N, 0, st))) return rc;
        std::swap(cur, oth);
    } else {
        if ((rc = conv3x3_half<32, 32, false>(g, 4, net.L[4], cur, oth, Bc, N, st))) return rc;
        if ((rc = conv3x3_half<32, 32, false>(g, 5, net.L[5], oth, cur, Bc, N, st))) return rc;
    }
    if (pairs & 2) return launch_convh_pair<32, true, false, NN, R>(g, 6, net.L[6], net.L[7], cur, yc, Bc, N, net.n_out, st);
    if ((rc = conv3x3_half<32, 32, true>(g, 6, net.L[6], cur, oth, Bc, N, st))) return rc;
    return launch_conv_last(g, net.L[7], oth, yc, Bc, N, net.n_out, st);
}

static int cnn_forward_half(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N,
                            hipStream_t st) {
    int rc;
    float *A = g->work().actA, *Bb = g->work().actB;
    // optional member sub-batches ("member_chunk"): all layers of one sub-batch before the next, so that the
    // inter-layer activations of a sub-batch can stay in the 256 MB Infinity Cache
    const int mc = g->opt_member_chunk > 0 && g->opt_member_chunk < B ? g->opt_member_chunk : B;
    for (int b0 = 0; b0 < B; b0 += mc) {
        const int Bc = B - b0 < mc ? B - b0 : mc;
        const float *xc = x + (size_t)b0 * net.n_in * N * N;
        float *yc = y + (size_t)b0 * net.n_out * N * N;
        const Layer2Plan p = plan_layer2(g, net, Bc, N);
        LayerHost L0 = net.L[0], L1 = net.L[1];
        if (p.fold) {
            L0.scale = L0.ones; L0.shift = L0.zeros;
            L1.wh = L1.whF; L1.wh_unscale = L1.whF_unscale; L1.bias = L1.biasF;
        }
        if (g->opt_first_h) {
            rc = net.n_in == 4 ? launch_convh_first<4>(g, L0, xc, A, Bc, N, st, p.wino)
                               : launch_convh_first<2>(g, L0, xc, A, Bc, N, st, p.wino);
        } else rc = launch_conv_first(g, net.L[0], net.n_in, 2, 2, xc, A, Bc, N, st);
        if (rc) return rc;
        bool done1 = false;
        if (p.tiny && (rc = launch_convh2_part<128, 64, 5, false>(g, 1, L1, A, Bb, Bc, N, st, done1))) return rc;
        if (!done1 && p.wino) {
            if ((rc = launch_convw(g, 1, L1, p, A, Bb, Bc, N, st))) return rc;
            done1 = true;
        }
        if (!done1 && (rc = launch_convh2<128, 64, 5, false>(g, 1, L1, A, Bb, Bc, N, st, done1))) return rc;
        QGX_REQUIRE(done1, "generator: no f16x3 kernel for N=%d", N);
        // the fused (7, 8) pair writes at most two channels: a flux-form net takes layer 7's kernel and the VALU last layer
        const int no78 = net.n_out <= 2 ? ~0 : ~2, tiny_no78 = net.n_out <= 2 ? ~0 : ~1;
        if (p.tiny) {
            // (local names: the 64-channel activation of layer 2 is in Bb; `cur` holds a layer's input, `oth` takes its output)
            float *cur = Bb, *oth = A;
            // Layers (3, 4), (5, 6) and (7, 8) each as ONE launch on 2-row strips ("tiny_pairs" bits 2, 1, 0): a single member is
            // a chain of launch latencies, and a strip's fixed costs — layer B's 36 KB of MFMA weights above all — are cheaper
            // than a kernel boundary there; for (3, 4) the one launch also replaces split-K and its combine kernel
            const int tp = N == 64 ? g->opt_tiny_pairs & tiny_no78 : 0;
            if (tp & 4) {
                if ((rc = launch_convh_pair<64, false, false, 64, 2>(g, 2, net.L[2], net.L[3], cur, oth, Bc, N, 0, st))) return rc;
                std::swap(cur, oth);
            } else {
                bool done2 = false;
                if ((rc = launch_convh2_part<64, 32, 3, false>(g, 2, net.L[2], cur, oth, Bc, N, st, done2))) return rc;
                if (!done2 && (rc = conv3x3_half<64, 32, false>(g, 2, net.L[2], cur, oth, Bc, N, st))) return rc;
                if ((rc = conv3x3_half<32, 32, false>(g, 3, net.L[3], oth, cur, Bc, N, st))) return rc;
            }
            if ((rc = layers_5_to_8<64, 2>(g, net, ((tp >> 1) & 1) | ((tp & 1) << 1), cur, oth, yc, Bc, N, st))) return rc;
            continue;
        }
        // 3x3 layers fused pairwise at 64 x 64; "fuse" bits: 1 = layers (5, 6), 2 = layers (7, 8), 4 = layers (3, 4) — the
        // 64-channel pair measured slower fused
        const int fuse = N == 64 ? g->opt_fuse & no78 : 0;
        if (fuse & 4) {
            if ((rc = launch_convh_pair<64, false, false>(g, 2, net.L[2], net.L[3], Bb, A, Bc, N, 0, st))) return rc;
        } else {
            if ((rc = conv3x3_half<64, 32, false>(g, 2, net.L[2], Bb, A, Bc, N, st))) return rc;
            if ((rc = conv3x3_half<32, 32, false>(g, 3, net.L[3], A, Bb, Bc, N, st))) return rc;
        }
        // here the activation is in A (fused pair) or Bb (two kernels)
        float *cur = (fuse & 4) ? A : Bb, *oth = (fuse & 4) ? Bb : A;
        if (fuse) {
            // (4-row strips for the pairs, as the Winograd layer's small shape, measured slower at 8 ... 48 members: 25.4 -> 30.8 us at
            // 16, 26.3 -> 47.4 at 24 — a strip's fixed costs, layer B's 36 KB of weights above all, do not halve with its rows)
            rc = layers_5_to_8<64, 8>(g, net, fuse & 3, cur, oth, yc, Bc, N, st);
        } else {
            // 96 x 96: the pair kernel on 4-row strips (a 6-row intermediate patch of 98 columns is 85 KB); "fuse96" bits as "fuse".
            // Every other grid: two kernels per pair
            const int fuse96 = N == 96 && Bc * 24 >= 256 ? g->opt_fuse96 & no78 : 0;
            rc = layers_5_to_8<96, 4>(g, net, fuse96 & 3, cur, oth, yc, Bc, N, st);
        }
        if (rc) return rc;
    }
    return QGX_OK;
}

// the eight convolutions: x planar (B,n_in,N,N) -> y planar (B,n_out,N,N)
static int cnn_convs(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N, hipStream_t st) {
    int rc;
    if (net.generic) return cnng_convs(g, net, x, y, B, N, st);      // any other architecture than the shipped one: conv_generic.hip
    if (half_path_ok(g, B, N)) return cnn_forward_half(g, net, x, y, B, N, st);
    float *A = g->work().actA, *Bb = g->work().actB;
    if ((rc = launch_conv_first(g, net.L[0], net.n_in, g->opt_first_split, 0, x, A, B, N, st))) return rc;
    // calibration runs record the largest stored activation of every layer (launch_absmax keeps a running maximum
    // in calib_dev[2 * layer + 1]: it updates word [1] of the pair it is given)
    auto rec = [&](int layer, const float *buf, int ch) {
        if (g->calib_dev) launch_absmax(buf, (size_t)B * N * N * ch, g->calib_dev + 2 * layer, st);
    };
    rec(0, A, 128);
    if ((rc = conv_hidden<128, 64, 5>(g, 1, net.L[1], A, Bb, B, N, st))) return rc;
    rec(1, Bb, 64);
    if ((rc = conv_hidden<64, 32, 3>(g, 2, net.L[2], Bb, A, B, N, st))) return rc;
    rec(2, A, 32);
    if ((rc = conv_hidden<32, 32, 3>(g, 3, net.L[3], A, Bb, B, N, st))) return rc;
    rec(3, Bb, 32);
    if ((rc = conv_hidden<32, 32, 3>(g, 4, net.L[4], Bb, A, B, N, st))) return rc;
    rec(4, A, 32);
    if ((rc = conv_hidden<32, 32, 3>(g, 5, net.L[5], A, Bb, B, N, st))) return rc;
    rec(5, Bb, 32);
    if ((rc = conv_hidden<32, 32, 3>(g, 6, net.L[6], Bb, A, B, N, st))) return rc;
    rec(6, A, 32);
    // (the MFMA form of the last layer is instantiated for two output channels: a flux-form net takes the VALU kernel)
    if (g->opt_last_valu || net.flux()) rc = launch_conv_last(g, net.L[7], A, y, B, N, net.n_out, st);
    else rc = launch_conv<32, 2, 3, 16, false, true>(g, 7, net.L[7], A, y, B, N, net.n_out, st);
    if (rc) return rc;
    return QGX_OK;
}

// AndrewCNN.forward (cnn_tools.py:164-176): x planar (B,n_in,N,N) -> y planar (B,2,N,N).  div=True: the convolutions write the
// four fluxes into the workspace's F, and y = 10000 div F (fluxdiv.hip) — every caller (qgx_cnn_forward, generator_forward[_mean],
// the calibration's comparisons, the step kernel's deferred finish) sees the one output shape and needs no second path
int cnn_forward(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N, hipStream_t st) {
    if (!net.flux()) return cnn_convs(g, net, x, y, B, N, st);
    QGX_REQUIRE(fluxdiv_size_ok(N), "flux-form net: no divergence kernel for N = %d (16, 32, 48, 64, 96 or 128)", N);
    float *F = g->work().F;
    QGX_REQUIRE(F && g->work().cap_elems >= (size_t)B * N * N, "flux-form net: the flux buffer is not reserved");
    if (const int rc = cnn_convs(g, net, x, F, B, N, st)) return rc;
    return fluxdiv_forward(F, y, B, N, st);
}

// Whether cnn_forward takes B members at N x N under the options in force: the conditions its launchers assert, gathered so
// that every entry point (qgx_generator_forward, qgx_cnn_forward, qgx_step) refuses a grid BEFORE its first launch and before
// the stepper touches the sampler state; the launchers' own QGX_REQUIREs stay as backstops.  k_conv3 is an optimisation that
// hands a layer back when its tile does not fit, so the exact-f32 conditions are those of k_conv (or of the split-K form of
// small ensembles) and of the last layer.  With the shipped options: N = 16, 32, 48, 64, 96, 128 — 8, 12 and 24 have no
// whole number of row tiles, and from 192 on the 5x5 layer's 32-channel patch (R + 4 rows of N pixels) exceeds the LDS.
bool cnn_size_ok(const qgx_generator *g, const NetHost &net, int B, int N) {
    const int R = choose_rows(N);
    if (B < 1 || R <= 0 || N % R) return false;
    if (net.flux() && !fluxdiv_size_ok(N)) return false;
    if (net.generic) return cnng_size_ok(net, B, N);
    if (half_path_ok(g, B, N)) return N % 4 == 0;      // (launch_convh_first's float4 rows)
    constexpr size_t LIM = 160 * 1024;
    auto patch = [&](int rows, int ks, int stride) { return (size_t)(rows + ks - 1) * N * stride * sizeof(float); };
    if (patch(R, 5, net.n_in) > LIM) return false;                                        // layer 1: planar input
    const bool small = g->opt_small && small_ensemble(B, N);
    for (int l = 1; l < 7; ++l) {
        const int cin = l == 1 ? 128 : (l == 2 ? 64 : 32), ks = l == 1 ? 5 : 3;
        const size_t lds = small ? patch(rows_small(N), ks, (cin >= 64 ? 16 : 32) + 4)
                                 : patch(R, ks, (g->opt_cc == 32 ? 32 : 16) + 4);
        if (lds > LIM) return false;
    }
    if (g->opt_last_valu) {
        const int Rl = last_rows(g, B, N);
        return Rl > 0 && N % Rl == 0 && last_lds_bytes(Rl, N) <= LIM;
    }
    return patch(R, 3, 16 + 4) <= LIM;
}

// ---- f16x3 range calibration (run once by qgx_generator_create) ------------------------------------------------
// The f16x3 arithmetic stores every activation x as hi = f16(s x), lo = f16(s x - hi) with ONE power-of-two scale s
// for the whole net.  It is float32-class only while the stored values stay inside a window: above 65504 the hi part
// overflows; below 2^-2 (relative to a layer's largest value) the lo part is subnormal and the pair no longer carries
// 22 bits against that layer's scale.  Nothing about a user-trained net guarantees that, so the nets are evaluated
// here once in EXACT f32 on calibration inputs (unit-variance white noise, smooth large-scale fields of amplitude 2-3,
// constants: what ChannelwiseScaler-normalised PV and N(0,1) latent noise look like) and the largest stored
// activation of every layer decides:
//   * s = the power of two that puts the largest layer maximum at <= 2^10 (64x headroom below the f16 overflow for
//     inputs hotter than the calibration set; the run-time guard range_guard() catches what still escapes),
//     s = 1 whenever that already holds (the shipped nets);
//   * "fold" (layer 1 stores its pre-BatchNorm ReLU output) only if that tensor fits the same window;
//   * if the layer maxima span more than the window (2^12), f16x3 cannot be float32-class for this net:
//     precision 0 (the exact-f32 MFMA kernels) becomes the default.
// The 1-D Winograd form of the 5x5 layer (conv_wino.hpp) multiplies 0.4 x as much, but its float32 transforms and
// accumulators carry the condition of the Toom-Cook matrices: for the layer, 3-4 x the rounding error of the 25-tap form
// (float32 evaluation of both: tests/test_conv_transform_numerics_cpu.py), and how much of that reaches the net's output
// depends on the weights behind it (shipped nets: 3e-6 ... 9e-6 of max|y|; random-weight nets up to 5e-5).  So it is
// MEASURED per generator AND per grid size it is specialised for (32, 48, 64, 96, 128: the tile shapes, and with them the
// rows and quads a workgroup transforms together, differ between them): every net is evaluated on calibration inputs
// (white noise, one member hotter; smooth fields; constants) with the Winograd layer and with the exact-f32 kernels, and
// the Winograd form becomes the default AT THAT SIZE only if the largest difference stays below WINO_MAX_ERR of the
// largest output — half of the tolerance the golden vectors are held to.  (qgx_generator_wino_info_n reports the decision
// per size; option "wino" = 0 / 1 overrides it, 2 restores it.)  The two tile shapes a size may run in (full / half
// height) give bit-identical results, as do k_convw and k_convw2: one evaluation per size covers them.
static constexpr float WINO_MAX_ERR = 1e-5f;
// An OLS net's input is PV alone, a field without power at the smallest scales: its noise members are band-limited (wavenumbers
// |k_x|, |k_y| <= N/3, unit variance, then the member's amplitude factor) like the q it is fed.  On such inputs the Winograd
// form's error for the AndrewCNN(2, 2) shipped as GZ's net_mean is 3e-5 of max|y| where white noise shows 5-7e-6.
static void band_limited_field(std::vector<float> &f, int N, const std::function<float()> &white) {
    const int kc = N / 3;
    std::vector<double> re((size_t)N * N), im((size_t)N * N, 0.0), tr((size_t)N * N), ti((size_t)N * N), cs(N), sn(N);
    for (auto &v : re) v = white();
    for (int t = 0; t < N; ++t) { cs[t] = cos(6.283185307179586 * t / N); sn[t] = sin(6.283185307179586 * t / N); }
    auto pass = [&](bool rows, double sign) {       // DFT along x (rows) or y
        for (int a = 0; a < N; ++a)
            for (int k = 0; k < N; ++k) {
                double sr = 0.0, si = 0.0;
                for (int j = 0; j < N; ++j) {
                    const size_t o = rows ? (size_t)a * N + j : (size_t)j * N + a;
                    const int t = (int)(((long)k * j) % N);
                    const double c = cs[t], sv = sign * sn[t];
                    sr += re[o] * c - im[o] * sv;
                    si += re[o] * sv + im[o] * c;
                }
                const size_t o = rows ? (size_t)a * N + k : (size_t)k * N + a;
                tr[o] = sr; ti[o] = si;
            }
        re.swap(tr); im.swap(ti);
    };
    pass(true, -1.0); pass(false, -1.0);            // forward transform
    for (int y = 0; y < N; ++y)                       // low-pass
        for (int x = 0; x < N; ++x) {
            const int ky = y <= N / 2 ? y : y - N, kx = x <= N / 2 ? x : x - N;
            if (ky > kc || ky < -kc || kx > kc || kx < -kc) { re[(size_t)y * N + x] = 0.0; im[(size_t)y * N + x] = 0.0; }
        }
    pass(true, 1.0); pass(false, 1.0);              // inverse (unnormalised: the field is scaled to unit variance below)
    double m = 0.0, m2 = 0.0;
    for (double v : re) { m += v; m2 += v * v; }
    m /= (double)N * N;
    const double sd = sqrt(fmax(m2 / ((double)N * N) - m * m, 1e-300));
    f.resize((size_t)N * N);
    for (size_t i = 0; i < f.size(); ++i) f[i] = (float)((re[i] - m) / sd);
}

static int calibrate_wino(qgx_generator *g) {
    for (int i = 0; i < 5; ++i) { g->auto_wino_n[i] = 0; g->wino_err_n[i] = 0.f; }
    g->opt_wino = 0;
    if (g->opt_precision != 3) return QGX_OK;
    static const int SIZES[5] = {32, 48, 64, 96, 128};
    unsigned *cd = nullptr;
    QGX_HIP(hipMalloc((void **)&cd, 2 * sizeof(unsigned)));
    const int saved_part = g->opt_part_max_tiles, saved_min = g->opt_wino_min_tiles;
    int rc = QGX_OK;
    for (int si = 0; si < 5 && !rc; ++si) {
        const int N = SIZES[si], npix = N * N;
        // as many members as keep the workspace of the calibration at what eight 64 x 64 members need (2 at 128 x 128)
        const int B = N <= 64 ? 8 : (N == 96 ? 4 : 2);
        // member patterns: 0-2 white noise, 3 white x 2, 4 white x 1.5, 5-6 smooth large-scale fields + noise, 7 constants;
        // with fewer than eight members the hot, the smooth and the constant ones come first
        static const int PAT8[8] = {0, 1, 2, 3, 4, 5, 6, 7}, PAT4[4] = {3, 5, 7, 0}, PAT2[2] = {3, 5};
        const int *pat = B == 8 ? PAT8 : (B == 4 ? PAT4 : PAT2);
        rc = generator_reserve(g, B, N);
        if (rc) break;
        const Workspace &w = g->work();
        float worst = 0.f;
        for (int n = 0; n < g->n_nets && !rc; ++n) {
            const NetHost &net = g->nets[n];
            if (!net.L[1].ww[0]) { worst = INFINITY; break; }
            std::vector<float> x((size_t)B * net.n_in * npix);
            uint32_t lcg = 54321u + 977u * n;
            auto uni = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) + 0.5f) * (1.0f / 16777216.0f); };
            std::vector<float> band;
            for (int b = 0; b < B; ++b)
                for (int c = 0; c < net.n_in; ++c) {
                    const bool banded = g->kind == QGX_GEN_OLS && pat[b] < 5;
                    if (banded) band_limited_field(band, N, [&]() { return sqrtf(-2.f * logf(uni())) * cosf(6.2831853f * uni()); });
                    for (int y = 0; y < N; ++y)
                        for (int xx = 0; xx < N; ++xx) {
                            float v;
                            const int pb = pat[b];
                            const float white = banded ? band[(size_t)y * N + xx] : sqrtf(-2.f * logf(uni())) * cosf(6.2831853f * uni());
                            if (pb < 5) v = white * (pb == 3 ? 2.f : (pb == 4 ? 1.5f : 1.f));
                            else if (pb < 7) v = 2.f * sinf(6.2831853f * (y * (c + 1) + xx * (pb - 4)) / N)
                                                 + cosf(6.2831853f * 2 * xx / N) + 0.3f * white;
                            else v = 3.f * ((c & 1) ? -1.f : 1.f);
                            x[(((size_t)b * net.n_in + c) * N + y) * N + xx] = v;
                        }
                }
            QGX_HIP(hipMemcpy(w.X, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice));
            g->opt_precision = 0;
            rc = cnn_forward(g, net, w.X, w.Y0, B, N, nullptr);
            g->opt_precision = 3; g->opt_wino = 1; g->opt_wino_min_tiles = 1; g->opt_part_max_tiles = 0;
            if (!rc) rc = cnn_forward(g, net, w.X, w.Y1, B, N, nullptr);
            g->opt_wino = 0; g->opt_wino_min_tiles = saved_min; g->opt_part_max_tiles = saved_part;
            if (rc) break;
            QGX_HIP(hipMemset(cd, 0, 2 * sizeof(unsigned)));
            hipLaunchKernelGGL(k_absdiff_max, dim3(64), dim3(256), 0, nullptr, (const float *)w.Y1, (const float *)w.Y0,
                               (size_t)B * net.y_channels() * npix, cd);
            float h[2];
            QGX_HIP(hipMemcpy(h, cd, sizeof(h), hipMemcpyDeviceToHost));
            const float err = h[1] > 0.f ? h[0] / h[1] : INFINITY;
            worst = fmaxf(worst, std::isfinite(err) ? err : INFINITY);
        }
        g->wino_err_n[si] = worst;
        g->auto_wino_n[si] = !rc && worst <= WINO_MAX_ERR ? 1 : 0;
    }
    (void)hipFree(cd);
    QGX_HIP(hipMemset(g->range_dev, 0, 2 * sizeof(unsigned)));     // the calibration runs are not the caller's
    if (rc) return rc;
    g->opt_wino = 2;
    return QGX_OK;
}

static int calibrate(qgx_generator *g) {
    const int N = 32, B = 8, npix = N * N;
    int rc = generator_reserve(g, B, N);
    if (rc) return rc;
    const Workspace &w = g->work();
    unsigned *cd = nullptr;
    QGX_HIP(hipMalloc((void **)&cd, 20 * sizeof(unsigned)));
    QGX_HIP(hipMemset(cd, 0, 20 * sizeof(unsigned)));
    const int saved_precision = g->opt_precision;
    g->opt_precision = 0;
    for (int n = 0; n < g->n_nets && !rc; ++n) {
        const NetHost &net = g->nets[n];
        std::vector<float> x((size_t)B * net.n_in * npix);
        uint32_t lcg = 12345u + 977u * n;
        auto uni = [&]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) + 0.5f) * (1.0f / 16777216.0f); };
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < net.n_in; ++c)
                for (int y = 0; y < N; ++y)
                    for (int xx = 0; xx < N; ++xx) {
                        float v;
                        const float white = sqrtf(-2.f * logf(uni())) * cosf(6.2831853f * uni());
                        if (b < 4) v = white * (b == 3 ? 2.f : 1.f);                      // white noise, one member hotter
                        else if (b < 6) v = 2.f * sinf(6.2831853f * (y * (c + 1) + xx * (b - 3)) / N)
                                            + cosf(6.2831853f * 2 * xx / N) + 0.3f * white;   // smooth, amplitude ~3
                        else v = (b == 6 ? 3.f : -3.f) * ((c & 1) ? -1.f : 1.f);         // constants
                        x[(((size_t)b * net.n_in + c) * N + y) * N + xx] = v;
                    }
        QGX_HIP(hipMemcpy(w.X, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice));
        g->calib_dev = cd;
        rc = cnn_forward(g, net, w.X, w.Y0, B, N, nullptr);
        g->calib_dev = nullptr;
        if (rc) break;
        // layer 1 with an identity BatchNorm = what the folded f16x3 variant stores
        LayerHost L0 = net.L[0];
        L0.scale = L0.ones; L0.shift = L0.zeros;
        rc = launch_conv_first(g, L0, net.n_in, 2, 0, w.X, w.actA, B, N, nullptr);
        if (rc) break;
        launch_absmax(w.actA, (size_t)B * npix * 128, cd + 16, nullptr);
    }
    g->opt_precision = saved_precision;
    unsigned h[20];
    if (!rc) {
        if (hipMemcpy(h, cd, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) rc = QGX_ERR_HIP;
    }
    (void)hipFree(cd);
    if (rc) return rc;
    for (int l = 0; l < 10; ++l) memcpy(&g->calib_max[l], &h[2 * l + 1], sizeof(float));
    auto window = [&](bool with_fold, float &lo, float &hi) {
        lo = INFINITY; hi = 0.f;
        for (int l = with_fold ? 1 : 0; l < 7; ++l)
            if (g->calib_max[l] > 0.f) { lo = fminf(lo, g->calib_max[l]); hi = fmaxf(hi, g->calib_max[l]); }
        if (with_fold && g->calib_max[8] > 0.f) { lo = fminf(lo, g->calib_max[8]); hi = fmaxf(hi, g->calib_max[8]); }
    };
    const float TOP = 1024.f, BOT = 0.25f;                 // window of s * (layer maximum)
    float lo, hi;
    int fold = 1;
    window(true, lo, hi);
    if (!(hi > 0.f) || !std::isfinite(hi) || hi / lo > TOP / BOT) { fold = 0; window(false, lo, hi); }
    int precision = 3, e = 0;
    if (!(hi > 0.f) || !std::isfinite(hi) || hi / lo > TOP / BOT) precision = 0;
    else if (hi > TOP || lo < BOT) {
        int eh = 0;
        (void)frexpf(hi, &eh);                             // hi = m 2^eh, m in [0.5, 1): hi * 2^(10 - eh) in [512, 1024)
        e = 10 - eh;
    }
    g->auto_precision = precision; g->auto_fold = fold; g->auto_ascale_log2 = e;
    g->opt_precision = precision; g->opt_fold = fold; g->opt_ascale = ldexpf(1.f, e);
    return QGX_OK;
}

int cnn_calibrate(qgx_generator *g) {
    if (const int rc = calibrate(g)) return rc;
    return calibrate_wino(g);
}
void cnn_exact_f32_only(qgx_generator *g) {
    g->opt_precision = g->auto_precision = 0; g->opt_fold = g->auto_fold = 0; g->opt_wino = 0;
}

}  // namespace qgx

using namespace qgx;

#define UNET_REFUSE "%s: a U-Net generator handle runs the exact-f32 kernels of unet.hip only; this applies to the AndrewCNN kernels"
#define ANN_REFUSE "%s: an ANN generator handle runs the stencil-network kernels of ann.hip only; this applies to the AndrewCNN kernels"
#define REFUSE_NON_ANDREW(g, what)                                  \
    do {                                                            \
        QGX_REQUIRE(!(g)->unet, UNET_REFUSE, what);                 \
        QGX_REQUIRE(!(g)->ann, ANN_REFUSE, what);                   \
    } while (0)
extern "C" int qgx_generator_wino_info_n(const qgx_generator *g, int N, int *enabled, int *chosen_by_calibration, float *calibration_error) {
    QGX_REQUIRE(g, "qgx_generator_wino_info_n: null generator");
    REFUSE_NON_ANDREW(g, "qgx_generator_wino_info_n");
    const int si = wino_size_index(N);
    if (enabled) *enabled = si >= 0 && (g->opt_wino == 1 || (g->opt_wino == 2 && g->auto_wino_n[si]));
    if (chosen_by_calibration) *chosen_by_calibration = si >= 0 ? g->auto_wino_n[si] : 0;
    if (calibration_error) *calibration_error = si >= 0 ? g->wino_err_n[si] : INFINITY;
    return QGX_OK;
}

// which kernel the 5x5 layer (layer 2) of net `inet` takes for an ensemble of B members at N x N with the options in
// force (Layer2Plan::kernel): 0 exact-f32 MFMA, 1 the 25-tap f16x3 kernel, 2 its split-K form (tiny ensembles), 3 1-D
// Winograd (k_convw), 4 1-D Winograd with the transform under the MFMAs (k_convw2)
extern "C" int qgx_generator_layer2_kernel(const qgx_generator *g, int inet, int B, int N, int *kernel) {
    QGX_REQUIRE(g && kernel, "qgx_generator_layer2_kernel: null argument");
    REFUSE_NON_ANDREW(g, "qgx_generator_layer2_kernel");
    QGX_REQUIRE(inet >= 0 && inet < g->n_nets, "qgx_generator_layer2_kernel: net %d of %d", inet, g->n_nets);
    QGX_REQUIRE(!g->nets[inet].generic, "qgx_generator_layer2_kernel: net %d runs the generic engine (conv_generic.hip), which has one exact-f32 "
                "kernel for every layer; the question applies to the shipped architecture's 128 -> 64 5x5 layer", inet);
    *kernel = plan_layer2(g, g->nets[inet], B, N).kernel;
    return QGX_OK;
}

extern "C" int qgx_generator_wino_info(const qgx_generator *g, int *enabled, int *chosen_by_calibration, float *calibration_error) {
    QGX_REQUIRE(g, "qgx_generator_wino_info: null generator");
    REFUSE_NON_ANDREW(g, "qgx_generator_wino_info");
    // the 64 x 64 grid (the headline workload); qgx_generator_wino_info_n reports every size
    if (enabled) *enabled = g->opt_wino == 1 || (g->opt_wino == 2 && g->auto_wino_n[2]);
    if (chosen_by_calibration) *chosen_by_calibration = g->auto_wino_n[2];
    if (calibration_error) *calibration_error = g->wino_err_n[2];
    return QGX_OK;
}

extern "C" int qgx_generator_info(const qgx_generator *g, int *precision, int *ascale_log2, int *fold, float *layer_absmax) {
    QGX_REQUIRE(g, "qgx_generator_info: null generator");
    if (precision) *precision = g->opt_precision;
    if (ascale_log2) { int e = 0; (void)frexpf(g->opt_ascale, &e); *ascale_log2 = e - 1; }
    if (fold) *fold = g->opt_fold;
    if (layer_absmax) memcpy(layer_absmax, g->calib_max, sizeof(g->calib_max));
    return QGX_OK;
}

extern "C" int qgx_generator_profile(qgx_generator *g, int layer) {
    QGX_REQUIRE(g && layer >= -1 && layer < 8, "qgx_generator_profile: bad argument");
    REFUSE_NON_ANDREW(g, "qgx_generator_profile (per-layer profile)");
    g->prof_layer = layer;
    g->prof_used = 0;
    g->prof_seen = 0;
    return QGX_OK;
}

extern "C" int qgx_generator_profile_read(qgx_generator *g, double *total_ms, int64_t *launches) {
    QGX_REQUIRE(g && total_ms && launches, "qgx_generator_profile_read: null argument");
    REFUSE_NON_ANDREW(g, "qgx_generator_profile_read (per-layer profile)");
    double tot = 0.0;
    for (size_t i = 0; i + 1 < g->prof_used; i += 2) {
        QGX_HIP(hipEventSynchronize(g->prof_ev[i + 1]));
        float ms = 0.f;
        QGX_HIP(hipEventElapsedTime(&ms, g->prof_ev[i], g->prof_ev[i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)(g->prof_used / 2);
    g->prof_used = 0;
    return QGX_OK;
}

extern "C" int qgx_generator_set_option(qgx_generator *g, const char *name, int value) {
    QGX_REQUIRE(g && name, "qgx_generator_set_option: null argument");
    if (g->generic) {          // the generic engine has one exact-f32 kernel family and no variants to select
        QGX_REQUIRE(!strcmp(name, "precision") && value == 0,
                    "qgx_generator_set_option('%s'=%d): a handle of qgx_generator_create_arch with a net of another architecture than the shipped one "
                    "runs exact f32 (precision 0) only: the generic engine has no f16x3 or Winograd path and no kernel variants", name, value);
        return QGX_OK;
    }
    if (g->unet || g->ann) {   // every option selects between AndrewCNN kernels (net_mean runs the exact-f32 ones): only precision 0 holds
        QGX_REQUIRE(!strcmp(name, "precision") && value == 0,
                    "qgx_generator_set_option('%s'=%d): a%s generator handle runs exact f32 (precision 0) only; the option applies to the AndrewCNN kernels",
                    name, value, g->ann ? "n ANN" : " U-Net");
        return QGX_OK;
    }
    if (!strcmp(name, "chunk")) { QGX_REQUIRE(value == 16 || value == 32, "chunk must be 16 or 32"); g->opt_cc = value; }
    else if (!strcmp(name, "last_valu")) g->opt_last_valu = value ? 1 : 0;
    else if (!strcmp(name, "small")) g->opt_small = value ? 1 : 0;
    else if (!strcmp(name, "v3")) g->opt_v3 = value;   // -1 auto, 0 off, 1 = slice per tap row, 2 = per chunk
    else if (!strcmp(name, "precision")) { QGX_REQUIRE(value == 0 || value == 3, "precision must be 0 (f32) or 3 (f16x3)"); g->opt_precision = value; }
    else if (!strcmp(name, "member_chunk")) { QGX_REQUIRE(value >= 0, "member_chunk must be >= 0"); g->opt_member_chunk = value; }
    else if (!strcmp(name, "pair")) g->opt_pair = value ? 1 : 0;
    else if (!strcmp(name, "fuse")) g->opt_fuse = value & 7;
    else if (!strcmp(name, "fuse96")) g->opt_fuse96 = value & 3;
    else if (!strcmp(name, "small_tiles")) g->opt_small_tiles = value ? 1 : 0;
    else if (!strcmp(name, "tiny_pairs")) { QGX_REQUIRE(value >= 0 && value <= 7, "tiny_pairs: bits 0 (layers 7, 8), 1 (layers 5, 6), 2 (layers 3, 4)"); g->opt_tiny_pairs = value; }
    else if (!strcmp(name, "last_rows")) g->opt_last_rows = value;
    else if (!strcmp(name, "part_max_tiles")) g->opt_part_max_tiles = value;
    else if (!strcmp(name, "fold")) g->opt_fold = value ? 1 : 0;
    else if (!strcmp(name, "wino")) { QGX_REQUIRE(value >= 0 && value <= 2, "wino must be 0 (never), 1 (every specialised grid) or 2 (per grid size, as calibrated)"); g->opt_wino = value; }
    else if (!strcmp(name, "wino2")) g->opt_wino2 = value ? 1 : 0;
    else if (!strcmp(name, "h2_rows96")) { QGX_REQUIRE(value == 0 || value == 12 || value == 16, "h2_rows96 must be 0 (auto), 12 or 16"); g->opt_h2_rows96 = value; }
    else if (!strcmp(name, "wino_rows64")) { QGX_REQUIRE(value == 0 || value == 4 || value == 8, "wino_rows64 must be 0 (auto), 4 or 8"); g->opt_wino_rows64 = value; }
    else if (!strcmp(name, "wino_rows96")) { QGX_REQUIRE(value == 0 || value == 12 || value == 16, "wino_rows96 must be 0 (auto), 12 or 16"); g->opt_wino_rows96 = value; }
    else if (!strcmp(name, "wino_min_tiles")) { QGX_REQUIRE(value >= 1, "wino_min_tiles must be >= 1"); g->opt_wino_min_tiles = value; }
    else if (!strcmp(name, "h2_grid")) g->opt_h2_grid = value;
    else if (!strcmp(name, "prio_alt")) g->opt_prio_alt = value;
    else if (!strcmp(name, "h2_w8")) g->opt_h2_w8 = value & 3;
    else if (!strcmp(name, "h2_tw32")) g->opt_h2_tw32 = value ? 1 : 0;
    else if (!strcmp(name, "h2_x96")) g->opt_h2_x96 = value ? 1 : 0;
    else if (!strcmp(name, "h2_w8_min96")) g->opt_h2_w8_min96 = value;
    else if (!strcmp(name, "half_min_tiles")) { QGX_REQUIRE(value >= 1, "half_min_tiles must be >= 1"); g->opt_half_min_tiles = value; }
    else if (!strcmp(name, "first_h")) g->opt_first_h = value ? 1 : 0;
    else if (!strcmp(name, "ascale_log2")) { QGX_REQUIRE(value >= -24 && value <= 24, "ascale_log2 must be in -24..24"); g->opt_ascale = ldexpf(1.f, value); }
    else if (!strcmp(name, "prof_every")) { QGX_REQUIRE(value >= 1, "prof_every must be >= 1"); g->prof_every = value; }
    else if (!strcmp(name, "auto")) { g->opt_precision = g->auto_precision; g->opt_fold = g->auto_fold; g->opt_ascale = ldexpf(1.f, g->auto_ascale_log2); g->opt_wino = 2; }
    else if (!strcmp(name, "first_split")) { QGX_REQUIRE(value == 1 || value == 2 || value == 4, "first_split must be 1, 2 or 4"); g->opt_first_split = value; }
    else QGX_REQUIRE(false, "unknown generator option '%s'", name);
    return QGX_OK;
}

#ifdef QGX_AB
// A/B library, debugging: copy the first nbytes of activation buffer `which` (0: the odd layers' outputs, 1: the even layers',
// 2: the fluxes (B, 4, N, N) of a flux-form net's last forward)
extern "C" int qgx_debug_read_act(qgx_generator *g, int which, void *dst_dev, size_t nbytes, void *stream) {
    QGX_REQUIRE(g && dst_dev && which >= 0 && which <= 2, "qgx_debug_read_act: bad argument");
    const Workspace &w = g->work();
    QGX_REQUIRE(which != 2 || (w.F && nbytes <= w.cap_elems * 4 * sizeof(float)), "qgx_debug_read_act: no flux buffer of %zu bytes", nbytes);
    QGX_HIP(hipMemcpyAsync(dst_dev, which == 2 ? (const void *)w.F : which ? (const void *)w.actB : (const void *)w.actA, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return QGX_OK;
}
#endif
#ifdef QGX_STAMPS
// diagnostic builds only (bench_tools/conv_stamps.py): where the clock-stamp trace of layer `layer` goes
extern "C" int qgx_debug_set_stamps(qgx_generator *g, void *buf, int layer) {
    g->stamps = (unsigned long long *)buf;
    g->stamp_layer = layer;
    return QGX_OK;
}
#endif
