// A differentiable circular convolution (include/qgx_conv_train.h): the layer operation the training of AndrewCNN nets is made
// of.  Forward and data gradient run conv_generic.hip's k_convg (its bias-only NHWC epilogue); the weight gradient is this
// file's kernel.  All three are exact-f32 matrix-core kernels (v_mfma_f32_32x32x2_f32), stateless, on the caller's stream.
//
//   forward          the weights change every step, so cnn_pack_net_arch's host packer has a device twin, k_pack, that writes
//                    [group][coutp][8] (K padded to 8, N to 32, one zero group at the end) and the padded bias into the workspace
//   backward_data    dx = conv(dy, w'), w'[ci, co, ky, kx] = w[co, ci, k - 1 - ky, k - 1 - kx]: k_pack's flip-and-transpose mode,
//                    then the forward launch with the roles of cin and cout swapped
//   backward_weight  dw[co, ci, tap] = sum over pixels of dy[p, co] x[p + tap, ci]: a GEMM with M = cout, N = cin k^2,
//                    K = B N^2.  One workgroup owns a (32 output channels, 32 input channels) tile pair and a share of K: units
//                    of R image rows, walked in order.  Per unit the dy rows and the x rows with their halo are staged in LDS as
//                    NHWC patches of pixel stride 36 (k_convg's G_STRIDE: a lane half reads 32 consecutive channels, the other
//                    half the next pixel, 4 banks on); an MFMA takes A = dy at two pixels, B = x at the two shifted pixels, one
//                    ds_read_b32 each.  The k^2 taps are dealt to the four waves (tap = wave + 4 j: 3 | 2 | 2 | 2 accumulator
//                    tiles of 16 registers at 3 x 3, 7 | 6 | 6 | 6 at 5 x 5).  Each workgroup stores its accumulators into its own
//                    slice of the workspace; k_wgrad_reduce adds the slices in a fixed order.  No atomics: the bits do not depend on the
//                    stream or on the order the workgroups ran in.
//   db               per-block partial sums over fixed pixel ranges (k_dbias), added in order (k_dbias_reduce)
#include "generator.hpp"

namespace qgx {

#include "conv_types.hpp"

constexpr int T_STRIDE = 32 + 4;      // floats per patch pixel (conv_generic.hip::G_STRIDE)
static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- weights as k_convg reads them ---------------------------------------------------------
// out[g][n][e], g over (chunk of <= 32 K channels, tap, 8 channels), n < cnp, + one zero group; K channel c, output n:
//   flip = 0: w[n][c][tap]              (w is (cn, ck, T): the forward convolution)
//   flip = 1: w[c][n][T - 1 - tap]      (w is (ck, cn, T): the data gradient's flipped, transposed weights)
// and bp[n] = bias[n] (zero from cn on, or everywhere without a bias)
__global__ __launch_bounds__(256) void k_pack(const float *w, const float *bias, float *wp, float *bp, int ck, int cn, int ckp,
                                              int cnp, int T, int flip, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < cnp) bp[idx] = (bias && idx < cn) ? bias[idx] : 0.f;
    if (idx >= total) return;
    const int e = idx & 7, n = (idx >> 3) % cnp, g = idx / (cnp * 8);
    const int ngroups = T * (ckp >> 3);
    float v = 0.f;
    if (g < ngroups && n < cn) {
        const int q = g / (T * 4), rem = g - q * T * 4;
        const int left = (ckp >> 3) - q * 4, cc8 = left < 4 ? left : 4;
        const int tap = rem / cc8, g8 = rem - tap * cc8;
        const int c = q * 32 + g8 * 8 + e;
        if (c < ck) v = flip ? w[((size_t)c * cn + n) * T + (T - 1 - tap)] : w[((size_t)n * ck + c) * T + tap];
    }
    wp[idx] = v;
}

// ---- weight gradient -----------------------------------------------------------------------
struct WgradArgs {
    const float *x, *dy;     // NHWC (B, N, N, cin8), (B, N, N, cout8)
    float *part;             // [share][pair][tap][32 co][32 ci]
    int N, R, ks, cin8, cout8, cit_n, U, ups, tiles_per_img;
};

template <int TW>
__global__ __launch_bounds__(256) void k_wgrad(WgradArgs a) {
    const int N = a.N, R = a.R, KS = a.ks, P = KS / 2, T = KS * KS, PR = R + KS - 1;
    float *xpatch = reinterpret_cast<float *>(conv_smem);
    float *dpatch = xpatch + PR * N * T_STRIDE;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int li = lane & 31, h = lane >> 5;
    const int pair = blockIdx.x, share = blockIdx.y;
    const int cot = pair / a.cit_n, cit = pair - cot * a.cit_n;
    const int co0 = cot * 32, ci0 = cit * 32;
    const int ccx = a.cin8 - ci0 < 32 ? a.cin8 - ci0 : 32;      // real (8-padded) channels of the two tiles: multiples of 8
    const int ccd = a.cout8 - co0 < 32 ? a.cout8 - co0 : 32;

    f32x16 acc[TW];
    int tky[TW], tkx[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        const int tap = wave + 4 * j;
        tky[j] = tap / KS;
        tkx[j] = tap - tky[j] * KS - P;
    }

    const int u0 = share * a.ups, u1 = u0 + a.ups < a.U ? u0 + a.ups : a.U;
    for (int u = u0; u < u1; ++u) {
        const int b = u / a.tiles_per_img, y0 = (u - b * a.tiles_per_img) * R;
        __syncthreads();
        for (int it = threadIdx.x; it < PR * N * 8; it += 256) {
            const int c4 = it & 7, pl = it >> 3;
            const int pr = pl / N, xx = pl - pr * N;
            int gy = y0 - P + pr;
            gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c4 * 4 < ccx) v = *reinterpret_cast<const float4 *>(&a.x[(((size_t)b * N + gy) * N + xx) * a.cin8 + ci0 + c4 * 4]);
            *reinterpret_cast<float4 *>(&xpatch[pl * T_STRIDE + c4 * 4]) = v;
        }
        for (int it = threadIdx.x; it < R * N * 8; it += 256) {
            const int c4 = it & 7, pl = it >> 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c4 * 4 < ccd) v = *reinterpret_cast<const float4 *>(&a.dy[(((size_t)b * N + y0) * N + pl) * a.cout8 + co0 + c4 * 4]);
            *reinterpret_cast<float4 *>(&dpatch[pl * T_STRIDE + c4 * 4]) = v;
        }
        __syncthreads();
        for (int r = 0; r < R; ++r) {
#pragma unroll 2
            for (int xp = 0; xp < N; xp += 2) {
                const int px = xp + h;
                const float A = dpatch[(r * N + px) * T_STRIDE + li];
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    if (wave + 4 * j >= T) continue;            // wave-uniform
                    int col = px + tkx[j];
                    col = col < 0 ? col + N : (col >= N ? col - N : col);
                    const float Bv = xpatch[((r + tky[j]) * N + col) * T_STRIDE + li];
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A, Bv, acc[j], 0, 0, 0);
                }
            }
        }
    }
    // acc[j][r]: output channel co0 + (r & 3) + 8 (r >> 2) + 4 h, input channel ci0 + li, tap wave + 4 j
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int tap = wave + 4 * j;
        if (tap >= T) continue;
        float *o = a.part + (((size_t)share * gridDim.x + pair) * T + tap) * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + li] = acc[j][r];
    }
}

// dw[co][ci][tap] = the shares' slices added in a fixed order: a workgroup of RED_WAVES waves owns 64 consecutive elements of a
// slice (a slice is a multiple of 1024 elements); wave g adds the shares g, g + RED_WAVES, ... in order (coalesced 256-byte
// reads), then the waves' sums are added in order
constexpr int RED_WAVES = 8;
__global__ __launch_bounds__(64 * RED_WAVES) void k_wgrad_reduce(const float *part, float *dw, int S, int cit_n, int T, int cin,
                                                                int cout, int slice) {
    __shared__ float red[RED_WAVES][64];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + e;
    float s = 0.f;
#pragma unroll 4
    for (int sh = g; sh < S; sh += RED_WAVES) s += part[(size_t)sh * slice + idx];
    red[g][e] = s;
    __syncthreads();
    if (g) return;
    const int col = idx & 31, row = (idx >> 5) & 31, q = idx >> 10;
    const int pair = q / T, tap = q - pair * T;
    const int cot = pair / cit_n, cit = pair - cot * cit_n;
    const int co = cot * 32 + row, ci = cit * 32 + col;
    if (co >= cout || ci >= cin) return;
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < RED_WAVES; ++k) v += red[k][e];
    dw[((size_t)co * cin + ci) * T + tap] = v;
}

// db: block blk sums the pixels [blk ppb, (blk + 1) ppb) of every channel: thread (g, c) the pixels p0 + g, p0 + g + G, ...
// in order, then the G groups in order
__global__ __launch_bounds__(256) void k_dbias(const float *dy, float *bpart, int64_t npix, int64_t ppb, int cout8) {
    __shared__ float red[256];
    const int G = 256 / cout8, t = threadIdx.x;
    const int g = t / cout8, c = t - g * cout8;
    const int64_t p0 = (int64_t)blockIdx.x * ppb, p1 = p0 + ppb < npix ? p0 + ppb : npix;
    float s = 0.f;
    if (g < G)
        for (int64_t p = p0 + g; p < p1; p += G) s += dy[(size_t)p * cout8 + c];
    red[t] = s;
    __syncthreads();
    if (g == 0) {
        float v = 0.f;
        for (int k = 0; k < G; ++k) v += red[k * cout8 + c];
        bpart[(size_t)blockIdx.x * cout8 + c] = v;
    }
}
__global__ __launch_bounds__(256) void k_dbias_reduce(const float *bpart, float *db, int nb, int cout8, int cout) {
    const int c = threadIdx.x;
    if (c >= cout) return;
    float s = 0.f;
    for (int k = 0; k < nb; ++k) s += bpart[(size_t)k * cout8 + c];
    db[c] = s;
}

// ---- host side -------------------------------------------------------------------------------
// The weight gradient's partition, a function of (B, N, cin, cout, k) alone.  Units are R rows of an image: the most of 4, 2, 1
// whose two patches fit 80 KiB (two workgroups per CU), else the most that fit 160 KiB.  The U = B N / R units go to S shares of
// `ups` consecutive units (the last share may hold fewer), S chosen so that pairs x shares is about 512 workgroups.
struct WgradPlan {
    int R, U, ups, S, cot_n, cit_n, T, nb;
    int64_t ppb;
    size_t lds;
};
static size_t wgrad_lds(int R, int ks, int N) { return (size_t)(2 * R + ks - 1) * N * T_STRIDE * sizeof(float); }
static WgradPlan wgrad_plan(int64_t B, int N, int cin, int cout, int k) {
    WgradPlan p = {};
    for (const size_t cap : {(size_t)80 * 1024, (size_t)160 * 1024}) {
        for (int R = 4; R >= 1 && !p.R; R /= 2)
            if (wgrad_lds(R, k, N) <= cap) p.R = R;
        if (p.R) break;
    }
    p.lds = wgrad_lds(p.R, k, N);
    p.T = k * k;
    p.cot_n = round_up(cout, 32) / 32;
    p.cit_n = round_up(cin, 32) / 32;
    p.U = (int)(B * (N / p.R));
    const int pairs = p.cot_n * p.cit_n;
    int want = (512 + pairs - 1) / pairs;
    if (want > p.U) want = p.U;
    p.ups = (p.U + want - 1) / want;
    p.S = (p.U + p.ups - 1) / p.ups;
    // db: at most 256 blocks of at least 64 pixels
    const int64_t npix = B * N * N;
    int64_t nb = npix / 64 < 256 ? npix / 64 : 256;
    p.ppb = (npix + nb - 1) / nb;
    p.nb = (int)((npix + p.ppb - 1) / p.ppb);
    return p;
}

struct WorkLayout { size_t w, bias, part, bpart, floats; };
static size_t pack_floats(int ck, int cn, int T) { return (size_t)(T * (round_up(ck, 8) / 8) + 1) * round_up(cn, 32) * 8; }
static WorkLayout work_layout(int64_t B, int N, int cin, int cout, int k) {
    const WgradPlan p = wgrad_plan(B, N, cin, cout, k);
    auto al = [](size_t n) { return (n + 63) / 64 * 64; };
    WorkLayout L;
    const size_t a = pack_floats(cin, cout, k * k), b = pack_floats(cout, cin, k * k);
    L.w = 0;
    L.bias = al(a > b ? a : b);
    L.part = L.bias + 256;
    L.bpart = L.part + al((size_t)p.S * p.cot_n * p.cit_n * p.T * 1024);
    L.floats = L.bpart + al((size_t)p.nb * round_up(cout, 8));
    return L;
}

static int conv_shape_check(const char *what, int64_t B, int N, int cin, int cout, int k) {
    QGX_REQUIRE(N == 16 || N == 32 || N == 48 || N == 64 || N == 96 || N == 128, "%s: N = %d, expected 16, 32, 48, 64, 96 or 128", what, N);
    QGX_REQUIRE(B >= 1 && B <= ((int64_t)1 << 29) / (N * N), "%s: B = %lld, expected 1 ... 2^29 / N^2", what, (long long)B);
    QGX_REQUIRE(cin >= 1 && cin <= 256, "%s: cin = %d, expected 1 ... 256", what, cin);
    QGX_REQUIRE(cout >= 1 && cout <= 256, "%s: cout = %d, expected 1 ... 256", what, cout);
    QGX_REQUIRE(k == 3 || k == 5, "%s: k = %d, expected 3 or 5", what, k);
    return QGX_OK;
}
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define CONV_PTR(what, p)                                                                                  \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(aligned16(p), "%s: " #p " is not 16-byte aligned", what);                              \
    } while (0)
static int conv_work_check(const char *what, int64_t B, int N, int cin, int cout, int k, const void *work_dev, size_t work_bytes) {
    QGX_REQUIRE(work_dev, "%s: work_dev is NULL", what);
    QGX_REQUIRE(aligned16(work_dev), "%s: work_dev is not 16-byte aligned", what);
    const size_t need = work_layout(B, N, cin, cout, k).floats * sizeof(float);
    QGX_REQUIRE(work_bytes >= need, "%s: work_bytes = %zu, qgx_conv2d_workspace gives %zu", what, work_bytes, need);
    return QGX_OK;
}

// conv(in (B, N, N, ck8), weights of K channels ck -> cn outputs) + bias -> out (B, N, N, cn8)
static int conv_run(const char *what, const float *in, const float *w, const float *bias, float *out, int B, int N, int ck, int cn,
                    int k, int flip, float *ws, const WorkLayout &L, hipStream_t st) {
    const int ckp = round_up(ck, 8), cnp = round_up(cn, 32), T = k * k;
    QGX_REQUIRE(convg_linear_ok(B, N, cnp, k), "%s: N = %d is not supported by the generic engine (B = %d)", what, N, B);
    const int total = (int)pack_floats(ck, cn, T);
    hipLaunchKernelGGL(k_pack, dim3((total + 255) / 256), dim3(256), 0, st, w, bias, ws + L.w, ws + L.bias, ck, cn, ckp, cnp, T,
                       flip, total);
    QGX_HIP(hipGetLastError());
    return launch_convg_linear(in, out, ws + L.w, ws + L.bias, B, N, ckp, cnp, round_up(cn, 8), k, st);
}

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_conv2d_workspace(int64_t B, int N, int cin, int cout, int k, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_conv2d_workspace: bytes is NULL");
    if (const int rc = conv_shape_check("qgx_conv2d_workspace", B, N, cin, cout, k)) return rc;
    *bytes = work_layout(B, N, cin, cout, k).floats * sizeof(float);
    return QGX_OK;
}

int qgx_conv2d_forward(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t B, int N, int cin,
                       int cout, int k, void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_conv2d_forward";
    if (const int rc = conv_shape_check(what, B, N, cin, cout, k)) return rc;
    CONV_PTR(what, x_dev); CONV_PTR(what, w_dev); CONV_PTR(what, y_dev);
    QGX_REQUIRE(aligned16(bias_dev), "%s: bias_dev is not 16-byte aligned", what);
    if (const int rc = conv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    return conv_run(what, x_dev, w_dev, bias_dev, y_dev, (int)B, N, cin, cout, k, 0, (float *)work_dev,
                    work_layout(B, N, cin, cout, k), (hipStream_t)stream);
}

int qgx_conv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout, int k,
                             void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_conv2d_backward_data";
    if (const int rc = conv_shape_check(what, B, N, cin, cout, k)) return rc;
    CONV_PTR(what, dy_dev); CONV_PTR(what, w_dev); CONV_PTR(what, dx_dev);
    if (const int rc = conv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    return conv_run(what, dy_dev, w_dev, nullptr, dx_dev, (int)B, N, cout, cin, k, 1, (float *)work_dev,
                    work_layout(B, N, cin, cout, k), (hipStream_t)stream);
}

int qgx_conv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, float *db_dev, int64_t B, int N, int cin,
                               int cout, int k, void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_conv2d_backward_weight";
    if (const int rc = conv_shape_check(what, B, N, cin, cout, k)) return rc;
    CONV_PTR(what, x_dev); CONV_PTR(what, dy_dev); CONV_PTR(what, dw_dev);
    QGX_REQUIRE(aligned16(db_dev), "%s: db_dev is not 16-byte aligned", what);
    if (const int rc = conv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const WgradPlan p = wgrad_plan(B, N, cin, cout, k);
    const WorkLayout L = work_layout(B, N, cin, cout, k);
    float *ws = (float *)work_dev;
    QGX_REQUIRE(p.R > 0 && p.lds <= 160 * 1024, "%s: LDS patches %zu B too large for N = %d", what, p.lds, N);
    WgradArgs a = {};
    a.x = x_dev; a.dy = dy_dev; a.part = ws + L.part;
    a.N = N; a.R = p.R; a.ks = k; a.cin8 = round_up(cin, 8); a.cout8 = round_up(cout, 8); a.cit_n = p.cit_n;
    a.U = p.U; a.ups = p.ups; a.tiles_per_img = N / p.R;
    const int pairs = p.cot_n * p.cit_n;
    dim3 grid(pairs, p.S), block(256);
    if (const int rc = k == 3 ? launch_conv_kernel(k_wgrad<3>, grid, block, p.lds, st, a)
                              : launch_conv_kernel(k_wgrad<7>, grid, block, p.lds, st, a)) return rc;
    const int slice = pairs * p.T * 1024;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(slice / 64), dim3(64 * RED_WAVES), 0, st, (const float *)(ws + L.part), dw_dev, p.S,
                       p.cit_n, p.T, cin, cout, slice);
    QGX_HIP(hipGetLastError());
    if (db_dev) {
        hipLaunchKernelGGL(k_dbias, dim3(p.nb), dim3(256), 0, st, dy_dev, ws + L.bpart, (int64_t)(B * N * N), p.ppb, a.cout8);
        QGX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_dbias_reduce, dim3(1), dim3(256), 0, st, (const float *)(ws + L.bpart), db_dev, p.nb, a.cout8, cout);
        QGX_HIP(hipGetLastError());
    }
    return QGX_OK;
}

}  // extern "C"
