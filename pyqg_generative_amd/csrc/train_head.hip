// The two ends of a convolutional net's training step (include/qgx_head_train.h): the batch gather in front of the first
// convolution and the loss head behind the last.  Every kernel gives one lane a pixel: its record of 8 floats in the engine
// layout is one or two 16-byte accesses (the second only for C > 4), and the C planar values of the pixel are read or written
// coalesced along x, one 256-byte row piece per wave and channel.  These kernels move a few bytes per pixel and are bound by
// their launch, not by bandwidth: what they buy is ONE launch where torch runs a gather, a fill, a permuted copy, a slice, a
// softplus and a mean (and autograd the backward of each), and a loss whose bits do not depend on the order workgroups ran in.
//
//   k_gather        out[b] = src[idx[b]], planar -> engine layout, pad channels written as zero
//   k_head_loss     block blk adds (h(y) - t)^2 over the pixels [blk ppb, (blk + 1) ppb): a thread its pixels p0 + t, p0 + t + 256,
//                   ... in order, in float64 from the first add; the 64 lanes by a shuffle tree in registers, the four waves in
//                   order through LDS; one float64 per block into the workspace
//   k_head_finish   one block adds the partials (thread t: t, t + 256, ... in order, then the same tree) and divides once
//   k_head_grad     dy = s (h(y) - t) h'(y), s read from the device as float64 and rounded once; pad channels zero
//   k_head_apply    planar h(y), or (t - h(y))^2
#include "common.hpp"

namespace qgx {

constexpr int HEAD_BLOCK = 256;
constexpr int HEAD_MAX_PARTIALS = 1024;

template <int MODE>
__device__ __forceinline__ float head_value(float y) {
    if (MODE == QGX_HEAD_SOFTPLUS_MSE) return y > 20.f ? y : log1pf(expf(y));
    return y;
}
template <int MODE>
__device__ __forceinline__ float head_slope(float y) {
    if (MODE == QGX_HEAD_SOFTPLUS_MSE) {
        const float e = expf(y);
        return y > 20.f ? 1.f : e / (1.f + e);
    }
    return 1.f;
}

struct Pixel {
    int r;           // offset of the pixel in its image plane
    int64_t row;     // row of the planar array that batch member b reads
};
__device__ __forceinline__ Pixel pixel_of(int p, int NN, const int64_t *idx) {
    const int b = p / NN;
    Pixel q;
    q.r = p - b * NN;
    q.row = idx ? idx[b] : (int64_t)b;
    return q;
}
// the record of pixel p: channels 0 ... 7 (4 ... 7 are not read for C <= 4: they are pad channels)
__device__ __forceinline__ void load_record(const float *y, int p, int C, float (&v)[8]) {
    const float4 *rec = reinterpret_cast<const float4 *>(y) + (size_t)p * 2;
    const float4 a = rec[0];
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (C > 4) b = rec[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store_record(float *out, int p, const float (&v)[8]) {
    float4 *rec = reinterpret_cast<float4 *>(out) + (size_t)p * 2;
    rec[0] = make_float4(v[0], v[1], v[2], v[3]);
    rec[1] = make_float4(v[4], v[5], v[6], v[7]);
}

__global__ __launch_bounds__(HEAD_BLOCK) void k_gather(const float *src, const int64_t *idx, float *out, int NN, int C, int npix) {
    const int p = blockIdx.x * HEAD_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const Pixel q = pixel_of(p, NN, idx);
    const float *s = src + (size_t)q.row * C * NN + q.r;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        v[c] = 0.f;
        if (c < C) v[c] = s[(size_t)c * NN];
    }
    store_record(out, p, v);
}

// the sum of v over the block's 256 threads, valid in thread 0: lanes by a fixed shuffle tree, waves in order
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < HEAD_BLOCK / 64; ++w) s += red[w];
    return s;
}

template <int MODE>
__global__ __launch_bounds__(HEAD_BLOCK) void k_head_loss(const float *y, const float *t, const int64_t *idx, double *part, int NN,
                                                          int C, int npix, int ppb) {
    __shared__ double red[HEAD_BLOCK / 64];
    const int p0 = blockIdx.x * ppb, p1 = p0 + ppb < npix ? p0 + ppb : npix;
    double acc = 0.0;
    for (int p = p0 + threadIdx.x; p < p1; p += HEAD_BLOCK) {
        const Pixel q = pixel_of(p, NN, idx);
        const float *tp = t + (size_t)q.row * C * NN + q.r;
        float v[8];
        load_record(y, p, C, v);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < C) {
                const float d = head_value<MODE>(v[c]) - tp[(size_t)c * NN];
                acc += (double)d * (double)d;
            }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(HEAD_BLOCK) void k_head_finish(const double *part, double *loss, int nb, double count) {
    __shared__ double red[HEAD_BLOCK / 64];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nb; k += HEAD_BLOCK) acc += part[k];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) *loss = s / count;
}

template <int MODE>
__global__ __launch_bounds__(HEAD_BLOCK) void k_head_grad(const float *y, const float *t, const int64_t *idx, const double *gout,
                                                          float *dy, int NN, int C, int npix, double count) {
    const int p = blockIdx.x * HEAD_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const float s = (float)(*gout * 2.0 / count);
    const Pixel q = pixel_of(p, NN, idx);
    const float *tp = t + (size_t)q.row * C * NN + q.r;
    float v[8], g[8];
    load_record(y, p, C, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        g[c] = 0.f;
        if (c < C) {
            const float d = head_value<MODE>(v[c]) - tp[(size_t)c * NN];
            g[c] = (s * d) * head_slope<MODE>(v[c]);
        }
    }
    store_record(dy, p, g);
}

template <int MODE, bool RESIDUAL>
__global__ __launch_bounds__(HEAD_BLOCK) void k_head_apply(const float *y, const float *t, const int64_t *idx, float *out, int NN,
                                                           int C, int npix) {
    const int p = blockIdx.x * HEAD_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const int b = p / NN, r = p - b * NN;
    const float *tp = nullptr;
    if (RESIDUAL) tp = t + (size_t)(idx ? idx[b] : (int64_t)b) * C * NN + r;
    float *op = out + (size_t)b * C * NN + r;
    float v[8];
    load_record(y, p, C, v);
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < C) {
            float h = head_value<MODE>(v[c]);
            if (RESIDUAL) {
                const float d = tp[(size_t)c * NN] - h;
                h = d * d;
            }
            op[(size_t)c * NN] = h;
        }
}

// ---- host side -------------------------------------------------------------------------------
// The loss's partition, a function of (B, N) alone: at most HEAD_MAX_PARTIALS ranges of ppb pixels, ppb a multiple of the block
struct HeadPlan { int nb, ppb; };
static HeadPlan head_plan(int64_t B, int N) {
    const int64_t npix = B * N * N;
    int64_t nb = (npix + HEAD_BLOCK - 1) / HEAD_BLOCK;
    if (nb > HEAD_MAX_PARTIALS) nb = HEAD_MAX_PARTIALS;
    const int64_t ppb = ((npix + nb - 1) / nb + HEAD_BLOCK - 1) / HEAD_BLOCK * HEAD_BLOCK;
    HeadPlan p;
    p.ppb = (int)ppb;
    p.nb = (int)((npix + ppb - 1) / ppb);
    return p;
}
static size_t head_work_bytes(int64_t B, int N) { return ((size_t)head_plan(B, N).nb * sizeof(double) + 255) / 256 * 256; }

static int head_grid_check(const char *what, int64_t B, int N) {
    QGX_REQUIRE(N == 16 || N == 32 || N == 48 || N == 64 || N == 96 || N == 128, "%s: N = %d, expected 16, 32, 48, 64, 96 or 128", what, N);
    QGX_REQUIRE(B >= 1 && B <= ((int64_t)1 << 29) / (N * N), "%s: B = %lld, expected 1 ... 2^29 / N^2", what, (long long)B);
    return QGX_OK;
}
static int head_shape_check(const char *what, int64_t B, int N, int C) {
    if (const int rc = head_grid_check(what, B, N)) return rc;
    QGX_REQUIRE(C >= 1 && C <= 8, "%s: C = %d, expected 1 ... 8", what, C);
    return QGX_OK;
}
// the planar array of n rows that idx (or, without it, the batch member's own number) points into
static int head_rows_check(const char *what, int64_t n, int64_t B, const void *idx_dev) {
    QGX_REQUIRE(n >= 1, "%s: n = %lld, expected >= 1", what, (long long)n);
    QGX_REQUIRE(idx_dev || n >= B, "%s: n = %lld rows for B = %lld without idx_dev", what, (long long)n, (long long)B);
    return QGX_OK;
}
static int head_mode_check(const char *what, int mode) {
    QGX_REQUIRE(mode == QGX_HEAD_MSE || mode == QGX_HEAD_SOFTPLUS_MSE, "%s: mode = %d, expected QGX_HEAD_MSE (0) or QGX_HEAD_SOFTPLUS_MSE (1)", what, mode);
    return QGX_OK;
}
static bool head_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define HEAD_PTR(what, p)                                                                                  \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(head_aligned16(p), "%s: " #p " is not 16-byte aligned", what);                         \
    } while (0)
#define HEAD_OPTIONAL_PTR(what, p) QGX_REQUIRE(head_aligned16(p), "%s: " #p " is not 16-byte aligned", what)

static dim3 pixel_grid(int npix) { return dim3((npix + HEAD_BLOCK - 1) / HEAD_BLOCK); }

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_batch_gather(const float *src_dev, const int64_t *idx_dev, float *out_dev, int64_t n, int64_t B, int N, int C,
                     void *stream) {
    const char *what = "qgx_batch_gather";
    if (const int rc = head_shape_check(what, B, N, C)) return rc;
    if (const int rc = head_rows_check(what, n, B, idx_dev)) return rc;
    HEAD_PTR(what, src_dev); HEAD_PTR(what, out_dev); HEAD_OPTIONAL_PTR(what, idx_dev);
    const int NN = N * N, npix = (int)(B * NN);
    hipLaunchKernelGGL(k_gather, pixel_grid(npix), dim3(HEAD_BLOCK), 0, (hipStream_t)stream, src_dev, idx_dev, out_dev, NN, C, npix);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

int qgx_head_workspace(int64_t B, int N, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_head_workspace: bytes is NULL");
    if (const int rc = head_grid_check("qgx_head_workspace", B, N)) return rc;
    *bytes = head_work_bytes(B, N);
    return QGX_OK;
}

int qgx_head_loss(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, double *loss_dev, int64_t B, int N,
                  int C, int64_t n, void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_head_loss";
    if (const int rc = head_shape_check(what, B, N, C)) return rc;
    if (const int rc = head_rows_check(what, n, B, idx_dev)) return rc;
    if (const int rc = head_mode_check(what, mode)) return rc;
    HEAD_PTR(what, y_dev); HEAD_PTR(what, t_dev); HEAD_OPTIONAL_PTR(what, idx_dev); HEAD_PTR(what, loss_dev);
    HEAD_PTR(what, work_dev);
    const size_t need = head_work_bytes(B, N);
    QGX_REQUIRE(work_bytes >= need, "%s: work_bytes = %zu, qgx_head_workspace gives %zu", what, work_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const HeadPlan p = head_plan(B, N);
    const int NN = N * N, npix = (int)(B * NN);
    double *part = (double *)work_dev;
    if (mode == QGX_HEAD_MSE)
        hipLaunchKernelGGL(k_head_loss<QGX_HEAD_MSE>, dim3(p.nb), dim3(HEAD_BLOCK), 0, st, y_dev, t_dev, idx_dev, part, NN, C, npix, p.ppb);
    else
        hipLaunchKernelGGL(k_head_loss<QGX_HEAD_SOFTPLUS_MSE>, dim3(p.nb), dim3(HEAD_BLOCK), 0, st, y_dev, t_dev, idx_dev, part, NN, C, npix, p.ppb);
    QGX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_head_finish, dim3(1), dim3(HEAD_BLOCK), 0, st, (const double *)part, loss_dev, p.nb, (double)(B * C * NN));
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

int qgx_head_grad(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, const double *gout_dev,
                  float *dy_dev, int64_t B, int N, int C, int64_t n, void *stream) {
    const char *what = "qgx_head_grad";
    if (const int rc = head_shape_check(what, B, N, C)) return rc;
    if (const int rc = head_rows_check(what, n, B, idx_dev)) return rc;
    if (const int rc = head_mode_check(what, mode)) return rc;
    HEAD_PTR(what, y_dev); HEAD_PTR(what, t_dev); HEAD_OPTIONAL_PTR(what, idx_dev); HEAD_PTR(what, gout_dev);
    HEAD_PTR(what, dy_dev);
    hipStream_t st = (hipStream_t)stream;
    const int NN = N * N, npix = (int)(B * NN);
    const double count = (double)(B * C * NN);
    if (mode == QGX_HEAD_MSE)
        hipLaunchKernelGGL(k_head_grad<QGX_HEAD_MSE>, pixel_grid(npix), dim3(HEAD_BLOCK), 0, st, y_dev, t_dev, idx_dev, gout_dev, dy_dev, NN, C, npix, count);
    else
        hipLaunchKernelGGL(k_head_grad<QGX_HEAD_SOFTPLUS_MSE>, pixel_grid(npix), dim3(HEAD_BLOCK), 0, st, y_dev, t_dev, idx_dev, gout_dev, dy_dev, NN, C, npix, count);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

int qgx_head_apply(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, float *out_dev, int64_t B, int N,
                   int C, int64_t n, void *stream) {
    const char *what = "qgx_head_apply";
    if (const int rc = head_shape_check(what, B, N, C)) return rc;
    if (t_dev)
        if (const int rc = head_rows_check(what, n, B, idx_dev)) return rc;
    if (const int rc = head_mode_check(what, mode)) return rc;
    HEAD_PTR(what, y_dev); HEAD_OPTIONAL_PTR(what, t_dev); HEAD_OPTIONAL_PTR(what, idx_dev); HEAD_PTR(what, out_dev);
    hipStream_t st = (hipStream_t)stream;
    const int NN = N * N, npix = (int)(B * NN);
    const dim3 grid = pixel_grid(npix), block(HEAD_BLOCK);
    const bool soft = mode == QGX_HEAD_SOFTPLUS_MSE;
    if (t_dev && soft)
        hipLaunchKernelGGL((k_head_apply<QGX_HEAD_SOFTPLUS_MSE, true>), grid, block, 0, st, y_dev, t_dev, idx_dev, out_dev, NN, C, npix);
    else if (t_dev)
        hipLaunchKernelGGL((k_head_apply<QGX_HEAD_MSE, true>), grid, block, 0, st, y_dev, t_dev, idx_dev, out_dev, NN, C, npix);
    else if (soft)
        hipLaunchKernelGGL((k_head_apply<QGX_HEAD_SOFTPLUS_MSE, false>), grid, block, 0, st, y_dev, t_dev, idx_dev, out_dev, NN, C, npix);
    else
        hipLaunchKernelGGL((k_head_apply<QGX_HEAD_MSE, false>), grid, block, 0, st, y_dev, t_dev, idx_dev, out_dev, NN, C, npix);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // extern "C"
