// ANNModel's pointwise stencil network (pyqg_generative/models/ann_model.py; net: tools/cnn_tools.py:184-210, ANN) on
// gfx950.  Every grid point of every single-channel image (member, layer) is mapped by ONE small MLP to one forcing value:
//   x_f = float32(q[(y + dy - s/2) mod N, (x + dx - s/2) mod N]) / x_scale,    f = dy * s + dx     (xarray_to_stencil,
//                                                                                                    cnn_tools.py:321-339)
//   y   = Linear(h_last, 1)(ReLU(... ReLU(Linear(s*s, h0)(x))))                                     (ann_model.py:82-93)
//   scale_invariant: y = |x|^2 * layers(x / |x|), |x| the 2-norm of the s*s stencil values (ANN degree = 2)
// in float32.  The kernel reads q (float64) directly: a workgroup stages its tile of rows plus the wrapped halo in LDS
// (converted and divided by x_scale once per value), then every thread evaluates the net for two points.
// Summation order: each neuron starts from its bias and adds its inputs in index order with one fmaf each; nothing depends
// on the ensemble size, the tile or the stream, so a member's output is bitwise the same in any launch.
// ReLU is  v < 0 ? 0 : v : a NaN (the 0/0 of a zero-norm stencil under scale_invariant) propagates as it does in torch,
// where fmaxf(NaN, 0) would return 0.
// Weights are wave-uniform.  The default net (3 x 3, [24, 24]) is specialised: its loops are unrolled, every weight index
// is a constant, and the weights are scalar-loaded (SGPR operands of the packed FMAs, two points per lane).  Other shapes
// (odd s <= 7, 1-4 hidden layers of width <= 128) take a generic kernel with run-time loops.
#include "common.hpp"
#include <new>

namespace qgx {

typedef float ann_f2 __attribute__((ext_vector_type(2)));

constexpr int ANN_THREADS = 256;
constexpr int ANN_PTS = 2 * ANN_THREADS;     // points per tile: two per thread
constexpr int ANN_LDS = 4096;                // floats of the staged tile: (rows + 2h) (N + 2h) <= 7 * 518 at N = 512
constexpr int ANN_MAX_N = 512;

struct AnnArgs {
    const float *w;           // per linear layer l: W_l (out, in) row-major at off_w[l], b_l (out) at off_b[l]
    int s, nl, si;            // stencil size, linear layers (hidden + 1), scale_invariant
    int width[6];             // width[0] = s * s, width[1 .. nl-1] = hidden, width[nl] = 1
    int off_w[5], off_b[5];
};

struct Ann {
    AnnArgs a;
    float *w = nullptr;
};

// tile rows: at most ANN_PTS points per workgroup, at most the whole image
static inline int ann_tile_rows(int N) {
    int r = ANN_PTS / N;
    if (r < 1) r = 1;
    return r > N ? N : r;
}

// rows r0 - h .. r0 + rows + h - 1 and columns -h .. N + h - 1 of one image, wrapped, as float(v) / xs
template <typename T>
__device__ inline void ann_stage(float *t, const T *img, float xs, int N, int r0, int rows, int h) {
    const int W = N + 2 * h, n = (rows + 2 * h) * W;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = i / W, c = i - r * W;
        int gy = (r0 + r - h) % N, gx = (c - h) % N;
        gy += gy < 0 ? N : 0;
        gx += gx < 0 ? N : 0;
        t[i] = (float)img[(size_t)gy * N + gx] / xs;
    }
}

__device__ inline float ann_relu(float v) { return v < 0.f ? 0.f : v; }    // NaN stays NaN
__device__ inline ann_f2 ann_relu(ann_f2 v) { return ann_f2{ann_relu(v.x), ann_relu(v.y)}; }
__device__ inline ann_f2 ann_fma(ann_f2 a, float w, ann_f2 c) { return __builtin_elementwise_fma(a, ann_f2{w, w}, c); }

// The default net, 3 x 3 stencil, hidden [24, 24]: two points per thread (p and p + 256 of the tile), packed FMAs.
// Layer 2 and the output layer are interleaved: hidden neuron j of layer 2 is finished, rectified and added to the output
// (in the order j = 0 .. 23, as the output neuron sums them) before neuron j + 1 starts.
template <typename T, bool SI>
__global__ __launch_bounds__(ANN_THREADS, 8) void k_ann_s3h24(const T *__restrict__ in, float xs, const float *__restrict__ w,
                                                           float *__restrict__ y, int N, int TR, int tiles) {
    constexpr int S = 3, F = 9, H = 24;
    constexpr int W1 = 0, B1 = W1 + H * F, W2 = B1 + H, B2 = W2 + H * H, W3 = B2 + H, B3 = W3 + H;
    __shared__ float t[ANN_LDS];
    const int64_t img = blockIdx.x / tiles;
    const int r0 = (blockIdx.x % tiles) * TR;
    const int rows = min(TR, N - r0);
    const size_t npix = (size_t)N * N;
    ann_stage(t, in + img * npix, xs, N, r0, rows, 1);
    __syncthreads();
    const int np = rows * N, LW = N + 2;
    const int p0 = threadIdx.x, p1 = threadIdx.x + ANN_THREADS;
    const int c0 = p0 < np ? p0 : 0, c1 = p1 < np ? p1 : 0;      // a point past the tile computes point 0 and is not stored
    const int o0 = (c0 / N) * LW + c0 % N, o1 = (c1 / N) * LW + c1 % N;
    ann_f2 x[F];
#pragma unroll
    for (int dy = 0; dy < S; ++dy)
#pragma unroll
        for (int dx = 0; dx < S; ++dx) x[dy * S + dx] = ann_f2{t[o0 + dy * LW + dx], t[o1 + dy * LW + dx]};
    ann_f2 n2 = ann_f2{0.f, 0.f};
    if (SI) {
        n2 = x[0] * x[0];
#pragma unroll
        for (int f = 1; f < F; ++f) n2 = __builtin_elementwise_fma(x[f], x[f], n2);
        const ann_f2 nrm = ann_f2{sqrtf(n2.x), sqrtf(n2.y)};
#pragma unroll
        for (int f = 0; f < F; ++f) x[f] = x[f] / nrm;
        n2 = nrm * nrm;                                         // norm ** 2 (torch: pow(norm, 2) = norm * norm)
    }
    ann_f2 h[H];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        ann_f2 acc = ann_f2{w[B1 + j], w[B1 + j]};
#pragma unroll
        for (int f = 0; f < F; ++f) acc = ann_fma(x[f], w[W1 + j * F + f], acc);
        h[j] = ann_relu(acc);
    }
    ann_f2 out = ann_f2{w[B3], w[B3]};
#pragma unroll
    for (int j = 0; j < H; ++j) {
        ann_f2 acc = ann_f2{w[B2 + j], w[B2 + j]};
#pragma unroll
        for (int i = 0; i < H; ++i) acc = ann_fma(h[i], w[W2 + j * H + i], acc);
        out = ann_fma(ann_relu(acc), w[W3 + j], out);
    }
    if (SI) out = n2 * out;
    float *yi = y + img * npix + (size_t)r0 * N;
    if (p0 < np) yi[p0] = out.x;
    if (p1 < np) yi[p1] = out.y;
}

// Any admitted shape: run-time loops, activations in per-thread arrays, the same summation order as the default kernel.
template <typename T>
__global__ __launch_bounds__(ANN_THREADS) void k_ann_generic(const T *__restrict__ in, float xs, AnnArgs a,
                                                             float *__restrict__ y, int N, int TR, int tiles) {
    __shared__ float t[ANN_LDS];
    const int64_t img = blockIdx.x / tiles;
    const int r0 = (blockIdx.x % tiles) * TR;
    const int rows = min(TR, N - r0);
    const size_t npix = (size_t)N * N;
    const int S = a.s, h = S / 2, F = S * S, LW = N + 2 * h;
    ann_stage(t, in + img * npix, xs, N, r0, rows, h);
    __syncthreads();
    const int np = rows * N;
    float *yi = y + img * npix + (size_t)r0 * N;
    for (int p = threadIdx.x; p < np; p += ANN_THREADS) {
        float buf[2][128];
        float x[49];
        const int o = (p / N) * LW + p % N;
        for (int dy = 0; dy < S; ++dy)
            for (int dx = 0; dx < S; ++dx) x[dy * S + dx] = t[o + dy * LW + dx];
        float n2 = 0.f;
        if (a.si) {
            n2 = x[0] * x[0];
            for (int f = 1; f < F; ++f) n2 = fmaf(x[f], x[f], n2);
            const float nrm = sqrtf(n2);
            for (int f = 0; f < F; ++f) x[f] = x[f] / nrm;
            n2 = nrm * nrm;
        }
        const float *cur = x;
        float out = 0.f;
        for (int l = 0; l < a.nl; ++l) {
            const int nin = a.width[l], nout = a.width[l + 1];
            const float *W = a.w + a.off_w[l], *b = a.w + a.off_b[l];
            float *nxt = buf[l & 1];
            for (int j = 0; j < nout; ++j) {
                float acc = b[j];
                for (int i = 0; i < nin; ++i) acc = fmaf(cur[i], W[j * nin + i], acc);
                if (l + 1 < a.nl) nxt[j] = ann_relu(acc);
                else out = acc;
            }
            cur = nxt;
        }
        yi[p] = a.si ? n2 * out : out;
    }
}

// The shape rules of qgx_generator_create_ann, checked before any HIP call.
int ann_check(const qgx_ann_weights *w) {
    QGX_REQUIRE(w, "qgx_generator_create_ann: null weights");
    QGX_REQUIRE(w->stencil_size >= 1 && w->stencil_size <= 7 && (w->stencil_size & 1),
                "qgx_generator_create_ann: stencil_size %d (odd, 1 ... 7)", w->stencil_size);
    QGX_REQUIRE(w->n_hidden >= 1 && w->n_hidden <= 4, "qgx_generator_create_ann: %d hidden layers (1 ... 4)", w->n_hidden);
    for (int l = 0; l < w->n_hidden; ++l)
        QGX_REQUIRE(w->hidden[l] >= 1 && w->hidden[l] <= 128, "qgx_generator_create_ann: hidden layer %d has width %d (1 ... 128)",
                    l, w->hidden[l]);
    for (int l = 0; l <= w->n_hidden; ++l)
        QGX_REQUIRE(w->w[l] && w->b[l], "qgx_generator_create_ann: layer %d: null weight or bias", l);
    return QGX_OK;
}

void ann_destroy(Ann *a) {
    if (!a) return;
    if (a->w) (void)hipFree(a->w);
    delete a;
}

int ann_create(const qgx_ann_weights *w, Ann **out) {
    int rc = ann_check(w);
    if (rc) return rc;
    Ann *n = new (std::nothrow) Ann();
    if (!n) { set_error("out of host memory"); return QGX_ERR_NOMEM; }
    AnnArgs &a = n->a;
    a.s = w->stencil_size; a.nl = w->n_hidden + 1; a.si = w->scale_invariant ? 1 : 0;
    a.width[0] = a.s * a.s;
    for (int l = 0; l < w->n_hidden; ++l) a.width[l + 1] = w->hidden[l];
    a.width[a.nl] = 1;
    std::vector<float> host;
    for (int l = 0; l < a.nl; ++l) {
        const size_t nw = (size_t)a.width[l + 1] * a.width[l];
        a.off_w[l] = (int)host.size();
        host.insert(host.end(), w->w[l], w->w[l] + nw);
        a.off_b[l] = (int)host.size();
        host.insert(host.end(), w->b[l], w->b[l] + a.width[l + 1]);
    }
    hipError_t e = hipMalloc((void **)&n->w, host.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(n->w, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("qgx_generator_create_ann: %s", hipGetErrorString(e));
        ann_destroy(n);
        return QGX_ERR_HIP;
    }
    a.w = n->w;
    *out = n;
    return QGX_OK;
}

// the specialised kernel applies: 3 x 3 stencil, two hidden layers of 24
static bool ann_default_shape(const AnnArgs &a) {
    return a.s == 3 && a.nl == 3 && a.width[1] == 24 && a.width[2] == 24;
}

template <typename T>
static int ann_launch(const Ann *n, const T *in, float xs, float *y, int64_t n_img, int N, hipStream_t st) {
    QGX_REQUIRE(n && in && y && n_img > 0, "ann_forward: bad argument");
    QGX_REQUIRE(N >= 1 && N <= ANN_MAX_N, "ANN generator: N = %d (1 ... %d)", N, ANN_MAX_N);
    const int TR = ann_tile_rows(N), tiles = (N + TR - 1) / TR;
    const int64_t blocks = n_img * tiles;
    QGX_REQUIRE(blocks <= 0x7fffffff, "ANN generator: %lld workgroups", (long long)blocks);
    const AnnArgs &a = n->a;
    if (ann_default_shape(a)) {
        if (a.si) hipLaunchKernelGGL((k_ann_s3h24<T, true>), dim3((unsigned)blocks), dim3(ANN_THREADS), 0, st, in, xs, a.w, y, N, TR, tiles);
        else hipLaunchKernelGGL((k_ann_s3h24<T, false>), dim3((unsigned)blocks), dim3(ANN_THREADS), 0, st, in, xs, a.w, y, N, TR, tiles);
    } else {
        hipLaunchKernelGGL(k_ann_generic<T>, dim3((unsigned)blocks), dim3(ANN_THREADS), 0, st, in, xs, a, y, N, TR, tiles);
    }
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

// q (n_img, N, N) float64 PV, each value float32(q) / x_scale; or x (n_img, N, N) float32 already normalised
int ann_forward_q(const Ann *n, const double *q, float x_scale, float *y, int64_t n_img, int N, hipStream_t st) {
    return ann_launch(n, q, x_scale, y, n_img, N, st);
}
int ann_forward_x(const Ann *n, const float *x, float *y, int64_t n_img, int N, hipStream_t st) {
    return ann_launch(n, x, 1.f, y, n_img, N, st);      // v / 1 is v: the same kernels on normalised input
}

}  // namespace qgx
