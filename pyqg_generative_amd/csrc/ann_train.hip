// Training of ANNModel's pointwise stencil network (pyqg_generative/models/ann_model.py:34-52 fit; tools/cnn_tools.py:373-396
// prepare_data_ANN, :645-700 train) on gfx950: stencil rows, loss + gradient of a batch, Adam.  include/qgx_train.h.
//
// One step is about 0.15 GFLOP and 1.3 MB of reads at the reference's batch of 2^15 rows: a microsecond of arithmetic, so a
// step is bound by launches and dependent latencies, and it is two launches:
//   k_ann_grad    one workgroup of 256 threads per TILE of rows (128 rows, fewer for nets whose activations do not fit).
//                 Phase A, one thread per row: gather the row, forward, the error, backward to the delta of every layer's
//                 pre-activation; activations and deltas go to LDS as COLUMNS (one column per neuron, one entry per row).
//                 Phase B, one thread per (neuron j, four inputs i .. i + 3) of a layer: dW[j][i] = sum over the tile's rows,
//                 in row order, of delta[j][row] * a[i][row], one fmaf each (the bias is the input "1": a column of ones).
//                 A workgroup adds its tiles in order into ITS slice of the partial-sum work space.
//   k_ann_update  per parameter: the workgroups' partial sums in 16 fixed slices, each in order, the slices then added in
//                 order -> the gradient; then Adam.  Its first workgroup adds the loss partials in a fixed tree.
// Nothing depends on the stream or on timing: the partition is a function of the batch size alone, every sum has a fixed
// order, there are no float atomics.  qgx_ann_trainer_grad, _adam and _step run the SAME update kernel with a mode word, so
// _step is _grad then _adam bit for bit.
// The default net (3 x 3, [24, 24]) has its phase A specialised as ann.hip's inference kernel is: activations in registers,
// loops unrolled, weights staged in LDS.  Every other admitted shape takes run-time loops over the LDS columns.
// ReLU and its mask as torch: v < 0 ? 0 : v lets NaN through, and so does the mask, relu(v) <= 0 ? 0 : delta.
#include "common.hpp"
#include <cmath>
#include <new>

struct qgx_ann_trainer {
    int device = 0;
    int P = 0;                       // floats of one packed vector
    float *vec[4] = {nullptr, nullptr, nullptr, nullptr};   // params, grad, m, v
    float *part = nullptr;           // (TR_MAX_PARTS, P) partial sums
    double *part_loss = nullptr;     // (TR_MAX_PARTS)
    void *args_dev = nullptr;        // TrainArgs
    int64_t steps = 0;               // Adam steps taken
    int RT = 0;
    bool dflt = false, si = false;
    int F = 0;
};

namespace qgx {

constexpr int TR_THREADS = 256;      // threads of a gradient workgroup
constexpr int TR_ROWS = 128;         // rows of a full tile: phase A runs on the first TR_ROWS threads, phase B on all
constexpr int TR_PAD = 4;            // a column holds RT + TR_PAD floats: 16-byte aligned, and 132 = 4 mod 64 spreads the banks
constexpr int TR_MAX_PARTS = 256;    // workgroups of a gradient launch at most
constexpr int TR_LDS = 15000;        // floats of the tile's columns (58.6 KiB)
constexpr int TR_WDEF = 868;         // the default net's 865 parameters, staged in LDS by its workgroups
constexpr int TR_SLICES = 16;        // update kernel: 64 parameters x 16 slices of the partial sums
constexpr int TR_UPD = 64 * TR_SLICES;
enum { UPD_REDUCE = 1, UPD_ADAM = 2, UPD_LOSS = 4 };

struct TrainArgs {
    int s, nl, si;            // stencil size, linear layers, scale_invariant
    int width[6];             // width[0] = s * s, hidden ..., width[nl] = 1
    int off_w[5], off_b[5];   // packed offsets of W_l (out, in) and b_l
    int act[5], del[5];       // first LDS column of layer l's input activations / of its pre-activation deltas
    int ones;                 // the column of ones
    int item0[6];             // phase B: first work item of layer l; item0[nl] = all
    int RT, P;
};

struct BatchArgs {
    const float *x, *y;
    const int64_t *idx;       // or null: rows 0 .. n - 1
    int64_t n, tiles;
    float xs, ys, gscale;     // gscale = 2 / n
    int fwd_only;
};

struct AdamArgs { float w1, b2, c2, bc2s, eps, step; };

__device__ inline float tr_relu(float v) { return v < 0.f ? 0.f : v; }    // NaN stays NaN

// Phase A of the default net for one row: everything in registers, then stored as columns.  c: the row's entry of column 0.
template <bool SI>
__device__ inline float train_row_default(const TrainArgs *a, const float *__restrict__ w, const float *__restrict__ xr, float xs,
                                          float yt, float gscale, int fwd_only, float *c, int RTP) {
    constexpr int F = 9, H = 24;
    constexpr int W1 = 0, B1 = W1 + H * F, W2 = B1 + H, B2 = W2 + H * H, W3 = B2 + H, B3 = W3 + H;
    float x[F], h1[H], h2[H];
#pragma unroll
    for (int f = 0; f < F; ++f) x[f] = xr[f] / xs;
    float n2 = 0.f;
    if (SI) {
        n2 = x[0] * x[0];
#pragma unroll
        for (int f = 1; f < F; ++f) n2 = fmaf(x[f], x[f], n2);
        const float nrm = sqrtf(n2);
#pragma unroll
        for (int f = 0; f < F; ++f) x[f] = x[f] / nrm;
        n2 = nrm * nrm;
    }
#pragma unroll
    for (int j = 0; j < H; ++j) {
        float acc = w[B1 + j];
#pragma unroll
        for (int f = 0; f < F; ++f) acc = fmaf(x[f], w[W1 + j * F + f], acc);
        h1[j] = tr_relu(acc);
    }
    float out = w[B3];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        float acc = w[B2 + j];
#pragma unroll
        for (int i = 0; i < H; ++i) acc = fmaf(h1[i], w[W2 + j * H + i], acc);
        h2[j] = tr_relu(acc);
        out = fmaf(h2[j], w[W3 + j], out);
    }
    const float e = (SI ? n2 * out : out) - yt;
    if (fwd_only) return e;
    // columns: act[0] = 0 .. 8, act[1] = 9 .. 32, act[2] = 33 .. 56, del[0] = 57 .. 80, del[1] = 81 .. 104, del[2] = 105
    constexpr int A0 = 0, A1 = F, A2 = F + H, D0 = F + 2 * H, D1 = D0 + H, D2 = D1 + H;
#pragma unroll
    for (int f = 0; f < F; ++f) c[(A0 + f) * RTP] = x[f];
#pragma unroll
    for (int j = 0; j < H; ++j) { c[(A1 + j) * RTP] = h1[j]; c[(A2 + j) * RTP] = h2[j]; }
    float d3 = gscale * e;
    if (SI) d3 *= n2;
    c[D2 * RTP] = d3;
    float d2[H];
#pragma unroll
    for (int j = 0; j < H; ++j) {
        d2[j] = h2[j] <= 0.f ? 0.f : d3 * w[W3 + j];
        c[(D1 + j) * RTP] = d2[j];
    }
#pragma unroll
    for (int i = 0; i < H; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < H; ++j) acc = fmaf(d2[j], w[W2 + j * H + i], acc);
        c[(D0 + i) * RTP] = h1[i] <= 0.f ? 0.f : acc;
    }
    return e;
}

// Phase A of any admitted net for one row: run-time loops over the LDS columns.
__device__ inline float train_row_generic(const TrainArgs *a, const float *__restrict__ w, const float *__restrict__ xr, float xs,
                                          float yt, float gscale, int fwd_only, float *c, int RTP) {
    const int F = a->width[0], nl = a->nl;
    float *A0 = c + a->act[0] * RTP;
    for (int f = 0; f < F; ++f) A0[f * RTP] = xr[f] / xs;
    float n2 = 0.f;
    if (a->si) {
        n2 = A0[0] * A0[0];
        for (int f = 1; f < F; ++f) n2 = fmaf(A0[f * RTP], A0[f * RTP], n2);
        const float nrm = sqrtf(n2);
        for (int f = 0; f < F; ++f) A0[f * RTP] = A0[f * RTP] / nrm;
        n2 = nrm * nrm;
    }
    float out = 0.f;
    for (int l = 0; l < nl; ++l) {
        const int nin = a->width[l], nout = a->width[l + 1];
        const float *W = w + a->off_w[l], *b = w + a->off_b[l];
        const float *in = c + a->act[l] * RTP;
        float *nxt = l + 1 < nl ? c + a->act[l + 1] * RTP : nullptr;
        for (int j = 0; j < nout; ++j) {
            float acc = b[j];
            for (int i = 0; i < nin; ++i) acc = fmaf(in[i * RTP], W[j * nin + i], acc);
            if (nxt) nxt[j * RTP] = tr_relu(acc);
            else out = acc;
        }
    }
    const float e = (a->si ? n2 * out : out) - yt;
    if (fwd_only) return e;
    float d = gscale * e;
    if (a->si) d *= n2;
    c[a->del[nl - 1] * RTP] = d;
    for (int l = nl - 1; l >= 1; --l) {
        const int nin = a->width[l], nout = a->width[l + 1];
        const float *W = w + a->off_w[l];
        const float *Dl = c + a->del[l] * RTP, *Al = c + a->act[l] * RTP;
        float *Dm = c + a->del[l - 1] * RTP;
        for (int i = 0; i < nin; ++i) {
            float acc = 0.f;
            for (int j = 0; j < nout; ++j) acc = fmaf(Dl[j * RTP], W[j * nin + i], acc);
            Dm[i * RTP] = Al[i * RTP] <= 0.f ? 0.f : acc;
        }
    }
    return e;
}

// the sum of v over the wave's lanes in a fixed tree (lane 0 holds it)
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// Phase B: the tile's contribution to every weight and bias gradient, into the workgroup's slice of the partial sums.
// rows4: the tile's rows rounded up to four (the entries rows .. rows4 - 1 of every column hold zeros): a column is read
// four rows at a time and summed in row order.
__device__ inline void train_phase_b(const TrainArgs *a, const float *lds, int rows4, float *__restrict__ part, bool first) {
    const int RTP = a->RT + TR_PAD, nl = a->nl;
    const int total = a->item0[nl];
    for (int it = threadIdx.x; it < total; it += TR_THREADS) {
        int l = 0;
        while (l + 1 < nl && it >= a->item0[l + 1]) ++l;
        const int nin = a->width[l], q = (nin + 4) / 4;          // blocks of four over the nin inputs and the bias
        const int k = it - a->item0[l], j = k / q, i0 = (k - j * q) * 4;
        const float4 *D = (const float4 *)(lds + (a->del[l] + j) * RTP);
        const float4 *c0 = (const float4 *)(lds + (i0 < nin ? a->act[l] + i0 : a->ones) * RTP);
        const float4 *c1 = (const float4 *)(lds + (i0 + 1 < nin ? a->act[l] + i0 + 1 : a->ones) * RTP);
        const float4 *c2 = (const float4 *)(lds + (i0 + 2 < nin ? a->act[l] + i0 + 2 : a->ones) * RTP);
        const float4 *c3 = (const float4 *)(lds + (i0 + 3 < nin ? a->act[l] + i0 + 3 : a->ones) * RTP);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 2
        for (int r = 0; r < rows4 / 4; ++r) {
            const float4 d = D[r], x0 = c0[r], x1 = c1[r], x2 = c2[r], x3 = c3[r];
            s0 = fmaf(d.w, x0.w, fmaf(d.z, x0.z, fmaf(d.y, x0.y, fmaf(d.x, x0.x, s0))));
            s1 = fmaf(d.w, x1.w, fmaf(d.z, x1.z, fmaf(d.y, x1.y, fmaf(d.x, x1.x, s1))));
            s2 = fmaf(d.w, x2.w, fmaf(d.z, x2.z, fmaf(d.y, x2.y, fmaf(d.x, x2.x, s2))));
            s3 = fmaf(d.w, x3.w, fmaf(d.z, x3.z, fmaf(d.y, x3.y, fmaf(d.x, x3.x, s3))));
        }
        const float s[4] = {s0, s1, s2, s3};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int i = i0 + kk;
            if (i <= nin) {
                const int o = i < nin ? a->off_w[l] + j * nin + i : a->off_b[l] + j;
                part[o] = first ? s[kk] : part[o] + s[kk];
            }
        }
    }
}

template <bool DEF, bool SI>
__global__ __launch_bounds__(TR_THREADS) void k_ann_grad(const TrainArgs *__restrict__ a, const float *__restrict__ w, BatchArgs b,
                                                         float *__restrict__ part, double *__restrict__ part_loss) {
    __shared__ __attribute__((aligned(16))) float lds[TR_LDS];
    __shared__ double wsum[TR_ROWS / 64];
    // the default net's weights from LDS (the same address in every lane: a broadcast read): with one wave per SIMD nothing
    // hides the latency of 865 scalar loads, and they do not fit the scalar registers
    __shared__ __attribute__((aligned(16))) float wl[DEF ? TR_WDEF : 4];
    const int RT = a->RT, RTP = RT + TR_PAD, F = a->width[0];
    const int tid = threadIdx.x;
    if (DEF)
        for (int i = tid; i < a->P; i += TR_THREADS) wl[i] = w[i];       // (visible after the tile loop's first barrier)
    for (int r = tid; r < RTP; r += TR_THREADS) lds[a->ones * RTP + r] = 1.f;
    double loss = 0.0;
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
        const int64_t r0 = tile * RT;
        const int64_t left = b.n - r0;
        const int rows = left < RT ? (int)left : RT;
        const int rows4 = (rows + 3) & ~3;       // <= RT: RT is a multiple of four
        __syncthreads();                         // the previous tile's phase B has read its columns
        float e = 0.f;
        if (tid < rows) {
            const int64_t row = b.idx ? b.idx[r0 + tid] : r0 + tid;
            const float *xr = b.x + row * F;
            const float yt = b.y[row] / b.ys;
            e = DEF ? train_row_default<SI>(a, wl, xr, b.xs, yt, b.gscale, b.fwd_only, lds + tid, RTP)
                    : train_row_generic(a, w, xr, b.xs, yt, b.gscale, b.fwd_only, lds + tid, RTP);
        } else if (tid < rows4 && !b.fwd_only) {
            for (int c = 0; c < a->ones; ++c) lds[c * RTP + tid] = 0.f;      // the last tile's rows past the batch
        }
        if (tid < TR_ROWS) {                     // the waves that hold rows: a fixed tree per wave, then the waves in order
            const double s = wave_sum(tid < rows ? (double)e * (double)e : 0.0);
            if ((tid & 63) == 0) wsum[tid >> 6] = s;
        }
        __syncthreads();
        if (tid == 0) loss += wsum[0] + wsum[1];
        if (!b.fwd_only) train_phase_b(a, lds, rows4, part + (size_t)blockIdx.x * a->P, first);
        first = false;
    }
    if (tid == 0) part_loss[blockIdx.x] = loss;
}

// gradient = the partial sums in a fixed order; Adam (torch.optim.Adam's defaults, its operation order); the loss partials
__global__ __launch_bounds__(TR_UPD) void k_ann_update(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                       float *__restrict__ v, const float *__restrict__ part,
                                                       const double *__restrict__ part_loss, int P, int nparts, int mode,
                                                       AdamArgs ad, double *loss_acc, double n_rows) {
    __shared__ float red[TR_SLICES][64];
    __shared__ double wl[4];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    if (mode & UPD_REDUCE) {
        float sum = 0.f;
        const int lo = slice * nparts / TR_SLICES, hi = (slice + 1) * nparts / TR_SLICES;
        if (i < P) {
#pragma unroll 16
            for (int b = lo; b < hi; ++b) sum += part[(size_t)b * P + i];
        }
        red[slice][lane] = sum;
        __syncthreads();
    }
    if (slice == 0 && i < P && (mode & (UPD_REDUCE | UPD_ADAM))) {
        float gg;
        if (mode & UPD_REDUCE) {
            gg = red[0][lane];
#pragma unroll
            for (int k = 1; k < TR_SLICES; ++k) gg += red[k][lane];
            g[i] = gg;
        } else {
            gg = g[i];
        }
        if (mode & UPD_ADAM) {
            float mm = m[i], vv = v[i];
            mm = fmaf(ad.w1, gg - mm, mm);                       // exp_avg.lerp_(grad, 1 - beta1)
            vv = fmaf(ad.c2 * gg, gg, vv * ad.b2);               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
            const float denom = sqrtf(vv) / ad.bc2s + ad.eps;
            p[i] = fmaf(-ad.step, mm / denom, p[i]);             // param.addcdiv_(exp_avg, denom, value = -lr / bc1)
            m[i] = mm;
            v[i] = vv;
        }
    }
    if ((mode & UPD_LOSS) && loss_acc && blockIdx.x == 0) {      // (uniform over the workgroup)
        if (threadIdx.x < TR_MAX_PARTS) {                        // one partial per thread, a fixed tree per wave, the waves in order
            const double s = wave_sum((int)threadIdx.x < nparts ? part_loss[threadIdx.x] : 0.0);
            if (lane == 0) wl[slice] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            loss_acc[0] += (wl[0] + wl[1]) + (wl[2] + wl[3]);
            loss_acc[1] += n_rows;
        }
    }
}

__global__ __launch_bounds__(256) void k_ann_rows(const float *__restrict__ img, float *__restrict__ rows, int64_t n_img, int N,
                                                  int s, int step, int nc, int64_t total) {
    const int F = s * s, h = s / 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / F;
        const int f = (int)(e - row * F);
        const int64_t cell = row / n_img, im = row - cell * n_img;
        const int cj = (int)(cell / nc), ci = (int)(cell - (int64_t)cj * nc);
        int gy = (cj * step + f / s - h) % N, gx = (ci * step + f % s - h) % N;
        gy += gy < 0 ? N : 0;
        gx += gx < 0 ? N : 0;
        rows[e] = img[(im * N + gy) * N + gx];
    }
}

static int train_batch_check(const char *who, const qgx_ann_trainer *t, const float *x, const float *y, int64_t n, float xs,
                             float ys) {
    QGX_REQUIRE(t && x && y, "%s: null argument", who);
    QGX_REQUIRE(n >= 1, "%s: n = %lld rows (>= 1)", who, (long long)n);
    QGX_REQUIRE(std::isfinite(xs) && xs > 0.f && std::isfinite(ys) && ys > 0.f, "%s: x_scale %g, y_scale %g (finite, > 0)", who,
                (double)xs, (double)ys);
    return QGX_OK;
}

static int train_lr_check(const char *who, double lr) {
    QGX_REQUIRE(std::isfinite(lr) && lr >= 0.0, "%s: lr = %g (finite, >= 0)", who, lr);
    return QGX_OK;
}

static int train_nparts(const qgx_ann_trainer *t, int64_t n, int64_t *tiles) {
    *tiles = (n + t->RT - 1) / t->RT;
    return *tiles < TR_MAX_PARTS ? (int)*tiles : TR_MAX_PARTS;
}

static int train_launch_grad(qgx_ann_trainer *t, const float *x, const float *y, const int64_t *idx, int64_t n, float xs, float ys,
                             int fwd_only, hipStream_t st, int *nparts) {
    BatchArgs b;
    b.x = x; b.y = y; b.idx = idx; b.n = n;
    *nparts = train_nparts(t, n, &b.tiles);
    b.xs = xs; b.ys = ys; b.gscale = (float)(2.0 / (double)n); b.fwd_only = fwd_only;
    const TrainArgs *a = (const TrainArgs *)t->args_dev;
    const dim3 grid((unsigned)*nparts), block(TR_THREADS);
    if (t->dflt && t->si) hipLaunchKernelGGL((k_ann_grad<true, true>), grid, block, 0, st, a, t->vec[0], b, t->part, t->part_loss);
    else if (t->dflt) hipLaunchKernelGGL((k_ann_grad<true, false>), grid, block, 0, st, a, t->vec[0], b, t->part, t->part_loss);
    else hipLaunchKernelGGL((k_ann_grad<false, false>), grid, block, 0, st, a, t->vec[0], b, t->part, t->part_loss);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

static int train_launch_update(qgx_ann_trainer *t, int nparts, int mode, double lr, double *loss_acc, int64_t n, hipStream_t st) {
    AdamArgs ad = {};
    if (mode & UPD_ADAM) {
        const double beta1 = 0.9, beta2 = 0.999;
        const double k = (double)(t->steps + 1);
        const double bc1 = 1.0 - std::pow(beta1, k), bc2 = 1.0 - std::pow(beta2, k);
        ad.w1 = (float)(1.0 - beta1); ad.b2 = (float)beta2; ad.c2 = (float)(1.0 - beta2);
        ad.bc2s = (float)std::sqrt(bc2); ad.eps = 1e-8f; ad.step = (float)(lr / bc1);
    }
    const int blocks = (mode & (UPD_REDUCE | UPD_ADAM)) ? (t->P + 63) / 64 : 1;
    hipLaunchKernelGGL(k_ann_update, dim3((unsigned)blocks), dim3(TR_UPD), 0, st, t->vec[0], t->vec[1], t->vec[2], t->vec[3], t->part,
                       t->part_loss, t->P, nparts, mode, ad, loss_acc, (double)n);
    QGX_HIP(hipGetLastError());
    if (mode & UPD_ADAM) ++t->steps;
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

extern "C" int qgx_ann_rows(const float *img_dev, int64_t n_img, int N, int s, int step, float *rows_dev, void *stream) {
    QGX_REQUIRE(img_dev && rows_dev, "qgx_ann_rows: null argument");
    QGX_REQUIRE(n_img >= 1 && N >= 1, "qgx_ann_rows: n_img = %lld, N = %d (>= 1)", (long long)n_img, N);
    QGX_REQUIRE(s >= 1 && s <= 7 && (s & 1), "qgx_ann_rows: stencil size %d (odd, 1 ... 7)", s);
    QGX_REQUIRE(step >= 1, "qgx_ann_rows: step = %d (>= 1)", step);
    const int nc = (N + step - 1) / step;
    const int64_t total = (int64_t)nc * nc * n_img * s * s;
    int64_t blocks = (total + 255) / 256;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    hipLaunchKernelGGL(k_ann_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img_dev, rows_dev, n_img, N, s, step,
                       nc, total);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

extern "C" int qgx_ann_trainer_destroy(qgx_ann_trainer *t) {
    if (!t) return QGX_OK;
    (void)hipSetDevice(t->device);
    for (float *p : t->vec)
        if (p) (void)hipFree(p);
    if (t->part) (void)hipFree(t->part);
    if (t->part_loss) (void)hipFree(t->part_loss);
    if (t->args_dev) (void)hipFree(t->args_dev);
    delete t;
    return QGX_OK;
}

extern "C" int qgx_ann_trainer_create(const qgx_ann_weights *init, int device, qgx_ann_trainer **out) {
    QGX_REQUIRE(init && out, "qgx_ann_trainer_create: null argument");
    if (int rc = ann_check(init)) return rc;             // every shape before the device is touched
    QGX_REQUIRE(device >= 0, "qgx_ann_trainer_create: device %d", device);
    TrainArgs a = {};
    a.s = init->stencil_size; a.nl = init->n_hidden + 1; a.si = init->scale_invariant ? 1 : 0;
    a.width[0] = a.s * a.s;
    for (int l = 0; l < init->n_hidden; ++l) a.width[l + 1] = init->hidden[l];
    a.width[a.nl] = 1;
    std::vector<float> host;
    int col = 0;
    for (int l = 0; l < a.nl; ++l) {
        const size_t nw = (size_t)a.width[l + 1] * a.width[l];
        a.off_w[l] = (int)host.size();
        host.insert(host.end(), init->w[l], init->w[l] + nw);
        a.off_b[l] = (int)host.size();
        host.insert(host.end(), init->b[l], init->b[l] + a.width[l + 1]);
        a.act[l] = col;
        col += a.width[l];
    }
    for (int l = 0; l < a.nl; ++l) { a.del[l] = col; col += a.width[l + 1]; }
    a.ones = col++;
    a.item0[0] = 0;
    for (int l = 0; l < a.nl; ++l) a.item0[l + 1] = a.item0[l] + a.width[l + 1] * ((a.width[l] + 4) / 4);
    a.RT = ((TR_LDS / col) & ~3) - TR_PAD;               // a multiple of four; a column holds RT + TR_PAD floats
    if (a.RT > TR_ROWS) a.RT = TR_ROWS;
    a.P = (int)host.size();
    QGX_REQUIRE(a.RT >= 4, "qgx_ann_trainer_create: the net's %d columns do not fit a tile", col);

    qgx_ann_trainer *t = new (std::nothrow) qgx_ann_trainer();
    if (!t) { set_error("out of host memory"); return QGX_ERR_NOMEM; }
    t->device = device; t->P = a.P; t->RT = a.RT; t->si = a.si != 0; t->F = a.width[0];
    t->dflt = a.s == 3 && a.nl == 3 && a.width[1] == 24 && a.width[2] == 24;
    const size_t bytes = (size_t)a.P * sizeof(float);
    hipError_t e = hipSetDevice(device);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) {
        e = hipMalloc((void **)&t->vec[k], bytes);
        if (e == hipSuccess) e = k == 0 ? hipMemcpy(t->vec[0], host.data(), bytes, hipMemcpyHostToDevice) : hipMemset(t->vec[k], 0, bytes);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&t->part, bytes * TR_MAX_PARTS);
    if (e == hipSuccess) e = hipMalloc((void **)&t->part_loss, sizeof(double) * TR_MAX_PARTS);
    if (e == hipSuccess) e = hipMalloc(&t->args_dev, sizeof(TrainArgs));
    if (e == hipSuccess) e = hipMemcpy(t->args_dev, &a, sizeof(TrainArgs), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("qgx_ann_trainer_create: %s", hipGetErrorString(e));
        qgx_ann_trainer_destroy(t);
        return QGX_ERR_HIP;
    }
    *out = t;
    return QGX_OK;
}

extern "C" int64_t qgx_ann_trainer_size(const qgx_ann_trainer *t) { return t ? t->P : -1; }

extern "C" int qgx_ann_trainer_grad(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                                    int64_t n, float x_scale, float y_scale, double *loss_acc_dev, void *stream) {
    if (int rc = train_batch_check("qgx_ann_trainer_grad", t, x_rows_dev, y_rows_dev, n, x_scale, y_scale)) return rc;
    QGX_REQUIRE(idx_dev, "qgx_ann_trainer_grad: null idx_dev");
    int nparts = 0;
    if (int rc = train_launch_grad(t, x_rows_dev, y_rows_dev, idx_dev, n, x_scale, y_scale, 0, (hipStream_t)stream, &nparts)) return rc;
    return train_launch_update(t, nparts, UPD_REDUCE | UPD_LOSS, 0.0, loss_acc_dev, n, (hipStream_t)stream);
}

extern "C" int qgx_ann_trainer_adam(qgx_ann_trainer *t, double lr, void *stream) {
    QGX_REQUIRE(t, "qgx_ann_trainer_adam: null handle");
    if (int rc = train_lr_check("qgx_ann_trainer_adam", lr)) return rc;
    return train_launch_update(t, 0, UPD_ADAM, lr, nullptr, 0, (hipStream_t)stream);
}

extern "C" int qgx_ann_trainer_step(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                                    int64_t n, float x_scale, float y_scale, double lr, double *loss_acc_dev, void *stream) {
    if (int rc = train_batch_check("qgx_ann_trainer_step", t, x_rows_dev, y_rows_dev, n, x_scale, y_scale)) return rc;
    QGX_REQUIRE(idx_dev, "qgx_ann_trainer_step: null idx_dev");
    if (int rc = train_lr_check("qgx_ann_trainer_step", lr)) return rc;
    int nparts = 0;
    if (int rc = train_launch_grad(t, x_rows_dev, y_rows_dev, idx_dev, n, x_scale, y_scale, 0, (hipStream_t)stream, &nparts)) return rc;
    return train_launch_update(t, nparts, UPD_REDUCE | UPD_ADAM | UPD_LOSS, lr, loss_acc_dev, n, (hipStream_t)stream);
}

extern "C" int qgx_ann_trainer_loss(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                                    int64_t n, float x_scale, float y_scale, double *loss_acc_dev, void *stream) {
    if (int rc = train_batch_check("qgx_ann_trainer_loss", t, x_rows_dev, y_rows_dev, n, x_scale, y_scale)) return rc;
    QGX_REQUIRE(loss_acc_dev, "qgx_ann_trainer_loss: null loss_acc_dev");
    int nparts = 0;
    if (int rc = train_launch_grad(t, x_rows_dev, y_rows_dev, idx_dev, n, x_scale, y_scale, 1, (hipStream_t)stream, &nparts)) return rc;
    return train_launch_update(t, nparts, UPD_LOSS, 0.0, loss_acc_dev, n, (hipStream_t)stream);
}

extern "C" int qgx_ann_trainer_read(qgx_ann_trainer *t, int what, float *host) {
    QGX_REQUIRE(t && host, "qgx_ann_trainer_read: null argument");
    QGX_REQUIRE(what >= 0 && what <= 3, "qgx_ann_trainer_read: what = %d (0 ... 3)", what);
    QGX_HIP(hipSetDevice(t->device));
    QGX_HIP(hipDeviceSynchronize());
    QGX_HIP(hipMemcpy(host, t->vec[what], (size_t)t->P * sizeof(float), hipMemcpyDeviceToHost));
    return QGX_OK;
}

extern "C" int qgx_ann_trainer_write(qgx_ann_trainer *t, int what, const float *host, int64_t adam_steps) {
    QGX_REQUIRE(t && host, "qgx_ann_trainer_write: null argument");
    QGX_REQUIRE(what >= 0 && what <= 3, "qgx_ann_trainer_write: what = %d (0 ... 3)", what);
    QGX_HIP(hipSetDevice(t->device));
    QGX_HIP(hipDeviceSynchronize());
    QGX_HIP(hipMemcpy(t->vec[what], host, (size_t)t->P * sizeof(float), hipMemcpyHostToDevice));
    QGX_HIP(hipDeviceSynchronize());
    if (adam_steps >= 0) t->steps = adam_steps;
    return QGX_OK;
}
