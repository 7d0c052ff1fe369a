// The latent step of a conditional VAE's training (include/qgx_latent_train.h), between the encoder's last convolution and
// the decoder's first.  Every kernel gives one lane FOUR consecutive pixels of an image row — a "quad": its two planar
// channels are one 16-byte access each, coalesced along x (a wave reads 1 KiB of a plane per instruction), its four records
// are four 16-byte accesses each way, and the eight normals of its two channels are exactly two Philox quads, so no draw is
// thrown away (every admitted N is a multiple of 4, so a quad straddles neither a row nor a channel).  These kernels move
// about 70 bytes per pixel and are bound by their launch, not by bandwidth: what they buy is ONE launch where torch runs a
// slice, an exp, a square, a randn, a multiply-add, a concatenation and four reductions (and autograd the backward of
// each), no read of a loss back to the host within a step, and no eps kept from the forward to the backward.
//
//   k_latent_forward    block blk takes the quads [blk qpb, (blk + 1) qpb): a thread its quads q0 + t, q0 + t + 256, ... in
//                       order; dec_in = [x, eps std + mu, 0 ...]; the four sums (KL terms, var, mu, mu^2) in float64 from
//                       the first add, the 64 lanes by a shuffle tree in registers, the four waves in order through LDS;
//                       four float64 per block into the workspace
//   k_latent_finish     one block adds the partials in a fixed order and forms the three statistics
//   k_latent_backward   d_enc = [dz + s mu, 0.5 dz eps std + 0.5 s (var - 1), 0 ...], s read from the device as float64 and
//                       rounded once
// The pixel-record access, the block sum and the shape of the partition restate those of train_head.hip for quads.
#include "common.hpp"
#include "philox.hpp"

namespace qgx {

constexpr int LATENT_BLOCK = 256;
constexpr int LATENT_MAX_PARTIALS = 256;      // 256 blocks x 256 lanes x 4 pixels: above 2^18 pixels a lane takes several quads
constexpr int LATENT_SUMS = 4;                // KL terms, var, mu, mu^2

struct Quad {
    int b;           // batch member
    int r;           // offset of the quad's first pixel in its image plane (a multiple of 4)
};
__device__ __forceinline__ Quad quad_of(int q, int NN) {
    const int p = q * 4;
    Quad u;
    u.b = p / NN;
    u.r = p - u.b * NN;
    return u;
}
__device__ __forceinline__ float4 load4(const float *base, size_t off) { return *reinterpret_cast<const float4 *>(base + off); }
__device__ __forceinline__ void get4(const float4 &a, float (&v)[4]) { v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }

// eps of the quad's four pixels, both channels: read from the planar eps (B, 2, N, N), or drawn
__device__ __forceinline__ void quad_eps(const float *eps, uint64_t seed, uint64_t step, const Quad &u, int NN, float (&e)[2][4]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (eps)
            get4(load4(eps, ((size_t)u.b * 2 + c) * NN + u.r), e[c]);
        else
            philox_normal4(seed, (uint64_t)u.b, step, (uint32_t)((c * NN + u.r) >> 2), e[c]);
    }
}
// channels 0 ... 3 of the record of pixel p
__device__ __forceinline__ float4 record_head(const float *a, int p) { return reinterpret_cast<const float4 *>(a)[(size_t)p * 2]; }
__device__ __forceinline__ void store_record(float *out, int p, float4 head) {
    float4 *rec = reinterpret_cast<float4 *>(out) + (size_t)p * 2;
    rec[0] = head;
    rec[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the sums of v[0 ... 3] over the block's 256 threads, valid in thread 0: lanes by a fixed shuffle tree, waves in order
__device__ __forceinline__ void block_sums(double (&v)[LATENT_SUMS], double (*red)[LATENT_BLOCK / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < LATENT_SUMS; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_down(v[k], off);
        if (lane == 0) red[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LATENT_SUMS; ++k) {
        double s = red[k][0];
#pragma unroll
        for (int w = 1; w < LATENT_BLOCK / 64; ++w) s += red[k][w];
        v[k] = s;
    }
}

__global__ __launch_bounds__(LATENT_BLOCK) void k_latent_forward(const float *enc, const float *x, const int64_t *idx, const float *eps,
                                                                 uint64_t seed, uint64_t step, float *dec_in, double *part, int NN,
                                                                 int nq, int qpb) {
    __shared__ double red[LATENT_SUMS][LATENT_BLOCK / 64];
    const int q0 = blockIdx.x * qpb, q1 = q0 + qpb < nq ? q0 + qpb : nq;
    double acc[LATENT_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int q = q0 + threadIdx.x; q < q1; q += LATENT_BLOCK) {
        const Quad u = quad_of(q, NN);
        const int64_t row = idx ? idx[u.b] : (int64_t)u.b;
        float xs[2][4], e[2][4];
        get4(load4(x, ((size_t)row * 2 + 0) * NN + u.r), xs[0]);
        get4(load4(x, ((size_t)row * 2 + 1) * NN + u.r), xs[1]);
        quad_eps(eps, seed, step, u, NN, e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = q * 4 + j;
            float m[4] = {0.f, 0.f, 0.f, 0.f};          // mu1, mu2, logvar1, logvar2: the prior without enc
            if (enc) get4(record_head(enc, p), m);
            float z[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float mu = m[c], lv = m[2 + c];
                const float sd = expf(0.5f * lv);
                const float var = sd * sd;
                z[c] = e[c][j] * sd + mu;
                acc[0] += (double)(0.5f * (mu * mu + var - 1.f - lv));
                acc[1] += (double)var;
                acc[2] += (double)mu;
                acc[3] += (double)mu * (double)mu;
            }
            store_record(dec_in, p, make_float4(xs[0][j], xs[1][j], z[0], z[1]));
        }
    }
    if (!part) return;                                   // the prior: no statistics (uniform over the grid)
    block_sums(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < LATENT_SUMS; ++k) part[(size_t)blockIdx.x * LATENT_SUMS + k] = acc[k];
    }
}

__global__ __launch_bounds__(LATENT_BLOCK) void k_latent_finish(const double *part, double *stats, int nb, double B, double count) {
    __shared__ double red[LATENT_SUMS][LATENT_BLOCK / 64];
    double acc[LATENT_SUMS] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nb; k += LATENT_BLOCK) {
#pragma unroll
        for (int s = 0; s < LATENT_SUMS; ++s) acc[s] += part[(size_t)k * LATENT_SUMS + s];
    }
    block_sums(acc, red);
    if (threadIdx.x == 0) {
        const double var_latent = acc[1] / count;
        stats[0] = acc[0] / B;
        stats[1] = var_latent;
        stats[2] = (acc[3] - acc[2] * acc[2] / count) / (count - 1.0) + var_latent;
    }
}

__global__ __launch_bounds__(LATENT_BLOCK) void k_latent_backward(const float *enc, const float *eps, uint64_t seed, uint64_t step,
                                                                  const float *d_dec_in, const double *gout, float *d_enc, int NN,
                                                                  int nq, double B) {
    const int q = blockIdx.x * LATENT_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const float s = (float)(*gout / B);
    const Quad u = quad_of(q, NN);
    float e[2][4];
    quad_eps(eps, seed, step, u, NN, e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = q * 4 + j;
        float m[4], d[4], g[4];
        get4(record_head(enc, p), m);
        get4(record_head(d_dec_in, p), d);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float mu = m[c], lv = m[2 + c], dz = d[2 + c];
            const float sd = expf(0.5f * lv);
            const float var = sd * sd;
            g[c] = dz + s * mu;
            g[2 + c] = 0.5f * dz * e[c][j] * sd + 0.5f * s * (var - 1.f);
        }
        store_record(d_enc, p, make_float4(g[0], g[1], g[2], g[3]));
    }
}

// ---- host side -------------------------------------------------------------------------------
// The partition of the sums, a function of (B, N) alone: at most LATENT_MAX_PARTIALS ranges of qpb quads, qpb a multiple of the block
struct LatentPlan { int nq, nb, qpb; };
static LatentPlan latent_plan(int64_t B, int N) {
    const int64_t nq = B * N * N / 4;
    int64_t nb = (nq + LATENT_BLOCK - 1) / LATENT_BLOCK;
    if (nb > LATENT_MAX_PARTIALS) nb = LATENT_MAX_PARTIALS;
    const int64_t qpb = ((nq + nb - 1) / nb + LATENT_BLOCK - 1) / LATENT_BLOCK * LATENT_BLOCK;
    LatentPlan p;
    p.nq = (int)nq;
    p.qpb = (int)qpb;
    p.nb = (int)((nq + qpb - 1) / qpb);
    return p;
}
static size_t latent_work_bytes(int64_t B, int N) {
    return ((size_t)latent_plan(B, N).nb * LATENT_SUMS * sizeof(double) + 255) / 256 * 256;
}

static int latent_grid_check(const char *what, int64_t B, int N) {
    QGX_REQUIRE(N == 16 || N == 32 || N == 48 || N == 64 || N == 96 || N == 128, "%s: N = %d, expected 16, 32, 48, 64, 96 or 128", what, N);
    QGX_REQUIRE(B >= 1 && B <= ((int64_t)1 << 29) / (N * N), "%s: B = %lld, expected 1 ... 2^29 / N^2", what, (long long)B);
    return QGX_OK;
}
static bool latent_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define LATENT_PTR(what, p)                                                                                \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(latent_aligned16(p), "%s: " #p " is not 16-byte aligned", what);                       \
    } while (0)
#define LATENT_OPTIONAL_PTR(what, p) QGX_REQUIRE(latent_aligned16(p), "%s: " #p " is not 16-byte aligned", what)

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_latent_workspace(int64_t B, int N, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_latent_workspace: bytes is NULL");
    if (const int rc = latent_grid_check("qgx_latent_workspace", B, N)) return rc;
    *bytes = latent_work_bytes(B, N);
    return QGX_OK;
}

int qgx_latent_forward(const float *enc_dev, const float *x_dev, const int64_t *idx_dev, const float *eps_dev, uint64_t seed,
                       uint64_t step, float *dec_in_dev, double *stats_dev, int64_t B, int N, int64_t n, void *work_dev,
                       size_t work_bytes, void *stream) {
    const char *what = "qgx_latent_forward";
    if (const int rc = latent_grid_check(what, B, N)) return rc;
    QGX_REQUIRE(n >= 1, "%s: n = %lld, expected >= 1", what, (long long)n);
    QGX_REQUIRE(idx_dev || n >= B, "%s: n = %lld rows for B = %lld without idx_dev", what, (long long)n, (long long)B);
    LATENT_OPTIONAL_PTR(what, enc_dev); LATENT_PTR(what, x_dev); LATENT_OPTIONAL_PTR(what, idx_dev); LATENT_OPTIONAL_PTR(what, eps_dev);
    LATENT_PTR(what, dec_in_dev);
    if (enc_dev) {
        LATENT_PTR(what, stats_dev); LATENT_PTR(what, work_dev);
        const size_t need = latent_work_bytes(B, N);
        QGX_REQUIRE(work_bytes >= need, "%s: work_bytes = %zu, qgx_latent_workspace gives %zu", what, work_bytes, need);
    }
    hipStream_t st = (hipStream_t)stream;
    const LatentPlan p = latent_plan(B, N);
    double *part = enc_dev ? (double *)work_dev : nullptr;
    hipLaunchKernelGGL(k_latent_forward, dim3(p.nb), dim3(LATENT_BLOCK), 0, st, enc_dev, x_dev, idx_dev, eps_dev, seed, step, dec_in_dev,
                       part, N * N, p.nq, p.qpb);
    QGX_HIP(hipGetLastError());
    if (enc_dev) {
        hipLaunchKernelGGL(k_latent_finish, dim3(1), dim3(LATENT_BLOCK), 0, st, (const double *)part, stats_dev, p.nb, (double)B,
                           (double)(2 * B * N * N));
        QGX_HIP(hipGetLastError());
    }
    return QGX_OK;
}

int qgx_latent_backward(const float *enc_dev, const float *eps_dev, uint64_t seed, uint64_t step, const float *d_dec_in_dev,
                        const double *gout_kl_dev, float *d_enc_dev, int64_t B, int N, void *stream) {
    const char *what = "qgx_latent_backward";
    if (const int rc = latent_grid_check(what, B, N)) return rc;
    LATENT_PTR(what, enc_dev); LATENT_OPTIONAL_PTR(what, eps_dev); LATENT_PTR(what, d_dec_in_dev); LATENT_PTR(what, gout_kl_dev);
    LATENT_PTR(what, d_enc_dev);
    const int NN = N * N, nq = (int)(B * NN / 4);
    hipLaunchKernelGGL(k_latent_backward, dim3((nq + LATENT_BLOCK - 1) / LATENT_BLOCK), dim3(LATENT_BLOCK), 0, (hipStream_t)stream,
                       enc_dev, eps_dev, seed, step, d_dec_in_dev, gout_kl_dev, d_enc_dev, NN, nq, (double)B);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // extern "C"
