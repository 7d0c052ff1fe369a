// The generator handle: lifecycle and workspaces, the model-independent kernels around a net (network input from q and the
// latent noise, output scaling + de-mean, range words, Monte-Carlo moments), generator_forward with its dispatch over the
// model kinds, generator_forward_mean (deterministic sampling: the mean of M realisations per member), and the C ABI that is not AndrewCNN-specific.
//
// Replaces the model wrappers models/cgan_regression.py:157-162, cvae_regression.py:131-136, mean_var_model.py:105-109,
// ols_model.py:68-75, ann_model.py:82-93 and the per-layer de-mean of models/parameterization.py:25.  The nets themselves
// are three back ends behind narrow interfaces: the AndrewCNN (conv.hip, through generator.hpp), the DeepInversion U-Net
// (unet.hip) and the pointwise stencil ANN (ann.hip).
#include "generator.hpp"
#include "philox.hpp"
#include <algorithm>
#include <new>

namespace qgx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- small pointwise kernels around the CNN ---------------------------------------------
// X = [float(q)/x_std, z]  (cgan_regression.py:158 + generate :133-137)
// largest |x| of the network input, for the f16x3 range guard: a NaN counts as infinity; non-negative floats
// order like their bit patterns, so one atomicMax on the bits per wave keeps the running maximum
__device__ __forceinline__ void input_absmax(float m, unsigned *range) {
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
    // the running maximum settles after the first launches: read it, and only a new record costs an atomic
    if ((threadIdx.x & 63) == 0 && __float_as_uint(m) > __builtin_nontemporal_load(range + 1)) atomicMax(range + 1, __float_as_uint(m));
}

__global__ void k_prep_input(const double *q, const float *z, float *X, int n_in, int npix, float xs0, float xs1,
                             unsigned *range) {
    const int b = blockIdx.y;
    float m = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
        const size_t qo = (size_t)b * 2 * npix + i;
        float *x = X + (size_t)b * n_in * npix + i;
        const float x0 = (float)q[qo] / xs0, x1 = (float)q[qo + npix] / xs1;
        x[0] = x0;
        x[npix] = x1;
        m = fmaxf(m, fmaxf(abs_or_inf(x0), abs_or_inf(x1)));
        if (n_in == 4) {
            const float z0 = z[qo], z1 = z[qo + npix];
            x[2 * (size_t)npix] = z0;
            x[3 * (size_t)npix] = z1;
            m = fmaxf(m, fmaxf(abs_or_inf(z0), abs_or_inf(z1)));
        }
    }
    input_absmax(m, range);
}

// the normalised PV of every member (channels 0, 1 of the generator's 4-channel input) as the 2-channel input of the
// regression net (cgan_regression.py:159-161: apply_function(self.net_mean, X) on the same X)
__global__ void k_take2(const float *X, float *X2, int npix2) {      // npix2 = 2 npix, a multiple of 4
    const int b = blockIdx.y;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(X + (size_t)b * 2 * npix2);
    f32x4 *dst = reinterpret_cast<f32x4 *>(X2 + (size_t)b * npix2);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix2 / 4; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

__global__ void k_absmax(const float *x, size_t n, unsigned *range) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = fmaxf(m, abs_or_inf(x[i]));
    input_absmax(m, range);
}

// Fused sampler update + input assembly of one online step (GAN / VAE):
//   z <- a z + b xi  (float; xi from Philox or the external draw), X = [float(q)/x_std, z]
// One thread per quad of 4 consecutive elements of the (2,N,N) member field.
__global__ void k_prep_noise(const double *q, float *z, const float *xi_ext, float *X, int npix, float xs0,
                             float xs1, uint64_t seed, uint64_t member_offset, uint64_t step, float a, float b,
                             unsigned *range) {
    const int member = blockIdx.y;
    const int quads = 2 * npix / 4;
    const int quad = blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.f;
    if (quad < quads) {
        const size_t o = (size_t)member * 2 * npix + 4 * (size_t)quad;
        float x[4];
        if (xi_ext) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = xi_ext[o + e];
        } else {
            philox_normal4(seed, member_offset + member, step, (uint32_t)quad, x);
        }
        float *Xm = X + (size_t)member * 4 * npix;
        const int i = 4 * quad;                          // flat index in (2, npix); npix % 4 == 0
        const float xs = i < npix ? xs0 : xs1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float zn = a == 0.f ? b * x[e] : a * z[o + e] + b * x[e];
            z[o + e] = zn;
            Xm[2 * (size_t)npix + i + e] = zn;
            const float xq = (float)q[o + e] / xs;
            Xm[i + e] = xq;
            m = fmaxf(m, fmaxf(abs_or_inf(zn), abs_or_inf(xq)));
        }
    }
    input_absmax(m, range);
}

// Deterministic sampling, input assembly of one chunk of R realisations (first_real .. first_real + R - 1) of every member:
//   X[p] = [float(q_b)/x_std, xi],  p = b R + r,  xi = Philox(seed, member, step + ((first_real + r + 1) << 32))
// One thread per quad of the (2,N,N) member field; the q channels are converted once per thread and stored for every
// realisation the thread writes (r = blockIdx.z, blockIdx.z + gridDim.z, ...); the draw goes straight into X, there is no z.
__global__ void k_prep_mean(const double *q, float *X, int npix, int R, int first_real, float xs0, float xs1, uint64_t seed,
                            uint64_t member_offset, uint64_t step, unsigned *range) {
    const int member = blockIdx.y;
    const int quads = 2 * npix / 4;
    const int quad = blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.f;
    if (quad < quads) {
        const size_t o = (size_t)member * 2 * npix + 4 * (size_t)quad;
        const int i = 4 * quad;                          // flat index in (2, npix); npix % 4 == 0
        const float xs = i < npix ? xs0 : xs1;
        f32x4 xq;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xq[e] = (float)q[o + e] / xs;
            m = fmaxf(m, abs_or_inf(xq[e]));
        }
        for (int r = blockIdx.z; r < R; r += gridDim.z) {
            float x[4];
            philox_normal4(seed, member_offset + member, step + ((uint64_t)(first_real + r + 1) << 32), (uint32_t)quad, x);
            float *Xp = X + ((size_t)member * R + r) * 4 * npix;
            *reinterpret_cast<f32x4 *>(Xp + i) = xq;
            f32x4 xi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xi[e] = x[e];
                m = fmaxf(m, abs_or_inf(x[e]));
            }
            *reinterpret_cast<f32x4 *>(Xp + 2 * (size_t)npix + i) = xi;
        }
    }
    input_absmax(m, range);
}

// ... and the sum over them: acc (B,2,N,N) float64 <- [acc +] the chunk's R outputs y (B R, 2, N, N) in realisation order
// (first: the first chunk overwrites, no memset); after the last chunk mean (B,2,N,N) <- float(acc / M)
// (predict_mean_snapshot: .mean(0) — here in float64, rounded once).  One thread per 4 elements, no atomics: bitwise repeatable.
__global__ void k_mean_accumulate(const float *y, double *acc, float *mean, int n4_member, int B, int R, int first, int last,
                                  double M) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * n4_member) return;
    const size_t b = idx / n4_member, i4 = idx % n4_member;
    f64x2 *a = reinterpret_cast<f64x2 *>(acc) + 2 * idx;
    f64x2 lo = {0.0, 0.0}, hi = {0.0, 0.0};
    if (!first) { lo = a[0]; hi = a[1]; }
    const f32x4 *src = reinterpret_cast<const f32x4 *>(y) + b * R * n4_member + i4;
    for (int r = 0; r < R; ++r) {
        const f32x4 v = src[(size_t)r * n4_member];
        lo[0] += (double)v[0]; lo[1] += (double)v[1];
        hi[0] += (double)v[2]; hi[1] += (double)v[3];
    }
    if (last) {
        const f32x4 mu = {(float)(lo[0] / M), (float)(lo[1] / M), (float)(hi[0] / M), (float)(hi[1] / M)};
        reinterpret_cast<f32x4 *>(mean)[idx] = mu;
    } else {
        a[0] = lo; a[1] = hi;
    }
}

// Fused output scaling + per-layer de-mean: one workgroup per (member, layer).
//   GAN/VAE: S = double(y * y_std)                         (cgan_regression.py:162)
//   GZ:      S = (mean + z sqrt(softplus(var))) * y_std    (mean_var_model.py:14-17,105-109)
//   GAN/VAE with regression != 'None': S = double((y + net_mean(x)) * y_std), the sum in float32
//                                                          (cgan_regression.py:159-162, cvae_regression.py:133-136)
//   then S -= mean_{y,x} S                                 (parameterization.py:25)
enum { FIN_PLAIN = 0, FIN_GZ = 1, FIN_SUM = 2 };
template <int MODE>
__global__ __launch_bounds__(1024) void k_finish(const float *y0, const float *y1, const double *z, double *S, int npix, float ys0,
                                                 float ys1, int demean, unsigned *range) {
    __shared__ double sm[16];
    __shared__ double mean_s;
    const size_t o = (size_t)blockIdx.x * npix;
    const float ys = (blockIdx.x & 1) ? ys1 : ys0;
    auto value = [&](int i) -> double {
        if constexpr (MODE == FIN_GZ) {
            const float vr = y1[o + i];
            const float sp = vr > 20.f ? vr : log1pf(expf(vr));
            return ((double)y0[o + i] + z[o + i] * (double)sqrtf(sp)) * (double)ys;
        } else if constexpr (MODE == FIN_SUM) {
            return (double)((y0[o + i] + y1[o + i]) * ys);
        } else {
            return (double)(y0[o + i] * ys);
        }
    };
    // one workgroup per (member, layer) is a short latency chain: 1024 threads, and the values are read ONCE
    // (kept in registers between the mean and the store for grids up to 128 x 128)
    constexpr int KEEP = 16;
    double keep[KEEP];
    const bool cached = npix <= KEEP * (int)blockDim.x;
    double acc = 0.0;
    if (cached) {
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int i = u * blockDim.x + threadIdx.x;
            keep[u] = i < npix ? value(i) : 0.0;
            acc += keep[u];
        }
    } else if (demean) {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) acc += value(i);
    }
    double mu = 0.0;
    if (demean) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sm[w];
            mean_s = t / (double)npix;
        }
        __syncthreads();
        mu = mean_s;
    }
    if (cached) {
        bool bad = false;
#pragma unroll
        for (int u = 0; u < KEEP; ++u) {
            const int i = u * blockDim.x + threadIdx.x;
            if (i < npix) S[o + i] = keep[u] - mu;
            bad |= !(fabs(keep[u]) <= 1.79e308);
        }
        if (bad) atomicOr(range, 0x80000000u);      // a non-finite forcing never reaches the model unnoticed
    } else {
        bool bad = false;
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const double val = value(i);
            S[o + i] = val - mu;
            bad |= !(fabs(val) <= 1.79e308);
        }
        if (bad) atomicOr(range, 0x80000000u);
    }
}

// running first and second moments over Monte-Carlo samples (generate_mean_var, cgan_regression.py:139-146)
__global__ void k_moments(const float *y, double *sum, double *sumsq, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = (double)y[i];
        sum[i] += v;
        sumsq[i] += v * v;
    }
}
// ---- host side ---------------------------------------------------------------------------
void launch_absmax(const float *x, size_t n, unsigned *range, hipStream_t st) {
    hipLaunchKernelGGL(k_absmax, dim3(256), dim3(256), 0, st, x, n, range);
}

int generator_select_workspace(qgx_generator *g, int idx) {
    QGX_REQUIRE(g && (idx == 0 || idx == 1), "generator_select_workspace: bad argument");
    g->ws_active = idx;
    return QGX_OK;
}

int generator_reserve(qgx_generator *g, int B, int N) {
    Workspace &w = g->work();
    const size_t need = (size_t)B * N * N;
    if (need <= w.cap_elems) return QGX_OK;
    w.free_activations();
    if (g->ann) {        // the ANN kernel reads q and writes its raw output (B, 2, N, N): no activations, no input buffer
        QGX_HIP(hipMalloc((void **)&w.Y0, need * 2 * sizeof(float)));
        w.cap_elems = need;
        return QGX_OK;
    }
    const size_t actA = g->unet ? std::max(need * g->actw[0], unet_workspace_floats(B, N)) : need * g->actw[0];
    QGX_HIP(hipMalloc((void **)&w.actA, actA * sizeof(float)));
    QGX_HIP(hipMalloc((void **)&w.actB, need * g->actw[1] * sizeof(float)));
    QGX_HIP(hipMalloc((void **)&w.X, need * 6 * sizeof(float)));    // (B, 4, N, N), and behind it (B, 2, N, N) for a regression net
    QGX_HIP(hipMalloc((void **)&w.Y0, need * 2 * sizeof(float)));
    QGX_HIP(hipMalloc((void **)&w.Y1, need * 2 * sizeof(float)));
    // a flux-form net (n_out = 4) writes its fluxes (B, 4, N, N) here, and the divergence kernel reads them
    if (g->nets[0].flux() || (g->n_nets == 2 && g->nets[1].flux())) QGX_HIP(hipMalloc((void **)&w.F, need * 4 * sizeof(float)));
    w.cap_elems = need;
    return QGX_OK;
}

int generator_reserve_part(qgx_generator *g, size_t elems) {
    Workspace &w = g->work();
    if (w.part_elems >= elems) return QGX_OK;
    w.free_part();
    QGX_HIP(hipMalloc((void **)&w.part, elems * sizeof(float)));
    w.part_elems = elems;
    return QGX_OK;
}

bool generator_noise_is_double(const qgx_generator *g) { return g->kind == QGX_GEN_GZ; }
bool generator_takes_noise(const qgx_generator *g) { return g->kind != QGX_GEN_OLS && g->kind != QGX_GEN_ANN; }
bool generator_reads_q(const qgx_generator *g) { return g->ann != nullptr; }

int generator_input_info(qgx_generator *g, int B, int N, GenFuse *gf) {
    QGX_REQUIRE(g && gf && g->kind != QGX_GEN_GZ && !g->ann, "generator_input_info: bad argument");
    int rc = generator_reserve(g, B, N);
    if (rc) return rc;
    gf->X = g->work().X; gf->xs[0] = g->x_std[0]; gf->xs[1] = g->x_std[1]; gf->range = g->range_dev;
    // OLS: X = float(q)/x_std alone, (B, 2, N, N) as k_prep_input lays it out with n_in = 2
    gf->xc = g->kind == QGX_GEN_OLS ? 2 : 4;
    gf->no_noise = g->kind == QGX_GEN_OLS;
    return QGX_OK;
}

// net 0 of a GAN / VAE handle: the AndrewCNN generator / decoder, or the U-Net of qgx_generator_create_unet
static int net0_forward(qgx_generator *g, const float *x, float *y, int B, int N, hipStream_t st) {
    if (g->unet) return unet_forward(g->unet, x, y, g->work().actA, B, N, st);
    return cnn_forward(g, g->nets[0], x, y, B, N, st);
}

template <int MODE>
static void launch_finish(qgx_generator *g, const float *y1, const double *z, double *S, int B, int npix, int demean, hipStream_t st) {
    hipLaunchKernelGGL(k_finish<MODE>, dim3(2 * B), dim3(1024), 0, st, (const float *)g->work().Y0, y1, z, S, npix,
                       g->y_std[0], g->y_std[1], demean, g->range_dev);
}
// the tail of every model kind: S from the raw output Y0 (and y1: FIN_SUM the regression net's output, FIN_GZ the variance
// net's, with the latent noise z), or — defer != null — the description of that work for the step kernel (GenFuse::y)
static void finish(qgx_generator *g, GenFuse *defer, int mode, const float *y1, const double *z, double *S, int B, int npix,
                   int demean, hipStream_t st) {
    if (defer) {
        defer->y = g->work().Y0; defer->y1 = y1;
        defer->ys[0] = g->y_std[0]; defer->ys[1] = g->y_std[1]; defer->demean = demean;
        defer->range = g->range_dev;
    } else if (mode == FIN_GZ) launch_finish<FIN_GZ>(g, y1, z, S, B, npix, demean, st);
    else if (mode == FIN_SUM) launch_finish<FIN_SUM>(g, y1, z, S, B, npix, demean, st);
    else launch_finish<FIN_PLAIN>(g, y1, z, S, B, npix, demean, st);
}

// The one grid-size rule of a handle, asked by qgx_generator_forward, qgx_cnn_forward (inet >= 0: that net alone) and
// qgx_step before anything is launched or any sampler state is touched: net 0 of a U-Net handle takes unet_size_ok's grids,
// every AndrewCNN what its launchers take (cnn_size_ok), the ANN every N its own launcher admits (ann.hip, before its launch).
int generator_size_ok(const qgx_generator *g, int B, int N, int inet) {
    QGX_REQUIRE(g && B > 0, "generator: bad argument");
    if (g->ann) return QGX_OK;
    for (int n = 0; n < g->n_nets; ++n) {
        if (inet >= 0 && n != inet) continue;
        if (g->unet && n == 0) {
            QGX_REQUIRE(unet_size_ok(N), "U-Net generator: N = %d is not supported (32, 48, 64, 96 or 128)", N);
            continue;
        }
        QGX_REQUIRE(cnn_size_ok(g, g->nets[n], B, N),
                    "generator: N = %d is not supported by the AndrewCNN kernels (B = %d; with the shipped options 16, 32, 48, 64, 96 or 128)", N, B);
    }
    return QGX_OK;
}

int generator_forward(qgx_generator *g, const double *q, const void *z, double *S, int B, int N,
                      int demean, hipStream_t st, const NoiseUpdate *nu, GenFuse *defer, bool input_ready) {
    QGX_REQUIRE(g && q && (z || !generator_takes_noise(g)) && S && B > 0, "generator_forward: bad argument");
    if (const int src = generator_size_ok(g, B, N)) return src;
    int rc = generator_reserve(g, B, N);
    if (rc) return rc;
    const int npix = N * N;
    QGX_REQUIRE(npix % 4 == 0, "generator_forward: N*N must be a multiple of 4");
    const Workspace &w = g->work();
    dim3 pg((npix + 255) / 256, B), pb(256);
    if (g->ann) {
        // ANNModel.predict_snapshot (ann_model.py:82-93): y = net(stencil(float32(q)) / x_scale) per point of each (member,
        // layer) image, read from q by the kernel itself; S = double(float32(y_scale * y)) is k_finish<FIN_PLAIN> with
        // ys0 = ys1 = y_scale, or the step kernel's prologue (GenFuse::y).  No latent noise, no input to assemble.
        if ((rc = ann_forward_q(g->ann, q, g->x_std[0], w.Y0, 2 * (int64_t)B, N, st))) return rc;
        finish(g, defer, FIN_PLAIN, nullptr, nullptr, S, B, npix, demean, st);
    } else if (g->kind == QGX_GEN_GZ) {
        if (nu && (rc = noise_update(const_cast<void *>(z), nu->xi_ext, true, B, 2 * npix, nu->seed, nu->member_offset,
                                     nu->step, nu->a, nu->b, st))) return rc;
        hipLaunchKernelGGL(k_prep_input, pg, pb, 0, st, q, (const float *)nullptr, w.X, 2, npix, g->x_std[0], g->x_std[1], g->range_dev);
        if ((rc = cnn_forward(g, g->nets[0], w.X, w.Y0, B, N, st))) return rc;
        if ((rc = cnn_forward(g, g->nets[1], w.X, w.Y1, B, N, st))) return rc;
        // (never deferred: the step kernel's prologue has no form of the double-precision noise term)
        finish(g, nullptr, FIN_GZ, w.Y1, (const double *)z, S, B, npix, demean, st);
    } else if (g->kind == QGX_GEN_OLS) {
        // OLSModel.predict_snapshot (ols_model.py:68-75): S = y_std * net(float(q)/x_std); no latent noise, z is never read
        if (!input_ready)      // (else the previous step kernel wrote X: GenFuse::X with xc = 2, no_noise)
            hipLaunchKernelGGL(k_prep_input, pg, pb, 0, st, q, (const float *)nullptr, w.X, 2, npix, g->x_std[0], g->x_std[1], g->range_dev);
        if ((rc = cnn_forward(g, g->nets[0], w.X, w.Y0, B, N, st))) return rc;
        finish(g, defer, FIN_PLAIN, nullptr, nullptr, S, B, npix, demean, st);
    } else {
        if (input_ready) {
            // the previous step kernel wrote X and z (GenFuse::X)
        } else if (nu) {
            dim3 qg((2 * npix / 4 + 255) / 256, B);
            hipLaunchKernelGGL(k_prep_noise, qg, pb, 0, st, q, (float *)const_cast<void *>(z), (const float *)nu->xi_ext,
                               w.X, npix, g->x_std[0], g->x_std[1], nu->seed, nu->member_offset, nu->step,
                               (float)nu->a, (float)nu->b, g->range_dev);
        } else {
            hipLaunchKernelGGL(k_prep_input, pg, pb, 0, st, q, (const float *)z, w.X, 4, npix, g->x_std[0], g->x_std[1], g->range_dev);
        }
        const bool regression = g->n_nets == 2;     // regression != 'None': Y += net_mean(X) on the normalised PV alone
        if (regression) {
            float *X2 = w.X + (size_t)B * 4 * npix;
            hipLaunchKernelGGL(k_take2, dim3((2 * npix / 4 + 255) / 256, B), pb, 0, st, (const float *)w.X, X2, 2 * npix);
            if ((rc = cnn_forward(g, g->nets[1], X2, w.Y1, B, N, st))) return rc;
        }
        if ((rc = net0_forward(g, w.X, w.Y0, B, N, st))) return rc;
        finish(g, defer, regression ? FIN_SUM : FIN_PLAIN, regression ? w.Y1 : nullptr, nullptr, S, B, npix, demean, st);
    }
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

// ---- deterministic sampling: predict_mean_snapshot for every member ------------------------------------------------------
// realisations per launch of net 0: the largest R with B R <= chunk (0: 256, a measured default — DESIGN.md, "Deterministic
// sampling"), at least 1, at most M
static int mean_chunk_R(int B, int M, int chunk) {
    const int cap = chunk > 0 ? chunk : 256;
    return std::max(1, std::min(M, cap / B));
}

int generator_mean_check(const qgx_generator *g, int B, int N, int M, int chunk, uint64_t step) {
    QGX_REQUIRE(g && B > 0, "generator_forward_mean: bad argument");
    QGX_REQUIRE(M >= 1 && M <= 65536, "generator_forward_mean: M = %d realisations (1 ... 65536)", M);
    QGX_REQUIRE(step < (1ull << 32), "generator_forward_mean: step must be below 2^32 (its high word numbers the realisation)");
    QGX_REQUIRE(chunk == 0 || chunk >= B, "generator_forward_mean: chunk = %d is below the member count %d (0 = automatic)", chunk, B);
    QGX_REQUIRE(generator_takes_noise(g),
                "deterministic sampling: the reference defines no predict_mean_snapshot for an OLS or ANN parameterization");
    QGX_REQUIRE(N > 0 && (N * N) % 4 == 0, "generator_forward_mean: N*N must be a multiple of 4");
    if (g->kind == QGX_GEN_GZ) return generator_size_ok(g, B, N, 0);          // the mean net alone
    // net 0 on the pseudo-batches actually launched (full chunks and the remainder), the regression net on the B members
    const int R = mean_chunk_R(B, M, chunk);
    QGX_REQUIRE((int64_t)B * R <= INT32_MAX / 8, "generator_forward_mean: pseudo-batch %d x %d is too large", B, R);
    if (const int rc = generator_size_ok(g, B * R, N, 0)) return rc;
    if (M % R) { if (const int rc = generator_size_ok(g, B * (M % R), N, 0)) return rc; }
    if (g->n_nets == 2) return generator_size_ok(g, B, N, 1);
    return QGX_OK;
}

int generator_forward_mean(qgx_generator *g, const double *q, double *S, int B, int N, int M, int chunk, int demean,
                           uint64_t seed, uint64_t member_offset, uint64_t step, hipStream_t st) {
    QGX_REQUIRE(g && q && S, "generator_forward_mean: null argument");
    if (const int rc = generator_mean_check(g, B, N, M, chunk, step)) return rc;
    const int npix = N * N;
    dim3 pg((npix + 255) / 256, B), pb(256);
    int rc;
    if (g->kind == QGX_GEN_GZ) {
        // mean_var_model.py:111-115: S = y_std * net_mean(q / x_std); no draws, net_var is not evaluated
        if ((rc = generator_reserve(g, B, N))) return rc;
        const Workspace &w = g->work();
        hipLaunchKernelGGL(k_prep_input, pg, pb, 0, st, q, (const float *)nullptr, w.X, 2, npix, g->x_std[0], g->x_std[1], g->range_dev);
        if ((rc = cnn_forward(g, g->nets[0], w.X, w.Y0, B, N, st))) return rc;
        finish(g, nullptr, FIN_PLAIN, nullptr, nullptr, S, B, npix, demean, st);
        QGX_HIP(hipGetLastError());
        return QGX_OK;
    }
    const int R = mean_chunk_R(B, M, chunk);
    if ((rc = generator_reserve(g, B * R, N))) return rc;          // every buffer below holds B R pseudo-members
    Workspace &w = g->work();
    const size_t out_elems = (size_t)B * 2 * npix;
    if (w.mean_elems < out_elems) {
        w.free_mean();
        QGX_HIP(hipMalloc((void **)&w.mean_acc, out_elems * sizeof(double)));
        w.mean_elems = out_elems;
    }
    const bool regression = g->n_nets == 2;
    if (regression) {
        // net_mean(q / x_std), ONCE on the B members (cgan_regression.py:169-170), before the chunks take X over
        hipLaunchKernelGGL(k_prep_input, pg, pb, 0, st, q, (const float *)nullptr, w.X, 2, npix, g->x_std[0], g->x_std[1], g->range_dev);
        if ((rc = cnn_forward(g, g->nets[1], w.X, w.Y1, B, N, st))) return rc;
    }
    const int quads = 2 * npix / 4, n4 = 2 * npix / 4;
    for (int j0 = 0; j0 < M; j0 += R) {
        const int Rc = std::min(R, M - j0);
        // net 0's raw output of the chunk: the (B R, 2, N, N) region behind X (Y0 takes the mean, Y1 the regression net's output)
        float *Yc = w.X + (size_t)B * R * 4 * npix;
        hipLaunchKernelGGL(k_prep_mean, dim3((quads + 255) / 256, B, std::min(Rc, 16)), pb, 0, st, q, w.X, npix, Rc, j0,
                           g->x_std[0], g->x_std[1], seed, member_offset, step, g->range_dev);
        if ((rc = net0_forward(g, w.X, Yc, B * Rc, N, st))) return rc;
        const size_t threads = (size_t)B * n4;
        hipLaunchKernelGGL(k_mean_accumulate, dim3((unsigned)((threads + 255) / 256)), pb, 0, st, (const float *)Yc, w.mean_acc,
                           w.Y0, n4, B, Rc, j0 == 0 ? 1 : 0, j0 + Rc == M ? 1 : 0, (double)M);
    }
    finish(g, nullptr, regression ? FIN_SUM : FIN_PLAIN, regression ? w.Y1 : nullptr, nullptr, S, B, npix, demean, st);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

// what the three creators share: the handle with its kind, scales and zeroed range words
static int new_handle(const char *who, int kind, int n_nets, const float x_std[2], const float y_std[2], int device,
                      qgx_generator **out) {
    QGX_HIP(hipSetDevice(device));
    qgx_generator *g = new (std::nothrow) qgx_generator();
    if (!g) { set_error("out of host memory"); return QGX_ERR_NOMEM; }
    g->kind = kind; g->device = device; g->n_nets = n_nets;
    for (int i = 0; i < 2; ++i) { g->x_std[i] = x_std[i]; g->y_std[i] = y_std[i]; }
    hipError_t e = hipMalloc((void **)&g->range_dev, 2 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(g->range_dev, 0, 2 * sizeof(unsigned));
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        qgx_generator_destroy(g);
        return QGX_ERR_HIP;
    }
    *out = g;
    return QGX_OK;
}
// a creator's last statement: a handle that failed half-way is destroyed, *out is written on success only
static int hand_out(int rc, qgx_generator *g, qgx_generator **out) {
    if (rc) qgx_generator_destroy(g);
    else *out = g;
    return rc;
}

extern "C" int qgx_generator_create(int kind, const qgx_cnn_weights *nets, int n_nets, const float x_std[2],
                                    const float y_std[2], int device, qgx_generator **out) {
    QGX_REQUIRE(nets && out && x_std && y_std, "qgx_generator_create: null argument");
    QGX_REQUIRE(kind == QGX_GEN_GAN || kind == QGX_GEN_VAE || kind == QGX_GEN_GZ || kind == QGX_GEN_OLS,
                "unknown generator kind %d", kind);
    // GAN / VAE: the generator or decoder, and optionally (regression != 'None', cgan_regression.py:59-60) the 2-channel net_mean;
    // OLS: the one AndrewCNN(2, 2) of OLSModel (ols_model.py:29-31)
    QGX_REQUIRE(kind == QGX_GEN_GZ ? n_nets == 2 : kind == QGX_GEN_OLS ? n_nets == 1 : (n_nets == 1 || n_nets == 2),
                "generator kind %d needs %s nets, not %d", kind,
                kind == QGX_GEN_GZ ? "2" : kind == QGX_GEN_OLS ? "1" : "1 or 2", n_nets);
    for (int n = 0; n < n_nets; ++n) {      // every net's shape before anything is allocated
        const int want_in = kind == QGX_GEN_GZ || kind == QGX_GEN_OLS || n == 1 ? 2 : 4;
        // n_out = 4: a flux-form net (AndrewCNN(n_in, 2, div=True)), each net of a GAN / VAE / OLS handle on its own; MeanVarModel's
        // variance net has no such form here
        const bool out_ok = nets[n].n_out == 2 || (nets[n].n_out == 4 && kind != QGX_GEN_GZ);
        QGX_REQUIRE(nets[n].n_in == want_in && out_ok, "net %d: n_in=%d n_out=%d, expected %d and %s", n,
                    nets[n].n_in, nets[n].n_out, want_in, kind == QGX_GEN_GZ ? "2" : "2 (or 4: flux form)");
    }
    qgx_generator *g = nullptr;
    int rc = new_handle("qgx_generator_create", kind, n_nets, x_std, y_std, device, &g);
    if (rc) return rc;
    for (int n = 0; n < n_nets && !rc; ++n) rc = cnn_pack_net(g->nets[n], &nets[n]);
    if (!rc) rc = cnn_calibrate(g);
    return hand_out(rc, g, out);
}

// The same rules per kind as qgx_generator_create, for nets described by their architecture.  A descriptor list that spells
// the shipped architecture throughout IS qgx_generator_create (one code path, hence the same handle); otherwise the handle is
// exact f32 only: nets of another architecture are packed for the generic engine (conv_generic.hip), a shipped-architecture
// net beside them (a GAN's / VAE's net_mean) as ever, and takes conv.hip's exact-f32 kernels, as beside a U-Net.
extern "C" int qgx_generator_create_arch(int kind, const qgx_cnn_arch *nets, int n_nets, const float x_std[2],
                                         const float y_std[2], int device, qgx_generator **out) {
    QGX_REQUIRE(nets && out && x_std && y_std, "qgx_generator_create_arch: null argument");
    QGX_REQUIRE(kind == QGX_GEN_GAN || kind == QGX_GEN_VAE || kind == QGX_GEN_GZ || kind == QGX_GEN_OLS,
                "unknown generator kind %d", kind);
    QGX_REQUIRE(kind == QGX_GEN_GZ ? n_nets == 2 : kind == QGX_GEN_OLS ? n_nets == 1 : (n_nets == 1 || n_nets == 2),
                "generator kind %d needs %s nets, not %d", kind,
                kind == QGX_GEN_GZ ? "2" : kind == QGX_GEN_OLS ? "1" : "1 or 2", n_nets);
    bool all_shipped = true;
    for (int n = 0; n < n_nets; ++n) {      // every field of every net before anything is allocated
        if (const int rc = cnn_arch_check(&nets[n], n)) return rc;
        const int want_in = kind == QGX_GEN_GZ || kind == QGX_GEN_OLS || n == 1 ? 2 : 4;
        const int n_out = nets[n].channels[nets[n].n_layers];
        QGX_REQUIRE(nets[n].channels[0] == want_in && (n_out == 2 || kind != QGX_GEN_GZ),
                    "qgx_cnn_arch (net %d): channels[0] = %d, channels[%d] = %d, expected n_in %d and n_out %s", n, nets[n].channels[0],
                    nets[n].n_layers, n_out, want_in, kind == QGX_GEN_GZ ? "2" : "2 (or 4: flux form)");
        all_shipped = all_shipped && cnn_arch_is_shipped(&nets[n]);
    }
    if (all_shipped) {
        qgx_cnn_weights w[2];
        for (int n = 0; n < n_nets; ++n) cnn_arch_to_weights(&nets[n], &w[n]);
        return qgx_generator_create(kind, w, n_nets, x_std, y_std, device, out);
    }
    qgx_generator *g = nullptr;
    int rc = new_handle("qgx_generator_create_arch", kind, n_nets, x_std, y_std, device, &g);
    if (rc) return rc;
    cnn_exact_f32_only(g);
    g->generic = 1;
    for (int n = 0; n < n_nets && !rc; ++n) {
        if (cnn_arch_is_shipped(&nets[n])) {
            qgx_cnn_weights w;
            cnn_arch_to_weights(&nets[n], &w);
            rc = cnn_pack_net(g->nets[n], &w);
        } else rc = cnn_pack_net_arch(g->nets[n], &nets[n]);
    }
    g->actw[0] = g->actw[1] = 8;
    for (int n = 0; n < n_nets; ++n)
        for (int k = 0; k < 2; ++k) g->actw[k] = std::max(g->actw[k], g->nets[n].act_width(k));
    return hand_out(rc, g, out);
}

extern "C" int qgx_generator_create_unet(const qgx_unet_weights *w, const qgx_cnn_weights *net_mean, const float x_std[2],
                                         const float y_std[2], int device, qgx_generator **out) {
    QGX_REQUIRE(w && out && x_std && y_std, "qgx_generator_create_unet: null argument");
    QGX_REQUIRE(!net_mean || (net_mean->n_in == 2 && (net_mean->n_out == 2 || net_mean->n_out == 4)),
                "qgx_generator_create_unet: net_mean must be an AndrewCNN(2, 2), n_out = 4 in flux form (n_in=%d n_out=%d)", net_mean->n_in, net_mean->n_out);
    qgx_generator *g = nullptr;
    int rc = new_handle("qgx_generator_create_unet", QGX_GEN_GAN, net_mean ? 2 : 1, x_std, y_std, device, &g);
    if (rc) return rc;
    // exact f32 throughout: the U-Net has no f16x3 path, and net_mean takes the exact-f32 AndrewCNN kernels
    cnn_exact_f32_only(g);
    g->nets[0].n_in = 4; g->nets[0].n_out = 2;
    rc = unet_create(w, &g->unet);
    if (!rc && net_mean) rc = cnn_pack_net(g->nets[1], net_mean);
    return hand_out(rc, g, out);
}

extern "C" int qgx_generator_create_ann(const qgx_ann_weights *w, float x_scale, float y_scale, int device,
                                        qgx_generator **out) {
    QGX_REQUIRE(w && out, "qgx_generator_create_ann: null argument");
    if (int rc = ann_check(w)) return rc;        // every shape before the device is touched
    const float xs[2] = {x_scale, x_scale}, ys[2] = {y_scale, y_scale};   // scalars: one net for both layers
    qgx_generator *g = nullptr;
    int rc = new_handle("qgx_generator_create_ann", QGX_GEN_ANN, 1, xs, ys, device, &g);
    if (rc) return rc;
    cnn_exact_f32_only(g);
    g->nets[0].n_in = 1; g->nets[0].n_out = 1;
    return hand_out(ann_create(w, &g->ann), g, out);
}

extern "C" int qgx_generator_destroy(qgx_generator *g) {
    if (!g) return QGX_OK;
    (void)hipSetDevice(g->device);
    for (NetHost &net : g->nets) cnn_free_net(net);
    for (Workspace &w : g->ws) { w.free_activations(); w.free_part(); w.free_mean(); }
    if (g->range_dev) (void)hipFree(g->range_dev);
    unet_destroy(g->unet);
    ann_destroy(g->ann);
    for (hipEvent_t e : g->prof_ev) (void)hipEventDestroy(e);
    delete g;
    return QGX_OK;
}

extern "C" int qgx_generator_range_read(qgx_generator *g, unsigned *flags, float *input_absmax, void *stream) {
    QGX_REQUIRE(g && flags && input_absmax, "qgx_generator_range_read: null argument");
    unsigned h[2] = {0, 0};
    QGX_HIP(hipMemcpyAsync(h, g->range_dev, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
    QGX_HIP(hipMemsetAsync(g->range_dev, 0, sizeof(h), (hipStream_t)stream));
    QGX_HIP(hipStreamSynchronize((hipStream_t)stream));
    *flags = h[0];
    memcpy(input_absmax, &h[1], sizeof(float));
    return QGX_OK;
}

extern "C" int qgx_generator_forward(qgx_generator *g, const double *q_dev, const void *z_dev, double *S_dev,
                                     int B, int N, int demean, void *stream) {
    return generator_forward(g, q_dev, z_dev, S_dev, B, N, demean, (hipStream_t)stream, nullptr);
}

extern "C" int qgx_generator_forward_mean(qgx_generator *g, const double *q_dev, double *S_dev, int B, int N, int M, int chunk,
                                          int demean, uint64_t seed, uint64_t member_offset, uint64_t step, void *stream) {
    return generator_forward_mean(g, q_dev, S_dev, B, N, M, chunk, demean, seed, member_offset, step, (hipStream_t)stream);
}

extern "C" int qgx_generator_size_ok(const qgx_generator *g, int inet, int B, int N) {
    QGX_REQUIRE(g && inet >= -1 && inet < g->n_nets, "qgx_generator_size_ok: bad argument");
    return generator_size_ok(g, B, N, inet);
}

extern "C" int qgx_cnn_forward(qgx_generator *g, int inet, const float *x_dev, float *y_dev, int B, int N,
                               void *stream) {
    QGX_REQUIRE(g && x_dev && y_dev && inet >= 0 && inet < g->n_nets && B > 0, "qgx_cnn_forward: bad argument");
    if (const int src = generator_size_ok(g, B, N, inet)) return src;
    int rc = generator_reserve(g, B, N);
    if (rc) return rc;
    launch_absmax(x_dev, (size_t)B * g->nets[inet].n_in * N * N, g->range_dev, (hipStream_t)stream);
    if (g->ann) return ann_forward_x(g->ann, x_dev, y_dev, B, N, (hipStream_t)stream);   // (B, 1, N, N) -> (B, 1, N, N)
    if (inet == 0) return net0_forward(g, x_dev, y_dev, B, N, (hipStream_t)stream);
    return cnn_forward(g, g->nets[inet], x_dev, y_dev, B, N, (hipStream_t)stream);
}

extern "C" int qgx_moments_accumulate(const float *y_dev, double *sum_dev, double *sumsq_dev, size_t n, void *stream) {
    QGX_REQUIRE(y_dev && sum_dev && sumsq_dev && n > 0, "qgx_moments_accumulate: bad argument");
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_moments, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       y_dev, sum_dev, sumsq_dev, n);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
