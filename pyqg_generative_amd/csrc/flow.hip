// The derived flow fields behind dataset_statistics / dataset_smart_read, for whole stacks of velocity snapshots.
//
// Restates pyqg_generative/tools/comparison_tools.py:305-324 (and :209-217) per (snapshot, layer) plane of u, v:
//
//   omega = curl(u, v) = ddx(v) - ddy(u)      FeatureExtractor 'curl(u,v)': ifft(ik vh - il uh), spectral on the fields' grid
//   KE    = (u^2 + v^2) / 2,  Vabs = sqrt(2 KE),  Ens = omega^2 / 2
//   KE_time: the plane sum of KE (the layer weights and the division by runs x N^2 stay on the host)
//
// all of it in float64 whatever the input dtype.  Small grids: ONE LDS-resident kernel, one workgroup per plane: u and v are
// read once and travel as the packed pair (u + i v) through one forward complex transform; the half spectra come out of it as
// uh = (Z(k) + conj Z(-k)) / 2, vh = (Z(k) - conj Z(-k)) / 2i; W = ik vh - il uh is written back IN PLACE with its Hermitian
// extension; one inverse transform, omega is its real part.  On a self-conjugate column (i = 0, N/2) the stored value is
// the Hermitian mean of rows j and -j, which is what a complex-to-real transform makes of the half spectrum qgx_spec_curl
// writes: there kx of column N/2 and ly of row N/2 cancel.  Other grids: the plan's batched transforms around three small
// kernels, one plane (u, v) per member of the plan, in chunks of its members — no plane shares a transform with another, so
// a NaN stays in its plane on both paths.  The plane sum is a fixed-order reduction by a workgroup of always 1024 threads.
#include "common.hpp"
#include "fft_lds.hpp"
#include "spectral_elem.hpp"
#include "spectral_pack.hpp"

namespace qgx {

struct FlowArgs {
    const void *u, *v;              // (P, N, N) float or double, P = 2 S planes
    double *omega;                  // (P, N, N) or null
    void *ke, *vabs;                // (P, N, N) input dtype, or null
    double *ens;                    // (P, N, N) or null
    double *ke_sum;                 // (P) or null
};

constexpr int FLOW_THREADS = 1024;

// ---- per-element formulas, shared by both paths
__device__ __forceinline__ double flow_sq(double u, double v) { return u * u + v * v; }
__device__ __forceinline__ double flow_ke(double s) { return 0.5 * s; }
__device__ __forceinline__ double flow_vabs(double s) { return sqrt(s); }
__device__ __forceinline__ double flow_ens(double w) { return 0.5 * (w * w); }
// W = ik vh - il uh
__device__ __forceinline__ double2 flow_curl_hat(double kx, double ly, double2 uh, double2 vh) {
    return make_double2(-kx * vh.y - (-ly * uh.y), kx * vh.x - ly * uh.x);
}

// KE, Vabs of element idx of a plane stored, and this element's share of the plane sum returned
template <typename T>
__device__ __forceinline__ double flow_point(const FlowArgs &a, size_t o, double u, double v) {
    const double s = flow_sq(u, v), ke = flow_ke(s);
    if (a.ke) reinterpret_cast<T *>(a.ke)[o] = (T)ke;
    if (a.vabs) reinterpret_cast<T *>(a.vabs)[o] = (T)flow_vabs(s);
    return ke;
}

// the sum of x over the workgroup in a fixed order (per-thread partial sums, wave shuffles, waves in order), on thread 0
__device__ __forceinline__ double flow_block_sum(double x) {
    __shared__ double s_part[FLOW_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < FLOW_THREADS / 64; ++w) t += s_part[w];
    return t;
}

// ------------------------------------------------------------------ small grids: everything in one kernel
template <int NN, typename T>
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_small(SpecDev d, FlowArgs a) {
    double2 *Z = reinterpret_cast<double2 *>(qgx_smem);
    int *pos_lds;
    Grid g = make_grid(d, Z, pos_lds);
    if (NN) { g.N = NN; g.NK = NN / 2 + 1; g.LD = NN + 1; }
    const int N = NN ? NN : d.N, NK = NN ? NN / 2 + 1 : d.NK, LD = NN ? NN + 1 : d.LD;
    const int sz = N * NK, rz = N * N;
    const size_t po = (size_t)blockIdx.x * rz;
    const T *u = reinterpret_cast<const T *>(a.u) + po, *v = reinterpret_cast<const T *>(a.v) + po;
    const bool curl = a.omega || a.ens;          // (uniform over the launch)
    // ---- u, v read once: the pointwise fields, the plane sum's shares, the pair (u + i v) into LDS
    double part = 0.0;
    for (int idx = threadIdx.x; idx < rz; idx += FLOW_THREADS) {
        const double uu = (double)u[idx], vv = (double)v[idx];
        part += flow_point<T>(a, po + idx, uu, vv);
        if (curl) {
            const int y = idx / N, x = idx - y * N;
            Z[y * LD + x] = make_double2(uu, vv);
        }
    }
    if (a.ke_sum) {
        const double t = flow_block_sum(part);
        if (threadIdx.x == 0) a.ke_sum[blockIdx.x] = t;
    }
    if (!curl) return;
    __syncthreads();                             // (the pair and make_grid's tables)
    fft2d_fwd_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
    // ---- W = ik vh - il uh as the pair (W + i 0), IN PLACE: the thread of element (j, i) reads and writes the field at (j, i)
    // and at its mirror (-j, -i) only.  On a self-conjugate column both are elements of the half spectrum: the thread of the
    // smaller row does both, the other one nothing
    const double2 zero = make_double2(0.0, 0.0);
    for (int idx = threadIdx.x; idx < sz; idx += FLOW_THREADS) {
        const int j = idx / NK, i = idx - j * NK;
        const bool selfc = i == 0 || 2 * i == N;
        const int jm = neg_mod(j, N);
        if (selfc && jm < j) continue;
        const double kx = d.kk[i];
        double2 uh, vh;
        unpack_pair(Z, g, j, i, uh, vh);
        const double2 w = flow_curl_hat(kx, d.ll[j], uh, vh);
        if (!selfc) { pack_store(Z, g, j, i, w, zero, d.invN2); continue; }
        double2 um, vm;
        unpack_pair(Z, g, jm, i, um, vm);
        const double2 wm = flow_curl_hat(kx, d.ll[jm], um, vm);
        pack_store(Z, g, j, i, herm_mean(w, wm), zero, d.invN2);
        if (jm != j) pack_store(Z, g, jm, i, herm_mean(wm, w), zero, d.invN2);
    }
    __syncthreads();
    fft2d_inv_x<NN>(Z, N, LD, g.nrad, g.rad, g.tw);
    for (int idx = threadIdx.x; idx < rz; idx += FLOW_THREADS) {
        const int y = idx / N, x = idx - y * N;
        const double w = Z[y * LD + x].x;
        if (a.omega) a.omega[po + idx] = w;
        if (a.ens) a.ens[po + idx] = flow_ens(w);
    }
}

// ------------------------------------------------------------------ other grids: three kernels around the batched transforms
// one workgroup per plane of the chunk: the pointwise fields and the plane sum; pair (null: no curl asked for) <- the plane's
// (u, v) as the two real fields of member p, float64.  a's pointers are the chunk's.
template <typename T>
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_points(int rz, FlowArgs a, double *pair) {
    const size_t po = (size_t)blockIdx.x * rz;
    const T *u = reinterpret_cast<const T *>(a.u) + po, *v = reinterpret_cast<const T *>(a.v) + po;
    double part = 0.0;
    for (int idx = threadIdx.x; idx < rz; idx += FLOW_THREADS) {
        const double uu = (double)u[idx], vv = (double)v[idx];
        part += flow_point<T>(a, po + idx, uu, vv);
        if (pair) { pair[2 * po + idx] = uu; pair[2 * po + rz + idx] = vv; }
    }
    if (a.ke_sum) {
        const double t = flow_block_sum(part);
        if (threadIdx.x == 0) a.ke_sum[blockIdx.x] = t;
    }
}

// h (P, 2, N, NK): (uh, vh) -> (W, 0), in place; grid (chunks, P)
__global__ void k_flow_curl(SpecDev d, double2 *h) {
    const int sz = d.N * d.NK;
    double2 *h0 = h + (size_t)blockIdx.y * 2 * sz, *h1 = h0 + sz;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < sz; idx += gridDim.x * blockDim.x) {
        const int j = idx / d.NK, i = idx - j * d.NK;
        h0[idx] = flow_curl_hat(d.kk[i], d.ll[j], h0[idx], h1[idx]);
        h1[idx] = make_double2(0.0, 0.0);
    }
}

// pair (P, 2, N, N): omega is field 0 of member p; grid (chunks, P)
__global__ void k_flow_store(int rz, const double *pair, double *omega, double *ens) {
    const size_t po = (size_t)blockIdx.y * rz;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < rz; idx += gridDim.x * blockDim.x) {
        const double w = pair[2 * po + idx];
        if (omega) omega[po + idx] = w;
        if (ens) ens[po + idx] = flow_ens(w);
    }
}

// ------------------------------------------------------------------ host
static size_t flow_small_lds_bytes(const SpecDev &d) {      // field + digit-reversal table + twiddle table (make_grid)
    size_t bytes = (size_t)d.N * d.LD * sizeof(double2) + (size_t)((d.N + 3) & ~3) * sizeof(int) + (size_t)d.N * sizeof(double2);
    return (bytes + 15) & ~(size_t)15;
}
static size_t flow_align(size_t a) { return (a + 255) & ~(size_t)255; }
// planes per chunk of the batched path, and its two work fields: the pair (C, 2, N, N) real, the spectra (C, 2, N, NK) complex
static int64_t flow_chunk(const qgx_model *m, int64_t S) { return 2 * S < (int64_t)m->B ? 2 * S : (int64_t)m->B; }
static size_t flow_pair_bytes(const qgx_model *m, int64_t S) { return flow_align((size_t)flow_chunk(m, S) * 2 * m->N * m->N * sizeof(double)); }
static size_t flow_work_bytes(const qgx_model *m, int64_t S) {
    if (m->small) return 0;
    return flow_pair_bytes(m, S) + flow_align((size_t)flow_chunk(m, S) * 2 * m->N * m->NK * sizeof(double2));
}

#define QGX_FLOW_DISPATCH_N(N_, CALL)           \
    switch (N_) {                               \
        case 32: { constexpr int NN = 32; CALL; } break; \
        case 48: { constexpr int NN = 48; CALL; } break; \
        case 64: { constexpr int NN = 64; CALL; } break; \
        case 96: { constexpr int NN = 96; CALL; } break; \
        default: { constexpr int NN = 0; CALL; } break;  \
    }

template <typename T>
static int flow_small(const SpecDev &d, const FlowArgs &a, int64_t planes, hipStream_t st) {
    const size_t lds = flow_small_lds_bytes(d);
    QGX_FLOW_DISPATCH_N(d.N, {
        QGX_HIP(hipFuncSetAttribute((const void *)(k_flow_small<NN, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_flow_small<NN, T>), dim3((unsigned)planes), dim3(FLOW_THREADS), lds, st, d, a);
    })
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

template <typename T>
static int flow_large(qgx_model *m, const FlowArgs &all, int64_t planes, void *work, hipStream_t st) {
    const int N = m->N, rz = N * N, sz = N * m->NK;
    const int64_t C = planes < (int64_t)m->B ? planes : (int64_t)m->B;
    const bool curl = all.omega || all.ens;
    double *pair = reinterpret_cast<double *>(work);
    double2 *spec = reinterpret_cast<double2 *>((char *)work + flow_pair_bytes(m, planes / 2));
    // a view of the plan with the chunk's member count (the last chunk may be short); it owns nothing
    qgx_model view = *m;
    for (int64_t p0 = 0; p0 < planes; p0 += C) {
        const int n = (int)(planes - p0 < C ? planes - p0 : C);
        const size_t o = (size_t)p0 * rz;
        FlowArgs a;
        a.u = reinterpret_cast<const T *>(all.u) + o;
        a.v = reinterpret_cast<const T *>(all.v) + o;
        a.omega = all.omega ? all.omega + o : nullptr;
        a.ens = all.ens ? all.ens + o : nullptr;
        a.ke = all.ke ? reinterpret_cast<T *>(all.ke) + o : nullptr;
        a.vabs = all.vabs ? reinterpret_cast<T *>(all.vabs) + o : nullptr;
        a.ke_sum = all.ke_sum ? all.ke_sum + p0 : nullptr;
        if (a.ke || a.vabs || a.ke_sum || curl)
            hipLaunchKernelGGL(k_flow_points<T>, dim3(n), dim3(FLOW_THREADS), 0, st, rz, a, curl ? pair : (double *)nullptr);
        if (!curl) continue;
        view.B = n; view.d.B = n;
        int rc;
        if ((rc = large_q_to_qh(&view, pair, spec, st))) return rc;
        const dim3 gs((unsigned)((sz + 255) / 256 > 1024 ? 1024 : (sz + 255) / 256), n);
        const dim3 gr((unsigned)((rz + 255) / 256 > 1024 ? 1024 : (rz + 255) / 256), n);
        hipLaunchKernelGGL(k_flow_curl, gs, dim3(256), 0, st, view.d, spec);
        if ((rc = large_qh_to_q(&view, spec, pair, st))) return rc;
        hipLaunchKernelGGL(k_flow_store, gr, dim3(256), 0, st, rz, (const double *)pair, a.omega, a.ens);
    }
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
#undef QGX_FLOW_DISPATCH_N

}  // namespace qgx

using namespace qgx;

extern "C" int qgx_flow_features_workspace(const qgx_model *plan, int64_t S, size_t *bytes) {
    QGX_REQUIRE(plan && bytes, "qgx_flow_features_workspace: null argument");
    QGX_REQUIRE(S >= 1 && S <= (int64_t)0x3fffffff, "qgx_flow_features_workspace: S must be in [1, 2^30) (got %lld)", (long long)S);
    *bytes = flow_work_bytes(plan, S);
    return QGX_OK;
}

extern "C" int qgx_flow_features(qgx_model *plan, const void *u_dev, const void *v_dev, int is_double, int64_t S,
                                 double *omega_dev, void *ke_dev, double *ens_dev, void *vabs_dev, double *ke_sum_dev,
                                 void *work_dev, size_t work_bytes, void *stream) {
    QGX_REQUIRE(plan && u_dev && v_dev, "qgx_flow_features: null argument");
    QGX_REQUIRE(S >= 1 && S <= (int64_t)0x3fffffff, "qgx_flow_features: S must be in [1, 2^30) (got %lld)", (long long)S);
    QGX_REQUIRE(is_double == 0 || is_double == 1, "qgx_flow_features: is_double must be 0 or 1 (got %d)", is_double);
    QGX_REQUIRE(omega_dev || ke_dev || ens_dev || vabs_dev || ke_sum_dev, "qgx_flow_features: every output is NULL");
    const size_t need = flow_work_bytes(plan, S);
    QGX_REQUIRE(work_bytes >= need && (work_dev || need == 0), "qgx_flow_features: work space of %zu bytes, %zu needed",
                work_dev ? work_bytes : (size_t)0, need);
    FlowArgs a;
    a.u = u_dev; a.v = v_dev; a.omega = omega_dev; a.ke = ke_dev; a.ens = ens_dev; a.vabs = vabs_dev; a.ke_sum = ke_sum_dev;
    hipStream_t st = (hipStream_t)stream;
    if (plan->small) return is_double ? flow_small<double>(plan->d, a, 2 * S, st) : flow_small<float>(plan->d, a, 2 * S, st);
    return is_double ? flow_large<double>(plan, a, 2 * S, work_dev, st) : flow_large<float>(plan, a, 2 * S, work_dev, st);
}
