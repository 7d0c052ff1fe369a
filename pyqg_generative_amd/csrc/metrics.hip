// Online metrics (reference: pyqg_generative/tools/comparison_tools.py:116-195 diagnostic_differences_Perezhogin):
// the exact 1-Wasserstein distance scipy.stats.wasserstein_distance computes (_stats_py.py::_cdf_distance, p = 1),
//     W1 = sum_k |i_k/n_u - j_k/n_v| * (a_{k+1} - a_k)  over the merged sorted sample a,
// and the spectral curl behind the enstrophy feature.
//   keys     one pass over the strided input: feature -> order-preserving unsigned key, per-block sums of feature^2
//            and counts of non-finite values (a second one-block launch adds them in a fixed order)
//   sort     keys-only LSD radix sort, 8-bit digits; per pass: histogram of every 4096-key tile, one workgroup per
//            digit scans that digit's tile counts, stable scatter (ranks per wave by ballot, tile staged in LDS so each
//            digit's run is written contiguously).  No workgroup waits for another: each step is its own launch.
//   merge    merge path: a workgroup finds the co-ranks of its diagonal range, each thread the co-rank of its 32
//            diagonals inside that range, walks them and sums the terms in float64; a fixed tree per workgroup, then
//            one workgroup sums the partials in a fixed order.
// Every launch is on the caller's stream; nothing is memset.
#include "common.hpp"
#include <cmath>

namespace qgx {
namespace {

constexpr int KEY_THREADS = 256;
constexpr int SORT_THREADS = 256, SORT_WAVES = SORT_THREADS / 64, SORT_ITEMS = 16;
constexpr int TILE = SORT_THREADS * SORT_ITEMS;          // 4096 keys per tile
constexpr int WAVE_SEG = 64 * SORT_ITEMS;                // 1024 consecutive keys per wave
constexpr int RADIX = 256;
constexpr int MERGE_THREADS = 256, MERGE_ITEMS = 32;
constexpr int MERGE_SPAN = MERGE_THREADS * MERGE_ITEMS;  // 8192 merge positions per workgroup

// ---- keys -------------------------------------------------------------------------------------------------------
__device__ inline uint64_t key_of(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline uint32_t key_of(float x) {
    const uint32_t b = (uint32_t)__float_as_uint(x);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ inline double value_of(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ inline double value_of(uint32_t k) {
    return (double)__uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
__device__ inline double feature_of(const T *x, const T *y, size_t off, int feature) {
    // numpy's u**2 + v**2: two rounded squares and a rounded sum.  __dmul_rn / __dadd_rn are plain * and + in this toolchain's
    // headers, compiled with the default -ffp-contract, and fused into an fma after inlining (one rounding less for a float64
    // input): the products are written out here with contraction switched off for this function.
#pragma clang fp contract(off)
    const double a = (double)x[off];
    if (feature == QGX_W1_IDENTITY) return a;
    const double aa = a * a;
    if (feature == QGX_W1_SQUARE) return aa;
    const double b = (double)y[off];
    const double bb = b * b;
    return aa + bb;
}

// fixed-order tree over one value per thread of a KEY_THREADS / MERGE_THREADS (= 256) workgroup; result in lane 0
__device__ inline double block_sum_256(double v, double *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

template <typename T, typename K>
__global__ __launch_bounds__(KEY_THREADS) void k_w1_keys(const T *x, const T *y, int feature, int64_t T_, int64_t P,
                                                         int64_t stride_r, int64_t stride_t, size_t n, K *keys,
                                                         double *partials) {
    __shared__ double red[KEY_THREADS];
    double ss = 0., bad = 0.;
    const size_t rowlen = (size_t)P, rows_per_run = (size_t)T_;
    for (size_t e = (size_t)blockIdx.x * KEY_THREADS + threadIdx.x; e < n; e += (size_t)gridDim.x * KEY_THREADS) {
        const size_t row = e / rowlen, p = e - row * rowlen;
        const size_t r = row / rows_per_run, t = row - r * rows_per_run;
        const size_t off = r * (size_t)stride_r + t * (size_t)stride_t + p;
        const double f = feature_of(x, y, off, feature);
        if (!isfinite(f)) bad += 1.;
        ss += f * f;
        if constexpr (sizeof(K) == 4) keys[e] = key_of((float)f);   // float identity feature only: (float)f == x
        else keys[e] = key_of(f);
    }
    const double s = block_sum_256(ss, red);
    __syncthreads();
    const double b = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s;
        partials[QGX_W1_PARTIALS + blockIdx.x] = b;
    }
}

// stats[0] = sum of partials[0 .. nblk), stats[1] = sum of partials[QGX_W1_PARTIALS ...]: one workgroup, fixed order.
// The entries of blocks that were not launched are zeroed, so the caller's scratch is defined in full after the call.
__global__ __launch_bounds__(256) void k_w1_keys_finish(double *partials, int nblk, double *stats) {
    __shared__ double red[256];
    double s = 0., b = 0.;
    for (int i = nblk + threadIdx.x; i < QGX_W1_PARTIALS; i += 256) {
        partials[i] = 0.;
        partials[QGX_W1_PARTIALS + i] = 0.;
    }
    for (int i = threadIdx.x; i < nblk; i += 256) {
        s += partials[i];
        b += partials[QGX_W1_PARTIALS + i];
    }
    const double S = block_sum_256(s, red);
    __syncthreads();
    const double B = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        stats[0] = S;
        stats[1] = B;
    }
}

// ---- radix sort -------------------------------------------------------------------------------------------------
// tile b holds keys [b*TILE, (b+1)*TILE); wave w of its workgroup owns [w*WAVE_SEG, (w+1)*WAVE_SEG) of the tile and
// reads item i at lane offset i*64 + lane, so (wave, item, lane) is the keys' order inside the tile
template <typename K>
__global__ __launch_bounds__(SORT_THREADS) void k_radix_hist(const K *keys, size_t n, int shift, uint32_t *counts,
                                                             size_t ntiles) {
    __shared__ uint32_t hist[RADIX];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * TILE + (threadIdx.x >> 6) * WAVE_SEG + (threadIdx.x & 63);
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        const size_t idx = base + (size_t)i * 64;
        if (idx < n) atomicAdd(&hist[(uint32_t)(keys[idx] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
}

// exclusive scan of 256 values, one per thread of a 256-thread workgroup; returns the thread's prefix, *total the sum
template <typename V>
__device__ inline V block_exclusive_scan_256(V v, V *lds, V *total) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const V add = (int)threadIdx.x >= s ? lds[threadIdx.x - s] : V(0);
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    const V incl = lds[threadIdx.x];
    *total = lds[255];
    __syncthreads();
    return incl - v;
}

// workgroup d: offs[d][b] = sum of counts[d][0 .. b), totals[d] = sum over all tiles
__global__ __launch_bounds__(256) void k_radix_scan(const uint32_t *counts, size_t ntiles, uint64_t *offs,
                                                    uint64_t *totals) {
    __shared__ uint64_t lds[256];
    const size_t row = (size_t)blockIdx.x * ntiles;
    uint64_t carry = 0;
    for (size_t c = 0; c < ntiles; c += 256 * 4) {
        uint32_t v[4];
        uint64_t s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t i = c + (size_t)threadIdx.x * 4 + q;
            v[q] = i < ntiles ? counts[row + i] : 0u;
            s += v[q];
        }
        uint64_t tot;
        uint64_t pre = carry + block_exclusive_scan_256<uint64_t>(s, lds, &tot);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t i = c + (size_t)threadIdx.x * 4 + q;
            if (i < ntiles) offs[row + i] = pre;
            pre += v[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

template <typename K>
__global__ __launch_bounds__(SORT_THREADS) void k_radix_scatter(const K *in, K *out, size_t n, int shift,
                                                                const uint64_t *offs, const uint64_t *totals,
                                                                size_t ntiles) {
    __shared__ K stage[TILE];
    __shared__ uint32_t wcnt[SORT_WAVES][RADIX];      // per-wave running counts, then per-wave prefixes
    __shared__ uint32_t tstart[RADIX];                // first local position of each digit in the tile
    __shared__ uint64_t gbase[RADIX];                 // global position of the tile's first key of each digit
    __shared__ uint64_t scan64[RADIX];
    __shared__ uint32_t scan32[RADIX];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t tile0 = (size_t)blockIdx.x * TILE;

    // digit d's keys start at (sum of totals[0 .. d)) + offs[d][tile]
    uint64_t all;
    const uint64_t dbase = block_exclusive_scan_256<uint64_t>(totals[tid], scan64, &all);
    gbase[tid] = dbase + offs[(size_t)tid * ntiles + blockIdx.x];
#pragma unroll
    for (int q = 0; q < SORT_WAVES; ++q) wcnt[q][tid] = 0;
    __syncthreads();

    K key[SORT_ITEMS];
    uint32_t rank[SORT_ITEMS];
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    volatile uint32_t *cnt = wcnt[w];
    const size_t base = tile0 + (size_t)w * WAVE_SEG + lane;
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        const size_t idx = base + (size_t)i * 64;
        const bool valid = idx < n;
        key[i] = valid ? in[idx] : K(0);
        const uint32_t d = (uint32_t)(key[i] >> shift) & (RADIX - 1);
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const uint64_t b = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? b : ~b;
        }
        const uint32_t prior = valid ? cnt[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        rank[i] = prior + (uint32_t)__popcll(m & lt);
        if (valid && (m & lt) == 0) cnt[d] = prior + (uint32_t)__popcll(m);   // the group's lowest lane
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    uint32_t tile_count = 0;
#pragma unroll
    for (int q = 0; q < SORT_WAVES; ++q) {
        const uint32_t c = wcnt[q][tid];
        wcnt[q][tid] = tile_count;
        tile_count += c;
    }
    uint32_t tile_n;
    tstart[tid] = block_exclusive_scan_256<uint32_t>(tile_count, scan32, &tile_n);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SORT_ITEMS; ++i) {
        if (base + (size_t)i * 64 < n) {
            const uint32_t d = (uint32_t)(key[i] >> shift) & (RADIX - 1);
            stage[tstart[d] + wcnt[w][d] + rank[i]] = key[i];
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < tile_n; j += SORT_THREADS) {
        const K k = stage[j];
        const uint32_t d = (uint32_t)(k >> shift) & (RADIX - 1);
        out[gbase[d] + (j - tstart[d])] = k;
    }
}

// ---- merge path -------------------------------------------------------------------------------------------------
// number of a-keys among the first d keys of the merge (ties: a first), searched in [lo, hi]
template <typename K>
__device__ inline size_t co_rank(const K *a, size_t na, const K *b, size_t nb, size_t d, size_t lo, size_t hi) {
    lo = lo > (d > nb ? d - nb : 0) ? lo : (d > nb ? d - nb : 0);
    hi = hi < (d < na ? d : na) ? hi : (d < na ? d : na);
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;      // mid < d and d - mid - 1 < nb inside the clamped range
        if (a[mid] <= b[d - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename K>
__global__ __launch_bounds__(MERGE_THREADS) void k_w1_merge(const K *a, size_t na, const K *b, size_t nb,
                                                            double *partials) {
    __shared__ size_t range[2];
    __shared__ double red[MERGE_THREADS];
    const size_t n = na + nb;
    const size_t D0 = (size_t)blockIdx.x * MERGE_SPAN, D1 = D0 + MERGE_SPAN < n ? D0 + MERGE_SPAN : n;
    if (threadIdx.x < 2) range[threadIdx.x] = co_rank(a, na, b, nb, threadIdx.x ? D1 : D0, 0, na);
    __syncthreads();
    const double dna = (double)na, dnb = (double)nb;
    double acc = 0.;
    const size_t d0 = D0 + (size_t)threadIdx.x * MERGE_ITEMS;
    if (d0 < D1) {
        const size_t d1 = d0 + MERGE_ITEMS < D1 ? d0 + MERGE_ITEMS : D1;
        size_t i = co_rank(a, na, b, nb, d0, range[0], range[1]), j = d0 - i;
        for (size_t k = d0; k < d1; ++k) {
            K cur;
            if (j >= nb || (i < na && a[i] <= b[j])) cur = a[i++];
            else cur = b[j++];
            if (k + 1 < n) {
                const K nxt = (j >= nb || (i < na && a[i] <= b[j])) ? a[i] : b[j];
                acc += fabs((double)i / dna - (double)j / dnb) * (value_of(nxt) - value_of(cur));
            }
        }
    }
    const double s = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_w1_finish(const double *partials, size_t nblk, const double *stats_u,
                                                   const double *stats_v, double *out) {
    __shared__ double red[256];
    double s = 0.;
    for (size_t i = threadIdx.x; i < nblk; i += 256) s += partials[i];
    const double S = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        const bool bad = (stats_u && stats_u[1] != 0.) || (stats_v && stats_v[1] != 0.);
        out[0] = bad ? __longlong_as_double(0x7ff8000000000000ll) : S;
    }
}

// out = ik*v - il*u
__global__ void k_spec_curl(const double2 *uh, const double2 *vh, double2 *out, int N, double dk) {
    const int NK = N / 2 + 1, f = blockIdx.y;
    const size_t o = (size_t)f * N * NK;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < N * NK; idx += gridDim.x * blockDim.x) {
        const int j = idx / NK, i = idx - j * NK;
        const double kx = dk * (double)i, ly = dk * (double)(j < N / 2 ? j : j - N);
        const double2 u = uh[o + idx], v = vh[o + idx];
        out[o + idx] = make_double2(-kx * v.y - (-ly * u.y), kx * v.x - ly * u.x);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t a) { return (a + 255) & ~(size_t)255; }

struct W1Layout {
    size_t alt, counts, offs, totals, partials, total;
};

W1Layout w1_layout(size_t nu, size_t nv, int key_bits) {
    const size_t nmax = nu > nv ? nu : nv, ntiles = ceil_div(nmax, TILE);
    W1Layout L;
    size_t at = 0;
    L.alt = at;      at += align_up(nmax * (size_t)(key_bits / 8));
    L.counts = at;   at += align_up(ntiles * RADIX * sizeof(uint32_t));
    L.offs = at;     at += align_up(ntiles * RADIX * sizeof(uint64_t));
    L.totals = at;   at += align_up(RADIX * sizeof(uint64_t));
    L.partials = at; at += align_up(ceil_div(nu + nv, MERGE_SPAN) * sizeof(double));
    L.total = at;
    return L;
}

template <typename K>
int radix_sort(K *keys, size_t n, char *work, const W1Layout &L, hipStream_t st) {
    const size_t ntiles = ceil_div(n, TILE);
    K *src = keys, *dst = (K *)(work + L.alt);
    uint32_t *counts = (uint32_t *)(work + L.counts);
    uint64_t *offs = (uint64_t *)(work + L.offs), *totals = (uint64_t *)(work + L.totals);
    for (int shift = 0; shift < (int)(8 * sizeof(K)); shift += 8) {      // an even number of passes: ends in `keys`
        hipLaunchKernelGGL(k_radix_hist<K>, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, st, src, n, shift, counts,
                           ntiles);
        hipLaunchKernelGGL(k_radix_scan, dim3(RADIX), dim3(256), 0, st, counts, ntiles, offs, totals);
        hipLaunchKernelGGL(k_radix_scatter<K>, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, st, src, dst, n, shift,
                           offs, totals, ntiles);
        K *t = src; src = dst; dst = t;
    }
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

template <typename K>
int w1_sorted(K *ku, size_t nu, const double *su, K *kv, size_t nv, const double *sv, char *work, const W1Layout &L,
              double *out, hipStream_t st) {
    int rc = radix_sort(ku, nu, work, L, st);
    if (rc) return rc;
    rc = radix_sort(kv, nv, work, L, st);
    if (rc) return rc;
    const size_t nblk = ceil_div(nu + nv, MERGE_SPAN);
    double *partials = (double *)(work + L.partials);
    hipLaunchKernelGGL(k_w1_merge<K>, dim3((unsigned)nblk), dim3(MERGE_THREADS), 0, st, ku, nu, kv, nv, partials);
    hipLaunchKernelGGL(k_w1_finish, dim3(1), dim3(256), 0, st, partials, nblk, su, sv, out);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

template <typename T, typename K>
void launch_keys(const void *x, const void *y, int feature, int64_t T_, int64_t P, int64_t sr, int64_t stt, size_t n,
                 void *keys, double *partials, unsigned nblk, hipStream_t st) {
    hipLaunchKernelGGL((k_w1_keys<T, K>), dim3(nblk), dim3(KEY_THREADS), 0, st, (const T *)x, (const T *)y, feature, T_,
                       P, sr, stt, n, (K *)keys, partials);
}

constexpr size_t MAX_KEYS = (size_t)1 << 40;   // tiles and merge blocks stay far inside a 32-bit grid

}  // namespace
}  // namespace qgx

using namespace qgx;

extern "C" int qgx_w1_workspace(size_t nu, size_t nv, int key_bits, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_w1_workspace: null argument");
    QGX_REQUIRE(nu > 0 && nv > 0 && nu <= MAX_KEYS && nv <= MAX_KEYS,
                "qgx_w1_workspace: sample sizes must be in [1, 2^40] (nu=%zu, nv=%zu)", nu, nv);
    QGX_REQUIRE(key_bits == 32 || key_bits == 64, "qgx_w1_workspace: key_bits must be 32 or 64 (got %d)", key_bits);
    *bytes = w1_layout(nu, nv, key_bits).total;
    return QGX_OK;
}

extern "C" int qgx_w1_keys(const void *x_dev, const void *y_dev, int is_double, int feature, int key_bits, int64_t R,
                           int64_t T, int64_t P, int64_t stride_r, int64_t stride_t, void *keys_dev,
                           double *partials_dev, double *stats_dev, void *stream) {
    QGX_REQUIRE(is_double == 0 || is_double == 1, "qgx_w1_keys: is_double must be 0 or 1 (got %d)", is_double);
    QGX_REQUIRE(feature == QGX_W1_IDENTITY || feature == QGX_W1_SUMSQ2 || feature == QGX_W1_SQUARE,
                "qgx_w1_keys: unknown feature %d", feature);
    QGX_REQUIRE(key_bits == 64 || (key_bits == 32 && !is_double && feature == QGX_W1_IDENTITY),
                "qgx_w1_keys: key_bits must be 64, or 32 for a float identity feature (got %d)", key_bits);
    QGX_REQUIRE(R > 0 && T > 0 && P > 0 && stride_r >= 0 && stride_t >= 0, "qgx_w1_keys: empty or negative view");
    QGX_REQUIRE(x_dev && keys_dev && partials_dev && stats_dev && (feature != QGX_W1_SUMSQ2 || y_dev),
                "qgx_w1_keys: null argument");
    QGX_REQUIRE((size_t)P <= MAX_KEYS && (size_t)T <= MAX_KEYS / (size_t)P &&
                (size_t)R <= MAX_KEYS / ((size_t)T * (size_t)P), "qgx_w1_keys: view too large");
    const size_t n = (size_t)R * (size_t)T * (size_t)P;
    const size_t want = ceil_div(n, KEY_THREADS);
    const unsigned nblk = (unsigned)(want < QGX_W1_PARTIALS ? want : QGX_W1_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    if (is_double) launch_keys<double, uint64_t>(x_dev, y_dev, feature, T, P, stride_r, stride_t, n, keys_dev,
                                                 partials_dev, nblk, st);
    else if (key_bits == 32) launch_keys<float, uint32_t>(x_dev, y_dev, feature, T, P, stride_r, stride_t, n, keys_dev,
                                                          partials_dev, nblk, st);
    else launch_keys<float, uint64_t>(x_dev, y_dev, feature, T, P, stride_r, stride_t, n, keys_dev, partials_dev, nblk,
                                      st);
    hipLaunchKernelGGL(k_w1_keys_finish, dim3(1), dim3(256), 0, st, partials_dev, (int)nblk, stats_dev);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

extern "C" int qgx_w1_sorted(void *keys_u_dev, size_t nu, const double *stats_u_dev, void *keys_v_dev, size_t nv,
                             const double *stats_v_dev, int key_bits, void *work_dev, size_t work_bytes, double *out_dev,
                             void *stream) {
    size_t need = 0;
    const int rc = qgx_w1_workspace(nu, nv, key_bits, &need);
    if (rc) return rc;
    QGX_REQUIRE(work_bytes >= need, "qgx_w1_sorted: work space of %zu bytes, %zu needed", work_bytes, need);
    QGX_REQUIRE(keys_u_dev && keys_v_dev && work_dev && out_dev, "qgx_w1_sorted: null argument");
    const W1Layout L = w1_layout(nu, nv, key_bits);
    hipStream_t st = (hipStream_t)stream;
    if (key_bits == 32)
        return w1_sorted((uint32_t *)keys_u_dev, nu, stats_u_dev, (uint32_t *)keys_v_dev, nv, stats_v_dev,
                         (char *)work_dev, L, out_dev, st);
    return w1_sorted((uint64_t *)keys_u_dev, nu, stats_u_dev, (uint64_t *)keys_v_dev, nv, stats_v_dev, (char *)work_dev,
                     L, out_dev, st);
}

extern "C" int qgx_spec_curl(const double *uh_dev, const double *vh_dev, double *out_dev, int nfields, int N, double L,
                             void *stream) {
    QGX_REQUIRE(uh_dev && vh_dev && out_dev && nfields > 0 && N >= 2 && N % 2 == 0 && nfields <= 65535,
                "qgx_spec_curl: bad argument");
    const int tot = N * (N / 2 + 1);
    dim3 grid((tot + 255) / 256 > 1024 ? 1024 : (tot + 255) / 256, nfields);
    hipLaunchKernelGGL(k_spec_curl, grid, dim3(256), 0, (hipStream_t)stream, (const double2 *)uh_dev,
                       (const double2 *)vh_dev, (double2 *)out_dev, N, 2. * 3.14159265358979323846 / L);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
