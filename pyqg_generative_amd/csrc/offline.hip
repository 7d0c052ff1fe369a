// Offline metrics (reference: pyqg_generative/models/parameterization.py:36-168 Parameterization.test_offline,
// tools/computational_tools.py:5-84 PDF_histogram / subgrid_scores): streaming reductions over the (R, T, 2, N, N)
// truth T, Monte-Carlo mean M, one sample G and the streamfunction psi.
//   spectra    per-wavenumber sums over snapshots of 22 (l, k) planes built from rfft2(.)/N^2 of T, G, M, psi, split by
//              the snapshot's time index into two windows (t < t0, t >= t0).  Snapshot s goes to accumulator group
//              s % QGX_OFFLINE_SPEC_GROUPS; a thread owns one (group, wavenumber) and adds its snapshots in increasing s,
//              so the sums do not depend on how the caller chunks the snapshots.  A finish launch adds the groups in
//              order.
//   moments    two passes of a grouped reduction over (run, time) [spatial], (run, y, x) [temporal] and (run, time, y,
//              x) [global].  A workgroup owns 1024 positions of one layer over a fixed range of (run, time) rows: it keeps
//              the spatial sums per position in registers and reduces every row to per-row sums (waves by shuffles, the
//              workgroup's waves in order).  Merge launches add row groups, runs and times in fixed orders.
//   histogram  counts of x / scale over a strided view with np.histogram's uniform-bin rule (edge correction, closed
//              last bin), per-workgroup LDS counts (integer atomics) added per bin in workgroup order; optionally the
//              view's mean and population std by two passes first.
// No float atomics, no memset, every launch on the caller's stream, 64-bit indexing.
#include "common.hpp"
#include <algorithm>
#include <cmath>

namespace qgx {
namespace {

constexpr int NPL = QGX_OFFLINE_PLANES;             // 22
constexpr int SPEC_G = QGX_OFFLINE_SPEC_GROUPS;     // 32
constexpr int SPEC_THREADS = 256;
constexpr int MOM_THREADS = 256, MOM_PPT = 4, MOM_TILE = MOM_THREADS * MOM_PPT;
constexpr int MOM_RG = 128;                          // at most this many (run, time) row groups
constexpr int MOM_NQS = 6, MOM_NQR = 9;              // pass-2 quantities per position / per row
constexpr int HIST_THREADS = 256, HIST_ITEMS = 8, HIST_BLOCKS = 1024;

inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t a) { return (a + 255) & ~(size_t)255; }

__device__ inline double sq(double2 a) { return a.x * a.x + a.y * a.y; }
__device__ inline double dotc(double2 a, double2 b) { return a.x * b.x + a.y * b.y; }      // Re(conj(a) b)

// ---- spectra ------------------------------------------------------------------------------------------------------
// planes: [f*2 + z] power, [10 + f*2 + z] Re(conj(psi) X), f = T, G, M, R = T - M, GR = G - M; [20] Re(conj(R0) R1),
// [21] Re(conj(GR0) GR1).  acc: (SPEC_G, 2 windows, NPL, P), P = N (N/2+1).
template <bool PSI>
__global__ __launch_bounds__(SPEC_THREADS) void k_offline_spectra(const double2 *th, const double2 *gh, const double2 *mh,
                                                                  const double2 *ph, int64_t S, int64_t P, int64_t s0,
                                                                  int64_t T, int64_t t0, double M2, int accumulate,
                                                                  double *acc) {
    const int64_t p = (int64_t)blockIdx.x * SPEC_THREADS + threadIdx.x;
    const int g = blockIdx.y;
    if (p >= P) return;
    double *A = acc + (int64_t)g * 2 * NPL * P + p;
    double a0[NPL], a1[NPL];       // the running sums themselves: every snapshot is added in the same order however
#pragma unroll                     // the caller chunks them
    for (int k = 0; k < NPL; ++k) {
        a0[k] = accumulate ? A[(int64_t)k * P] : 0.;
        a1[k] = accumulate ? A[(int64_t)(NPL + k) * P] : 0.;
    }
    for (int64_t j = ((int64_t)g - s0 % SPEC_G + SPEC_G) % SPEC_G; j < S; j += SPEC_G) {
        const int64_t o0 = j * 2 * P + p, o1 = o0 + P;
        double c[NPL];
        double2 r[2], q[2];
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            const int64_t o = z ? o1 : o0;
            const double2 tv = th[o], gv = gh[o], mv = mh[o];
            const double2 t = make_double2(tv.x / M2, tv.y / M2), gg = make_double2(gv.x / M2, gv.y / M2),
                          m = make_double2(mv.x / M2, mv.y / M2);
            r[z] = make_double2(t.x - m.x, t.y - m.y);
            q[z] = make_double2(gg.x - m.x, gg.y - m.y);
            c[0 + z] = sq(t); c[2 + z] = sq(gg); c[4 + z] = sq(m); c[6 + z] = sq(r[z]); c[8 + z] = sq(q[z]);
            if (PSI) {
                const double2 pv = ph[o], s = make_double2(pv.x / M2, pv.y / M2);
                c[10 + z] = dotc(s, t); c[12 + z] = dotc(s, gg); c[14 + z] = dotc(s, m); c[16 + z] = dotc(s, r[z]);
                c[18 + z] = dotc(s, q[z]);
            } else {
                c[10 + z] = c[12 + z] = c[14 + z] = c[16 + z] = c[18 + z] = 0.;
            }
        }
        c[20] = dotc(r[0], r[1]);
        c[21] = dotc(q[0], q[1]);
        if ((s0 + j) % T >= t0) {
#pragma unroll
            for (int k = 0; k < NPL; ++k) a1[k] += c[k];
        } else {
#pragma unroll
            for (int k = 0; k < NPL; ++k) a0[k] += c[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        A[(int64_t)k * P] = a0[k];
        A[(int64_t)(NPL + k) * P] = a1[k];
    }
}

__global__ __launch_bounds__(256) void k_offline_spectra_finish(const double *acc, int64_t n, double *out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s = 0.;
        for (int g = 0; g < SPEC_G; ++g) s += acc[(int64_t)g * n + i];
        out[i] = s;
    }
}

// ---- moments ------------------------------------------------------------------------------------------------------
// (R, T, 2, P) rows: row = r*T + t, element (row, z, p) at (row*2 + z)*P + p.
// pass 1: spatial [t, m] sums, row [t, m] sums.
// pass 2: spatial [(t-m)^2, t^2, (t-ts)^2, (m-ms)^2, (t-ts)(m-ms), (g-m)^2] with ts, ms the spatial means;
//         row [(t-m)^2, t^2, (t-tt)^2, (m-mt)^2, (t-tt)(m-mt), (g-m)^2, (t-tg)^2, (m-mg)^2, (t-tg)(m-mg)] with tt, mt the
//         temporal and tg, mg the global means.
struct MomLayout {
    int64_t P, RT, T, ntiles, rpg, ngroups;
    size_t spart, rpart, smean, tsum, tmean, gmean, total;
};

MomLayout mom_layout(int64_t R, int64_t T, int64_t N) {
    MomLayout L;
    L.P = N * N; L.RT = R * T; L.T = T;
    L.ntiles = (int64_t)ceil_div((size_t)L.P, MOM_TILE);
    L.rpg = (int64_t)ceil_div((size_t)L.RT, MOM_RG);
    L.ngroups = (int64_t)ceil_div((size_t)L.RT, (size_t)L.rpg);
    size_t at = 0;
    L.spart = at; at += align_up((size_t)L.ngroups * MOM_NQS * 2 * L.P * sizeof(double));
    L.rpart = at; at += align_up((size_t)L.RT * 2 * L.ntiles * MOM_NQR * sizeof(double));
    L.smean = at; at += align_up((size_t)2 * 2 * L.P * sizeof(double));
    L.tsum = at;  at += align_up((size_t)MOM_NQR * T * 2 * sizeof(double));
    L.tmean = at; at += align_up((size_t)2 * T * 2 * sizeof(double));
    L.gmean = at; at += align_up((size_t)2 * 2 * sizeof(double));
    L.total = at;
    return L;
}

template <typename TT, typename TM, typename TG, int PASS>
__global__ __launch_bounds__(MOM_THREADS) void k_moments(const TT *tv, const TM *mv, const TG *gv, int64_t RT, int64_t T,
                                                         int64_t P, int64_t ntiles, int64_t rpg, const double *smean,
                                                         const double *tmean, const double *gmean, double *spart,
                                                         double *rpart) {
    constexpr int NQS = PASS == 1 ? 2 : MOM_NQS, NQR = PASS == 1 ? 2 : MOM_NQR;
    __shared__ double red[MOM_THREADS / 64][NQR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t tile = blockIdx.x, z = blockIdx.y, rg = blockIdx.z;
    const int64_t row0 = rg * rpg, row1 = row0 + rpg < RT ? row0 + rpg : RT;
    double acc[MOM_PPT][NQS];
    double ms_t[MOM_PPT], ms_m[MOM_PPT];
    int64_t pos[MOM_PPT];
#pragma unroll
    for (int k = 0; k < MOM_PPT; ++k) {
        pos[k] = tile * MOM_TILE + (int64_t)k * MOM_THREADS + tid;
#pragma unroll
        for (int q = 0; q < NQS; ++q) acc[k][q] = 0.;
        ms_t[k] = ms_m[k] = 0.;
        if (PASS == 2 && pos[k] < P) {
            ms_t[k] = smean[(0 * 2 + z) * P + pos[k]];
            ms_m[k] = smean[(1 * 2 + z) * P + pos[k]];
        }
    }
    const double mg_t = PASS == 2 ? gmean[0 * 2 + z] : 0., mg_m = PASS == 2 ? gmean[1 * 2 + z] : 0.;
    for (int64_t row = row0; row < row1; ++row) {
        const int64_t t = row % T;
        const double mt_t = PASS == 2 ? tmean[(0 * T + t) * 2 + z] : 0., mt_m = PASS == 2 ? tmean[(1 * T + t) * 2 + z] : 0.;
        const int64_t base = (row * 2 + z) * P;
        double rs[NQR];
#pragma unroll
        for (int q = 0; q < NQR; ++q) rs[q] = 0.;
#pragma unroll
        for (int k = 0; k < MOM_PPT; ++k) {
            if (pos[k] < P) {
                const double a = (double)tv[base + pos[k]], b = (double)mv[base + pos[k]];
                if constexpr (PASS == 1) {
                    acc[k][0] += a; acc[k][1] += b;
                    rs[0] += a; rs[1] += b;
                } else {
                    const double c = (double)gv[base + pos[k]];
                    const double d = a - b, e = c - b, d2 = d * d, a2 = a * a, e2 = e * e;
                    const double sa = a - ms_t[k], sb = b - ms_m[k];
                    const double ta = a - mt_t, tb = b - mt_m, ga = a - mg_t, gb = b - mg_m;
                    acc[k][0] += d2; acc[k][1] += a2; acc[k][2] += sa * sa; acc[k][3] += sb * sb; acc[k][4] += sa * sb;
                    acc[k][5] += e2;
                    rs[0] += d2; rs[1] += a2; rs[2] += ta * ta; rs[3] += tb * tb; rs[4] += ta * tb; rs[5] += e2;
                    rs[6] += ga * ga; rs[7] += gb * gb; rs[8] += ga * gb;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQR; ++q) {
            double v = rs[q];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
            rs[q] = v;
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NQR; ++q) red[w][q] = rs[q];
        }
        __syncthreads();
        if (tid < NQR) {
            double s = 0.;
#pragma unroll
            for (int ww = 0; ww < MOM_THREADS / 64; ++ww) s += red[ww][tid];
            rpart[((row * 2 + z) * ntiles + tile) * NQR + tid] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < MOM_PPT; ++k) {
        if (pos[k] < P) {
#pragma unroll
            for (int q = 0; q < NQS; ++q) spart[((rg * NQS + q) * 2 + z) * P + pos[k]] = acc[k][q];
        }
    }
}

// spatial: out[(q*2 + z)*P + p] = scale * sum over row groups, in order
__global__ __launch_bounds__(256) void k_mom_merge_spatial(const double *spart, int64_t ngroups, int nq, int64_t P,
                                                           double scale, double *out) {
    const int64_t n = (int64_t)nq * 2 * P;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s = 0.;
        for (int64_t g = 0; g < ngroups; ++g) s += spart[g * n + i];
        out[i] = s * scale;
    }
}

// rows: tsum[(q*T + t)*2 + z] = sum over runs r, then tiles, in order
__global__ __launch_bounds__(256) void k_mom_merge_rows(const double *rpart, int64_t R, int64_t T, int64_t ntiles, int nq,
                                                        double *tsum) {
    const int64_t n = (int64_t)nq * T * 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t q = i / (T * 2), t = (i / 2) % T, z = i % 2;
        double s = 0.;
        for (int64_t r = 0; r < R; ++r)
            for (int64_t k = 0; k < ntiles; ++k) s += rpart[(((r * T + t) * 2 + z) * ntiles + k) * nq + q];
        tsum[i] = s;
    }
}

// pass 1: tmean = tsum / (R P), gmean[q*2 + z] = sum over t of tsum / (R T P)
__global__ __launch_bounds__(256) void k_mom_means(const double *tsum, int64_t R, int64_t T, int64_t P, double *tmean,
                                                   double *gmean) {
    const double nt = (double)R * (double)P, ng = nt * (double)T;
    for (int64_t i = threadIdx.x; i < 2 * T * 2; i += 256) tmean[i] = tsum[i] / nt;
    if (threadIdx.x < 4) {
        const int q = threadIdx.x >> 1, z = threadIdx.x & 1;
        double s = 0.;
        for (int64_t t = 0; t < T; ++t) s += tsum[(q * T + t) * 2 + z];
        gmean[q * 2 + z] = s / ng;
    }
}

// pass 2 outputs: temporal [6][T][2] (row quantities 0..5), global [6][2] (row quantities 0, 1, 6, 7, 8, 5 summed over t)
__global__ __launch_bounds__(256) void k_mom_out(const double *tsum, int64_t T, double *temporal, double *global) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 6 * T * 2; i += (int64_t)gridDim.x * 256)
        temporal[i] = tsum[i];
    if (blockIdx.x == 0 && threadIdx.x < 12) {
        const int q = threadIdx.x >> 1, z = threadIdx.x & 1;
        const int src[6] = {0, 1, 6, 7, 8, 5};
        double s = 0.;
        for (int64_t t = 0; t < T; ++t) s += tsum[(src[q] * T + t) * 2 + z];
        global[q * 2 + z] = s;
    }
}

template <typename TT, typename TM, typename TG>
int moments(const void *t, const void *m, const void *g, int64_t R, int64_t T, const MomLayout &L, char *work, double *out,
            hipStream_t st) {
    double *spart = (double *)(work + L.spart), *rpart = (double *)(work + L.rpart), *smean = (double *)(work + L.smean),
           *tsum = (double *)(work + L.tsum), *tmean = (double *)(work + L.tmean), *gmean = (double *)(work + L.gmean);
    const dim3 grid((unsigned)L.ntiles, 2, (unsigned)L.ngroups);
    const unsigned ms = (unsigned)std::min<size_t>(ceil_div((size_t)MOM_NQS * 2 * L.P, 256), 2048);
    const unsigned mr = (unsigned)std::min<size_t>(ceil_div((size_t)MOM_NQR * T * 2, 256), 1024);
    hipLaunchKernelGGL((k_moments<TT, TM, TG, 1>), grid, dim3(MOM_THREADS), 0, st, (const TT *)t, (const TM *)m,
                       (const TG *)g, L.RT, T, L.P, L.ntiles, L.rpg, smean, tmean, gmean, spart, rpart);
    hipLaunchKernelGGL(k_mom_merge_spatial, dim3(ms), dim3(256), 0, st, spart, L.ngroups, 2, L.P, 1. / (double)L.RT, smean);
    hipLaunchKernelGGL(k_mom_merge_rows, dim3(mr), dim3(256), 0, st, rpart, R, T, L.ntiles, 2, tsum);
    hipLaunchKernelGGL(k_mom_means, dim3(1), dim3(256), 0, st, tsum, R, T, L.P, tmean, gmean);
    hipLaunchKernelGGL((k_moments<TT, TM, TG, 2>), grid, dim3(MOM_THREADS), 0, st, (const TT *)t, (const TM *)m,
                       (const TG *)g, L.RT, T, L.P, L.ntiles, L.rpg, smean, tmean, gmean, spart, rpart);
    hipLaunchKernelGGL(k_mom_merge_spatial, dim3(ms), dim3(256), 0, st, spart, L.ngroups, MOM_NQS, L.P, 1., out);
    hipLaunchKernelGGL(k_mom_merge_rows, dim3(mr), dim3(256), 0, st, rpart, R, T, L.ntiles, MOM_NQR, tsum);
    double *temporal = out + (int64_t)MOM_NQS * 2 * L.P, *global = temporal + (int64_t)MOM_NQS * T * 2;
    hipLaunchKernelGGL(k_mom_out, dim3((unsigned)std::min<size_t>(ceil_div((size_t)12 * T, 256), 1024)), dim3(256), 0, st,
                       tsum, T, temporal, global);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

// ---- histogram ----------------------------------------------------------------------------------------------------
// view: R x (T - t0) rows of P values; row (r, t) starts at element ((r*T + t)*nlev + z)*P
struct View {
    int64_t T, nlev, P, z, t0, Tw, n;
    __device__ int64_t off(int64_t e) const {
        const int64_t row = e / P, p = e - row * P, r = row / Tw, t = t0 + (row - r * Tw);
        return ((r * T + t) * nlev + z) * P + p;
    }
};

__device__ inline double block_sum_256(double v, double *lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// mode 0: partials[b] = sum x, partials[HIST_BLOCKS + b] = non-finite count; mode 1: partials[b] = sum (x - stats[0])^2
template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void k_hist_stats(const T *x, View v, int mode, const double *stats,
                                                             double *partials) {
    __shared__ double red[HIST_THREADS];
    const double mean = mode ? stats[0] : 0.;
    double s = 0., bad = 0.;
    for (int64_t e = (int64_t)blockIdx.x * HIST_THREADS + threadIdx.x; e < v.n; e += (int64_t)gridDim.x * HIST_THREADS) {
        const double a = (double)x[v.off(e)];
        if (mode) {
            const double d = a - mean;
            s += d * d;
        } else {
            s += a;
            if (!isfinite(a)) bad += 1.;
        }
    }
    const double S = block_sum_256(s, red);
    const double B = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = S;
        if (!mode) partials[HIST_BLOCKS + blockIdx.x] = B;
    }
}

// mode 0: stats[0] = mean, stats[2] = non-finite count; mode 1: stats[1] = population std, and with no_bins (statistics
// only: no counting kernel follows to write it) stats[3] = the scale a count would have used
__global__ __launch_bounds__(256) void k_hist_stats_finish(const double *partials, int nblk, int mode, double n,
                                                           double *stats, int no_bins, int scale_std, double scale_val) {
    __shared__ double red[256];
    double s = 0., b = 0.;
    for (int i = threadIdx.x; i < nblk; i += 256) {
        s += partials[i];
        if (!mode) b += partials[HIST_BLOCKS + i];
    }
    const double S = block_sum_256(s, red);
    const double B = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        if (mode) {
            stats[1] = sqrt(S / n);
            if (no_bins) stats[3] = scale_std ? stats[1] : scale_val;
        } else {
            stats[0] = S / n;
            stats[2] = B;
        }
    }
}

// np.histogram's uniform-bin rule (numpy/lib/_histograms_impl.py, equal-width branch) on v = x / scale in float64:
// keep lo <= v <= hi; i = int(((v - lo) / (hi - lo)) * nbins); i == nbins -> nbins - 1; v < edge[i] -> i - 1;
// v >= edge[i + 1] and i != nbins - 1 -> i + 1.  Slot nbins counts non-finite x.
template <typename T>
__global__ __launch_bounds__(HIST_THREADS) void k_hist_count(const T *x, View v, const double *edges, int nbins,
                                                             const double *scale_dev, double scale_val,
                                                             uint32_t *partials) {
    extern __shared__ uint32_t hist[];
    for (int b = threadIdx.x; b <= nbins; b += HIST_THREADS) hist[b] = 0u;
    __syncthreads();
    const double scale = scale_dev ? scale_dev[1] : scale_val;
    const double lo = edges[0], hi = edges[nbins], denom = __dsub_rn(hi, lo), nb = (double)nbins;
    for (int64_t e = (int64_t)blockIdx.x * HIST_THREADS + threadIdx.x; e < v.n; e += (int64_t)gridDim.x * HIST_THREADS) {
        const double a = (double)x[v.off(e)];
        if (!isfinite(a)) {
            atomicAdd(&hist[nbins], 1u);
            continue;
        }
        const double u = __ddiv_rn(a, scale);
        if (!(u >= lo && u <= hi)) continue;
        int64_t i = (int64_t)__dmul_rn(__ddiv_rn(__dsub_rn(u, lo), denom), nb);
        if (i >= nbins) i = nbins - 1;
        if (i < 0) i = 0;
        if (u < edges[i] && i > 0) i -= 1;
        if (i != nbins - 1 && u >= edges[i + 1]) i += 1;
        atomicAdd(&hist[i], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= nbins; b += HIST_THREADS) partials[(int64_t)blockIdx.x * (nbins + 1) + b] = hist[b];
}

// counts[b] = sum over workgroups in order; stats[2] = non-finite count, stats[3] = the scale used
__global__ __launch_bounds__(256) void k_hist_count_finish(const uint32_t *partials, int nblk, int nbins,
                                                           const double *scale_dev, double scale_val, int64_t *counts,
                                                           double *stats) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b <= nbins; b += gridDim.x * 256) {
        uint64_t s = 0;
        for (int k = 0; k < nblk; ++k) s += partials[(int64_t)k * (nbins + 1) + b];
        if (b < nbins) counts[b] = (int64_t)s;
        else {
            stats[2] = (double)s;
            stats[3] = scale_dev ? scale_dev[1] : scale_val;
        }
    }
}

size_t hist_bytes(int nbins) {
    return align_up((size_t)2 * HIST_BLOCKS * sizeof(double)) + align_up((size_t)HIST_BLOCKS * (nbins + 1) * sizeof(uint32_t));
}

template <typename T>
int histogram(const void *x, const View &v, const double *edges, int nbins, int flags, double scale, char *work,
              int64_t *counts, double *stats, hipStream_t st) {
    const int nblk = (int)std::min<size_t>(ceil_div((size_t)v.n, (size_t)HIST_THREADS * HIST_ITEMS), HIST_BLOCKS);
    double *dpart = (double *)work;
    uint32_t *cpart = (uint32_t *)(work + align_up((size_t)2 * HIST_BLOCKS * sizeof(double)));
    if (flags & QGX_HIST_STATS) {
        for (int mode = 0; mode < 2; ++mode) {
            hipLaunchKernelGGL(k_hist_stats<T>, dim3(nblk), dim3(HIST_THREADS), 0, st, (const T *)x, v, mode,
                               (const double *)stats, dpart);
            hipLaunchKernelGGL(k_hist_stats_finish, dim3(1), dim3(256), 0, st, (const double *)dpart, nblk, mode,
                               (double)v.n, stats, (int)(nbins == 0), (int)((flags & QGX_HIST_SCALE_STD) != 0), scale);
        }
    }
    if (nbins > 0) {
        const double *sdev = (flags & QGX_HIST_SCALE_STD) ? stats : nullptr;
        hipLaunchKernelGGL(k_hist_count<T>, dim3(nblk), dim3(HIST_THREADS), (nbins + 1) * sizeof(uint32_t), st,
                           (const T *)x, v, edges, nbins, sdev, scale, cpart);
        hipLaunchKernelGGL(k_hist_count_finish, dim3((unsigned)ceil_div((size_t)nbins + 1, 256)), dim3(256), 0, st,
                           (const uint32_t *)cpart, nblk, nbins, sdev, scale, counts, stats);
    }
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;

bool fits(int64_t a, int64_t b, int64_t c, int64_t d) {      // a*b*c*d <= MAX_ELEMS for positive a..d
    return a <= MAX_ELEMS && b <= MAX_ELEMS / a && c <= MAX_ELEMS / (a * b) && d <= MAX_ELEMS / (a * b * c);
}

}  // namespace
}  // namespace qgx

using namespace qgx;

extern "C" int qgx_offline_workspace(int which, int64_t R, int64_t T, int64_t N, int nbins, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_offline_workspace: null argument");
    if (which == QGX_WORK_SPECTRA) {
        QGX_REQUIRE(N >= 2 && N % 2 == 0 && N <= 65536, "qgx_offline_workspace: N must be even, in [2, 65536] (got %lld)",
                    (long long)N);
        *bytes = (size_t)SPEC_G * 2 * NPL * (size_t)N * (size_t)(N / 2 + 1) * sizeof(double);
        return QGX_OK;
    }
    if (which == QGX_WORK_MOMENTS) {
        QGX_REQUIRE(R > 0 && T > 0 && N > 0 && fits(R, T, 2, N) && fits(R * T, 2, N, N),
                    "qgx_offline_workspace: moments need R, T, N >= 1 within 2^40 elements");
        *bytes = mom_layout(R, T, N).total;
        return QGX_OK;
    }
    if (which == QGX_WORK_HISTOGRAM) {
        QGX_REQUIRE(nbins >= 0 && nbins <= QGX_HIST_MAX_BINS, "qgx_offline_workspace: nbins must be in [0, %d] (got %d)",
                    QGX_HIST_MAX_BINS, nbins);
        *bytes = hist_bytes(nbins);
        return QGX_OK;
    }
    qgx::set_error("qgx_offline_workspace: unknown work kind %d", which);
    return QGX_ERR_INVALID;
}

extern "C" int qgx_offline_spectra(const double *th_dev, const double *gh_dev, const double *mh_dev,
                                   const double *psih_dev, int64_t S, int N, int64_t s0, int64_t T, int64_t t0,
                                   int accumulate, double *acc_dev, void *stream) {
    QGX_REQUIRE(th_dev && gh_dev && mh_dev && acc_dev, "qgx_offline_spectra: null argument");
    QGX_REQUIRE(N >= 2 && N % 2 == 0 && N <= 65536, "qgx_offline_spectra: N must be even, in [2, 65536] (got %d)", N);
    QGX_REQUIRE(S > 0 && T > 0 && s0 >= 0 && t0 >= 0 && S <= MAX_ELEMS && s0 <= MAX_ELEMS && T <= MAX_ELEMS &&
                t0 <= MAX_ELEMS, "qgx_offline_spectra: empty or negative snapshot range");
    QGX_REQUIRE(fits(S, 2, N, N / 2 + 1), "qgx_offline_spectra: view too large");
    QGX_REQUIRE(accumulate == 0 || accumulate == 1, "qgx_offline_spectra: accumulate must be 0 or 1 (got %d)", accumulate);
    const int64_t P = (int64_t)N * (N / 2 + 1);
    const dim3 grid((unsigned)ceil_div((size_t)P, SPEC_THREADS), SPEC_G);
    const double M2 = (double)N * (double)N;
    hipStream_t st = (hipStream_t)stream;
    if (psih_dev)
        hipLaunchKernelGGL(k_offline_spectra<true>, grid, dim3(SPEC_THREADS), 0, st, (const double2 *)th_dev,
                           (const double2 *)gh_dev, (const double2 *)mh_dev, (const double2 *)psih_dev, S, P, s0, T, t0,
                           M2, accumulate, acc_dev);
    else
        hipLaunchKernelGGL(k_offline_spectra<false>, grid, dim3(SPEC_THREADS), 0, st, (const double2 *)th_dev,
                           (const double2 *)gh_dev, (const double2 *)mh_dev, (const double2 *)nullptr, S, P, s0, T, t0,
                           M2, accumulate, acc_dev);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

extern "C" int qgx_offline_spectra_finish(const double *acc_dev, int N, double *out_dev, void *stream) {
    QGX_REQUIRE(acc_dev && out_dev, "qgx_offline_spectra_finish: null argument");
    QGX_REQUIRE(N >= 2 && N % 2 == 0 && N <= 65536, "qgx_offline_spectra_finish: N must be even, in [2, 65536] (got %d)", N);
    const int64_t n = (int64_t)2 * NPL * N * (N / 2 + 1);
    hipLaunchKernelGGL(k_offline_spectra_finish, dim3((unsigned)std::min<size_t>(ceil_div((size_t)n, 256), 4096)),
                       dim3(256), 0, (hipStream_t)stream, acc_dev, n, out_dev);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

template <typename TT, typename TM>
static int moments_g(int dg, const void *t, const void *m, const void *g, int64_t R, int64_t T, const MomLayout &L,
                     char *w, double *o, hipStream_t st) {
    return dg ? moments<TT, TM, double>(t, m, g, R, T, L, w, o, st) : moments<TT, TM, float>(t, m, g, R, T, L, w, o, st);
}

extern "C" int qgx_offline_moments(const void *t_dev, const void *m_dev, const void *g_dev, int dtypes, int64_t R,
                                   int64_t T, int N, void *work_dev, size_t work_bytes, double *out_dev, void *stream) {
    QGX_REQUIRE(dtypes >= 0 && dtypes <= 7, "qgx_offline_moments: dtypes must be a 3-bit mask (got %d)", dtypes);
    size_t need = 0;
    const int rc = qgx_offline_workspace(QGX_WORK_MOMENTS, R, T, N, 0, &need);
    if (rc) return rc;
    QGX_REQUIRE(t_dev && m_dev && g_dev && work_dev && out_dev, "qgx_offline_moments: null argument");
    QGX_REQUIRE(work_bytes >= need, "qgx_offline_moments: work space of %zu bytes, %zu needed", work_bytes, need);
    const MomLayout L = mom_layout(R, T, N);
    char *w = (char *)work_dev;
    hipStream_t st = (hipStream_t)stream;
    const int dt = dtypes & 1, dm = (dtypes >> 1) & 1, dg = (dtypes >> 2) & 1;
    if (dt && dm) return moments_g<double, double>(dg, t_dev, m_dev, g_dev, R, T, L, w, out_dev, st);
    if (dt) return moments_g<double, float>(dg, t_dev, m_dev, g_dev, R, T, L, w, out_dev, st);
    if (dm) return moments_g<float, double>(dg, t_dev, m_dev, g_dev, R, T, L, w, out_dev, st);
    return moments_g<float, float>(dg, t_dev, m_dev, g_dev, R, T, L, w, out_dev, st);
}

extern "C" int qgx_histogram(const void *x_dev, int is_double, int64_t R, int64_t T, int64_t nlev, int64_t P, int64_t z,
                             int64_t t0, const double *edges_dev, int nbins, int flags, double scale, void *work_dev,
                             size_t work_bytes, int64_t *counts_dev, double *stats_dev, void *stream) {
    QGX_REQUIRE(is_double == 0 || is_double == 1, "qgx_histogram: is_double must be 0 or 1 (got %d)", is_double);
    QGX_REQUIRE(flags >= 0 && flags <= 3 && (flags != QGX_HIST_SCALE_STD), "qgx_histogram: bad flags %d", flags);
    QGX_REQUIRE(nbins >= 0 && nbins <= QGX_HIST_MAX_BINS && (nbins > 0 || (flags & QGX_HIST_STATS)),
                "qgx_histogram: nbins must be in [1, %d], or 0 with QGX_HIST_STATS (got %d)", QGX_HIST_MAX_BINS, nbins);
    QGX_REQUIRE(R > 0 && T > 0 && nlev > 0 && P > 0 && z >= 0 && z < nlev && t0 >= 0 && t0 < T,
                "qgx_histogram: empty or negative view");
    QGX_REQUIRE(fits(R, T, nlev, P), "qgx_histogram: view too large");
    QGX_REQUIRE(x_dev && work_dev && stats_dev && (nbins == 0 || (edges_dev && counts_dev)),
                "qgx_histogram: null argument");
    QGX_REQUIRE(work_bytes >= hist_bytes(nbins), "qgx_histogram: work space of %zu bytes, %zu needed", work_bytes,
                hist_bytes(nbins));
    View v;
    v.T = T; v.nlev = nlev; v.P = P; v.z = z; v.t0 = t0; v.Tw = T - t0; v.n = R * v.Tw * P;
    hipStream_t st = (hipStream_t)stream;
    if (is_double)
        return histogram<double>(x_dev, v, edges_dev, nbins, flags, scale, (char *)work_dev, counts_dev, stats_dev, st);
    return histogram<float>(x_dev, v, edges_dev, nbins, flags, scale, (char *)work_dev, counts_dev, stats_dev, st);
}
