// The circular convolution of the DeepInversion U-Net's training and its two gradients (include/qgx_uconv_train.h): Conv2d(cin,
// cout, k, padding=k/2, padding_mode='circular'), k 1 or 3, any grid 2 ... 128, up to 512 -> 1024 channels, on the engine's NHWC
// layout.  All three are implicit GEMMs on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32) after dconv_train.hip's pattern,
// stateless, on the caller's stream.
//
//   forward          C[m][n] = sum_k A[m][k] W[n][k] + bias[n]: m a pixel (b, y, x), n an output channel, k = (tap, input channel),
//                    K = k^2 cin8.  A is gathered from x as it is staged (pixel (y + ty - P, x + tx - P) mod N); W is the weights
//                    repacked by k_upack into rows [co][tap][ci8] in the workspace (they change every step).
//   backward_data    the same kernel over dy with k_upack's flipped, transposed rows [ci][k^2 - 1 - tap][co8]: tap t' of the
//                    gather reads (y + t'y - P) = (y - ky + P) for ky = k - 1 - t'y.
//   backward_weight  C[co][n] = sum over pixels p of dy[p][co] x[p + tap(n)][ci(n)]: the (tap, channel) pairs n = tap cin + ci are
//                    dealt to the tile's columns; M = cout, N = k^2 cin, K = B N^2.  K is cut into units of 32 pixels and the units
//                    into S shares, a fixed function of the shape (uwgrad_plan); a workgroup walks its share in order and stores
//                    its tile into its own slice of the workspace, and k_uwgrad_reduce adds the slices in a fixed order.  With
//                    S = 1 (the bottom of the U-Net: a 512 x 4608 dw over 16 B pixels) the tile goes straight to dw and no second
//                    kernel runs.  The workgroups of the first column tile also sum their share of dy into db.  No atomics.
//
// One workgroup of four waves owns a 64 x 64 tile of C, wave w the quadrant (w & 1, w >> 1); a chunk of 32 k is staged k-major in
// LDS with a row stride of 65 floats (dconv_train.hip: the transposing ds_write_b32 and the MFMA operands' ds_read_b32 are free
// of bank conflicts within a 32-lane half).  The next chunk's global loads are issued before the current chunk's MFMAs.
#include "common.hpp"

namespace qgx {

#include "conv_types.hpp"

constexpr int UT = 64;                // tile edge of C
constexpr int UK = 32;                // k per staged chunk
constexpr int US = UT + 1;            // floats per staged k row
static int u_up(int v, int m) { return (v + m - 1) / m * m; }
static int u_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// mode 0 (forward):       wp[co][tap cin8 + ci] = w[co][ci][tap], zero for ci >= cin                     cout rows of k^2 cin8
// mode 1 (data gradient): wp[ci][tap cout8 + co] = w[co][ci][k^2 - 1 - tap], zero for co >= cout         cin rows of k^2 cout8
__global__ __launch_bounds__(256) void k_upack(const float *w, float *wp, int cin, int cout, int cin8, int cout8, int kk, int mode,
                                               int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float v = 0.f;
    if (mode == 0) {
        const int K = kk * cin8;
        const int co = idx / K, k = idx - co * K, tap = k / cin8, ci = k - tap * cin8;
        if (ci < cin) v = w[((size_t)co * cin + ci) * kk + tap];
    } else {
        const int K = kk * cout8;
        const int ci = idx / K, k = idx - ci * K, tap = k / cout8, co = k - tap * cout8;
        if (co < cout) v = w[((size_t)co * cin + ci) * kk + (kk - 1 - tap)];
    }
    wp[idx] = v;
}

// ---- forward and data gradient ---------------------------------------------------------------
struct UconvArgs {
    const float *a;      // the gathered tensor (B, N, N, ca8): x forward, dy data gradient
    const float *wp;     // k_upack's rows [cn][K]
    const float *bias;   // (cn) or NULL
    float *out;          // (B, N, N, cn8)
    int M;               // B N^2: the rows of C
    int N, ca8, K, cn, cn8, ks;
};

__global__ __launch_bounds__(256) void k_uconv_train(UconvArgs g) {
    __shared__ float As[UK * US], Bs[UK * US];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * UT, n0 = blockIdx.y * UT;
    const int kq = t & 7, lr = t >> 3;          // this thread stages the k quad kq of the tile rows lr and lr + 32
    const int P = g.ks >> 1;
    int pb[2], pi[2], pj[2];
    bool pm[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int m = m0 + lr + 32 * p;
        pm[p] = m < g.M;
        const int mm = pm[p] ? m : 0;
        pb[p] = mm / (g.N * g.N);
        const int rem = mm - pb[p] * g.N * g.N;
        pi[p] = rem / g.N;
        pj[p] = rem - pi[p] * g.N;
    }
    float4 va[2], vb[2];
    auto load = [&](int k0) {
        const int k = k0 + kq * 4;              // K is a multiple of 8: a quad is inside K or beyond it, and inside one tap
        const bool kin = k < g.K;
        const int tap = kin ? k / g.ca8 : 0, c = kin ? k - tap * g.ca8 : 0;
        const int ty = tap / g.ks, tx = tap - ty * g.ks;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int yy = pi[p] + ty - P, xx = pj[p] + tx - P;       // -1 ... N: one wrap each way (N >= 2)
            yy += yy < 0 ? g.N : 0; yy -= yy >= g.N ? g.N : 0;
            xx += xx < 0 ? g.N : 0; xx -= xx >= g.N ? g.N : 0;
            va[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kin && pm[p]) va[p] = *reinterpret_cast<const float4 *>(&g.a[(((size_t)pb[p] * g.N + yy) * g.N + xx) * g.ca8 + c]);
            const int n = n0 + lr + 32 * p;
            vb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kin && n < g.cn) vb[p] = *reinterpret_cast<const float4 *>(&g.wp[(size_t)n * g.K + k]);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ao = (wave & 1) * 32 + li, bo = (wave >> 1) * 32 + li;

    load(0);
    for (int k0 = 0; k0 < g.K; k0 += UK) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = lr + 32 * p;
            As[(kq * 4 + 0) * US + r] = va[p].x; As[(kq * 4 + 1) * US + r] = va[p].y;
            As[(kq * 4 + 2) * US + r] = va[p].z; As[(kq * 4 + 3) * US + r] = va[p].w;
            Bs[(kq * 4 + 0) * US + r] = vb[p].x; Bs[(kq * 4 + 1) * US + r] = vb[p].y;
            Bs[(kq * 4 + 2) * US + r] = vb[p].z; Bs[(kq * 4 + 3) * US + r] = vb[p].w;
        }
        __syncthreads();
        if (k0 + UK < g.K) load(k0 + UK);
#pragma unroll
        for (int kk = 0; kk < UK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * kk + h) * US + ao], Bs[(2 * kk + h) * US + bo], acc, 0, 0, 0);
    }
    // acc[r]: row (r & 3) + 8 (r >> 2) + 4 h of the wave's quadrant, column li
    const int n = n0 + bo;
    if (n >= g.cn8) return;
    const float bv = (g.bias && n < g.cn) ? g.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < g.M) g.out[(size_t)m * g.cn8 + n] = acc[r] + bv;
    }
}

// ---- weight gradient -------------------------------------------------------------------------
struct UwgradArgs {
    const float *x, *dy;     // NHWC (B, N, N, cin8), (B, N, N, cout8)
    float *part;             // [share][tile][64 co][64 (tap, ci)], S > 1
    float *dbpart;           // [share][cot_n 64], S > 1 and db asked for
    float *dw, *db;          // the results: written here with S = 1 (db may be NULL)
    int P;                   // B N^2 pixels: the GEMM's K
    int N, cin, cin8, cout, cout8, ks, U, ups, S, nt_n, cot_n;
};

__global__ __launch_bounds__(256) void k_uwgrad(UwgradArgs g) {
    __shared__ float As[UK * US], Bs[UK * US];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, share = blockIdx.y;
    const int cot = tile / g.nt_n, nt = tile - cot * g.nt_n;
    const int kk = g.ks * g.ks, pad = g.ks >> 1;
    // A = dy: this thread stages the channel quad (t & 15) of the chunk's pixels (t >> 4) and (t >> 4) + 16
    const int aq = (t & 15) * 4, ap = t >> 4;
    const bool alive = cot * UT + aq < g.cout8;
    // B = x at the column's tap: this thread stages column t & 63 of the chunk's pixels (t >> 6) + 4 j
    const int bc = t & 63, bp = t >> 6;
    const int n = nt * UT + bc;
    const bool blive = n < kk * g.cin;
    const int tap = blive ? n / g.cin : 0, ci = blive ? n - tap * g.cin : 0;
    const int ky = tap / g.ks - pad, kx = tap - (tap / g.ks) * g.ks - pad;
    const bool sum_db = g.db && nt == 0 && t < UT;

    // The unit's 32 pixels are decomposed once, by 32 lanes, into a table the 64 columns share: the image's first pixel and
    // (y << 8 | x); -1 for a pixel beyond P.  Two tables: unit u + 1's is written while unit u's is still read.
    __shared__ int tbase[2][UK], tyx[2][UK];
    auto table = [&](int u) {
        if (t < UK) {
            const int p = u * UK + t;
            int base = 0, yx = -1;
            if (p < g.P) {
                const int b = p / (g.N * g.N), rem = p - b * g.N * g.N, i = rem / g.N;
                base = b * g.N * g.N;
                yx = (i << 8) | (rem - i * g.N);
            }
            tbase[u & 1][t] = base;
            tyx[u & 1][t] = yx;
        }
    };
    float4 va[2];
    float vb[8];
    auto load = [&](int u) {
        const int p0 = u * UK;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = p0 + ap + 16 * j;
            va[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (alive && p < g.P) va[j] = *reinterpret_cast<const float4 *>(&g.dy[(size_t)p * g.cout8 + cot * UT + aq]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pl = bp + 4 * j;
            const int base = tbase[u & 1][pl], yx = tyx[u & 1][pl];
            int yy = (yx >> 8) + ky, xx = (yx & 0xff) + kx;
            yy += yy < 0 ? g.N : 0; yy -= yy >= g.N ? g.N : 0;
            xx += xx < 0 ? g.N : 0; xx -= xx >= g.N ? g.N : 0;
            vb[j] = 0.f;
            if (blive && yx >= 0) vb[j] = g.x[(size_t)(base + yy * g.N + xx) * g.cin8 + ci];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float dbacc = 0.f;
    const int ao = (wave & 1) * 32 + li, bo = (wave >> 1) * 32 + li;

    const int u0 = share * g.ups, u1 = u0 + g.ups < g.U ? u0 + g.ups : g.U;
    table(u0);
    __syncthreads();
    load(u0);
    for (int u = u0; u < u1; ++u) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float *o = &As[(ap + 16 * j) * US + aq];
            o[0] = va[j].x; o[1] = va[j].y; o[2] = va[j].z; o[3] = va[j].w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[(bp + 4 * j) * US + bc] = vb[j];
        if (u + 1 < u1) table(u + 1);
        __syncthreads();
        if (u + 1 < u1) load(u + 1);
#pragma unroll
        for (int q = 0; q < UK / 2; ++q)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * q + h) * US + ao], Bs[(2 * q + h) * US + bo], acc, 0, 0, 0);
        if (sum_db) {
#pragma unroll 8
            for (int p = 0; p < UK; ++p) dbacc += As[p * US + t];      // the unit's pixels in order (beyond P: zeros)
        }
    }
    if (g.S > 1) {
        float *o = g.part + ((size_t)share * gridDim.x + tile) * (UT * UT);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[((wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * UT + bo] = acc[r];
        if (sum_db) g.dbpart[(size_t)share * g.cot_n * UT + cot * UT + t] = dbacc;
        return;
    }
    // one share: the tile is the result
    const int nn = nt * UT + bo;
    if (nn < kk * g.cin) {
        const int tp = nn / g.cin, c = nn - tp * g.cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cot * UT + (wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (co < g.cout) g.dw[((size_t)co * g.cin + c) * kk + tp] = acc[r];
        }
    }
    if (sum_db && cot * UT + t < g.cout) g.db[cot * UT + t] = dbacc;
}

// dw[co][ci][tap] = the shares' slices added in a fixed order (dconv_train.hip's k_dwgrad_reduce): a workgroup of URED_WAVES
// waves owns 64 consecutive elements of a slice (one row of a tile); wave q adds the shares q, q + URED_WAVES, ... in order, then
// the waves' sums are added in order.  The workgroups after the slice's do the same for 64 channels of db.
constexpr int URED_WAVES = 8;
__global__ __launch_bounds__(64 * URED_WAVES) void k_uwgrad_reduce(const float *part, const float *dbpart, float *dw, float *db,
                                                                  int S, int nt_n, int cot_n, int cin, int cout, int kk, int slice) {
    __shared__ float red[URED_WAVES][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool bias = (int)blockIdx.x >= slice / 64;
    const int idx = (bias ? (int)blockIdx.x - slice / 64 : (int)blockIdx.x) * 64 + e;
    const float *src = bias ? dbpart : part;
    const size_t stride = bias ? (size_t)cot_n * UT : (size_t)slice;
    float s = 0.f;
#pragma unroll 4
    for (int sh = q; sh < S; sh += URED_WAVES) s += src[(size_t)sh * stride + idx];
    red[q][e] = s;
    __syncthreads();
    if (q) return;
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < URED_WAVES; ++k) v += red[k][e];
    if (bias) {
        if (idx < cout) db[idx] = v;
        return;
    }
    const int col = idx & 63, row = (idx >> 6) & 63, tile = idx >> 12;
    const int cot = tile / nt_n, nt = tile - cot * nt_n;
    const int co = cot * UT + row, n = nt * UT + col;
    if (co >= cout || n >= kk * cin) return;
    const int tap = n / cin, ci = n - tap * cin;
    dw[((size_t)co * cin + ci) * kk + tap] = v;
}

// ---- host side -------------------------------------------------------------------------------
// The weight gradient's partition, a function of (B, N, cin, cout, k) alone: U units of 32 pixels go to S shares of `ups`
// consecutive units (the last share may hold fewer), S chosen so that tiles x shares is about 512 workgroups.
struct UwgradPlan { int P, U, ups, S, cot_n, nt_n, tiles; };
static UwgradPlan uwgrad_plan(int64_t B, int N, int cin, int cout, int k) {
    UwgradPlan p = {};
    p.P = (int)(B * N * N);
    p.U = u_cdiv(p.P, UK);
    p.cot_n = u_cdiv(cout, UT);
    p.nt_n = u_cdiv(k * k * cin, UT);
    p.tiles = p.cot_n * p.nt_n;
    int want = u_cdiv(512, p.tiles);
    if (want > p.U) want = p.U;
    p.ups = u_cdiv(p.U, want);
    p.S = u_cdiv(p.U, p.ups);
    return p;
}

struct UworkLayout { size_t w, part, dbpart, floats; };
static UworkLayout uwork_layout(int64_t B, int N, int cin, int cout, int k) {
    const UwgradPlan p = uwgrad_plan(B, N, cin, cout, k);
    auto al = [](size_t n) { return (n + 63) / 64 * 64; };
    const size_t a = (size_t)cout * k * k * u_up(cin, 8), b = (size_t)cin * k * k * u_up(cout, 8);
    UworkLayout L;
    L.w = 0;
    L.part = al(a > b ? a : b);
    L.dbpart = L.part + (p.S > 1 ? al((size_t)p.S * p.tiles * UT * UT) : 0);
    L.floats = L.dbpart + (p.S > 1 ? al((size_t)p.S * p.cot_n * UT) : 0);
    return L;
}

static int uconv_shape_check(const char *what, int64_t B, int N, int cin, int cout, int k) {
    QGX_REQUIRE(N >= 2 && N <= 128, "%s: N = %d, expected 2 ... 128", what, N);
    QGX_REQUIRE(k == 1 || k == 3, "%s: k = %d, expected 1 or 3", what, k);
    QGX_REQUIRE(cin >= 1 && cin <= 512, "%s: cin = %d, expected 1 ... 512", what, cin);
    QGX_REQUIRE(cout >= 1 && cout <= 1024, "%s: cout = %d, expected 1 ... 1024", what, cout);
    QGX_REQUIRE(B >= 1 && B <= ((int64_t)1 << 29) / (N * N), "%s: B = %lld, expected 1 ... 2^29 / N^2", what, (long long)B);
    return QGX_OK;
}
static bool u_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define UCONV_PTR(what, p)                                                                                 \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(u_aligned16(p), "%s: " #p " is not 16-byte aligned", what);                            \
    } while (0)
static int uconv_work_check(const char *what, int64_t B, int N, int cin, int cout, int k, const void *work_dev, size_t work_bytes) {
    QGX_REQUIRE(work_dev, "%s: work_dev is NULL", what);
    QGX_REQUIRE(u_aligned16(work_dev), "%s: work_dev is not 16-byte aligned", what);
    const size_t need = uwork_layout(B, N, cin, cout, k).floats * sizeof(float);
    QGX_REQUIRE(work_bytes >= need, "%s: work_bytes = %zu, qgx_uconv2d_workspace gives %zu", what, work_bytes, need);
    return QGX_OK;
}

// pack the weights for `dgrad`, then the GEMM: gathered tensor a -> out
static int uconv_run(const float *a, const float *w, const float *bias, float *out, int B, int N, int cin, int cout, int k, int dgrad,
                     float *ws, hipStream_t st) {
    const int cin8 = u_up(cin, 8), cout8 = u_up(cout, 8), kk = k * k;
    const int total = dgrad ? cin * kk * cout8 : cout * kk * cin8;
    hipLaunchKernelGGL(k_upack, dim3((total + 255) / 256), dim3(256), 0, st, w, ws, cin, cout, cin8, cout8, kk, dgrad, total);
    QGX_HIP(hipGetLastError());
    UconvArgs g = {};
    g.a = a; g.wp = ws; g.bias = bias; g.out = out;
    g.M = B * N * N; g.N = N; g.ks = k;
    if (dgrad) { g.ca8 = cout8; g.K = kk * cout8; g.cn = cin; g.cn8 = cin8; }
    else { g.ca8 = cin8; g.K = kk * cin8; g.cn = cout; g.cn8 = cout8; }
    hipLaunchKernelGGL(k_uconv_train, dim3(u_cdiv(g.M, UT), u_cdiv(g.cn8, UT)), dim3(256), 0, st, g);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_uconv2d_workspace(int64_t B, int N, int cin, int cout, int k, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_uconv2d_workspace: bytes is NULL");
    if (const int rc = uconv_shape_check("qgx_uconv2d_workspace", B, N, cin, cout, k)) return rc;
    *bytes = uwork_layout(B, N, cin, cout, k).floats * sizeof(float);
    return QGX_OK;
}

int qgx_uconv2d_forward(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t B, int N, int cin,
                        int cout, int k, void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_uconv2d_forward";
    if (const int rc = uconv_shape_check(what, B, N, cin, cout, k)) return rc;
    UCONV_PTR(what, x_dev); UCONV_PTR(what, w_dev); UCONV_PTR(what, y_dev);
    QGX_REQUIRE(u_aligned16(bias_dev), "%s: bias_dev is not 16-byte aligned", what);
    if (const int rc = uconv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    return uconv_run(x_dev, w_dev, bias_dev, y_dev, (int)B, N, cin, cout, k, 0, (float *)work_dev, (hipStream_t)stream);
}

int qgx_uconv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout, int k,
                              void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_uconv2d_backward_data";
    if (const int rc = uconv_shape_check(what, B, N, cin, cout, k)) return rc;
    UCONV_PTR(what, dy_dev); UCONV_PTR(what, w_dev); UCONV_PTR(what, dx_dev);
    if (const int rc = uconv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    return uconv_run(dy_dev, w_dev, nullptr, dx_dev, (int)B, N, cin, cout, k, 1, (float *)work_dev, (hipStream_t)stream);
}

int qgx_uconv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, float *db_dev, int64_t B, int N, int cin,
                                int cout, int k, void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_uconv2d_backward_weight";
    if (const int rc = uconv_shape_check(what, B, N, cin, cout, k)) return rc;
    UCONV_PTR(what, x_dev); UCONV_PTR(what, dy_dev); UCONV_PTR(what, dw_dev);
    QGX_REQUIRE(u_aligned16(db_dev), "%s: db_dev is not 16-byte aligned", what);
    if (const int rc = uconv_work_check(what, B, N, cin, cout, k, work_dev, work_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const UwgradPlan p = uwgrad_plan(B, N, cin, cout, k);
    const UworkLayout L = uwork_layout(B, N, cin, cout, k);
    float *ws = (float *)work_dev;
    UwgradArgs g = {};
    g.x = x_dev; g.dy = dy_dev; g.part = ws + L.part; g.dbpart = ws + L.dbpart; g.dw = dw_dev; g.db = db_dev;
    g.P = p.P; g.N = N; g.cin = cin; g.cin8 = u_up(cin, 8); g.cout = cout; g.cout8 = u_up(cout, 8); g.ks = k;
    g.U = p.U; g.ups = p.ups; g.S = p.S; g.nt_n = p.nt_n; g.cot_n = p.cot_n;
    hipLaunchKernelGGL(k_uwgrad, dim3(p.tiles, p.S), dim3(256), 0, st, g);
    QGX_HIP(hipGetLastError());
    if (p.S == 1) return QGX_OK;
    const int slice = p.tiles * UT * UT;
    hipLaunchKernelGGL(k_uwgrad_reduce, dim3(slice / 64 + (db_dev ? p.cot_n : 0)), dim3(64 * URED_WAVES), 0, st,
                       (const float *)g.part, (const float *)g.dbpart, dw_dev, db_dev, p.S, p.nt_n, p.cot_n, cin, cout, k * k, slice);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // extern "C"
