// The stride-2 convolution of a DCGAN discriminator and its two gradients (include/qgx_dconv_train.h): Conv2d(cin, cout, 4,
// stride=2, padding=1, bias=False) with zero padding on the engine's NHWC layout.  All three are implicit GEMMs on the exact-f32
// matrix cores (v_mfma_f32_32x32x2_f32), stateless, on the caller's stream; No = N / 2 below.
//
//   forward          C[m][n] = sum_k A[m][k] W[n][k]: m an output pixel (b, i, j), n an output channel, k = (tap, input channel),
//                    K = 16 cin8.  A is gathered from x as it is staged (pixel (2i - 1 + ky, 2j - 1 + kx), zero outside the
//                    image); W is the weights repacked by k_dpack into rows [co][tap][ci8] in the workspace.
//   backward_data    four parity classes (py, px), one grid.z each: row 2i' + py of dx receives ky = 1 + 2 ty from output row
//                    i' - ty (py = 0) or ky = 2 - 2 ty from output row i' + ty (py = 1), ty in {0, 1}, and the same along x.
//                    Per class the same kernel with m = (b, i', j'), n an input channel, k = (ty, tx, output channel),
//                    K = 4 cout8, A gathered from dy and W = k_dpack's rows [class][ci][t][co8].  No zero-stuffed dy: a class
//                    multiplies only the four taps that reach it.
//   backward_weight  C[co][n] = sum over pixels of dy[p][co] x[p's pixel + tap(n)][ci(n)]: the (tap, channel) pairs n = tap cin +
//                    ci are dealt to the tile's columns, so that a first layer of 6 channels fills its 64-column tiles; M =
//                    cout, N = 16 cin, K = B No^2.  K is cut into units of 32 pixels and the units into S shares, a fixed
//                    function of the shape (dwgrad_plan); a workgroup walks its share in order and stores its tile into its own
//                    slice of the workspace; k_dwgrad_reduce adds the slices in a fixed order.  No atomics.  A unit's pixels are
//                    decomposed into (image, row, column) once, one unit ahead, into a table in LDS the 64 columns share.
//
// One workgroup of four waves owns a 64 x 64 tile of C, wave w the quadrant (w & 1, w >> 1); a chunk of 32 k is staged k-major in
// LDS with a row stride of 65 floats, which makes the transposing ds_write_b32 of the gather and the ds_read_b32 of the MFMA
// operands (lane l reads row 2 kk + (l >> 5), column l & 31) free of bank conflicts within a 32-lane half.  The next chunk's
// global loads are issued before the current chunk's MFMAs.
#include "common.hpp"

namespace qgx {

#include "conv_types.hpp"

constexpr int DT = 64;                // tile edge of C
constexpr int DK = 32;                // k per staged chunk
constexpr int DS = DT + 1;            // floats per staged k row
static int d_up(int v, int m) { return (v + m - 1) / m * m; }
static int d_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// mode 0 (forward):       wp[co][tap cin8 + ci] = w[co][ci][tap], zero for ci >= cin                      cout rows of 16 cin8
// mode 1 (data gradient): wp[cls][ci][t cout8 + co] = w[co][ci][ky(py, ty)][kx(px, tx)], zero for co >= cout   4 cin rows of 4 cout8
__global__ __launch_bounds__(256) void k_dpack(const float *w, float *wp, int cin, int cout, int cin8, int cout8, int mode, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    float v = 0.f;
    if (mode == 0) {
        const int K = 16 * cin8;
        const int co = idx / K, k = idx - co * K, tap = k / cin8, ci = k - tap * cin8;
        if (ci < cin) v = w[((size_t)co * cin + ci) * 16 + tap];
    } else {
        const int K = 4 * cout8;
        const int row = idx / K, k = idx - row * K, t = k / cout8, co = k - t * cout8;
        const int cls = row / cin, ci = row - cls * cin;
        const int py = cls >> 1, px = cls & 1, ty = t >> 1, tx = t & 1;
        const int ky = py ? 2 - 2 * ty : 1 + 2 * ty, kx = px ? 2 - 2 * tx : 1 + 2 * tx;
        if (co < cout) v = w[((size_t)co * cin + ci) * 16 + ky * 4 + kx];
    }
    wp[idx] = v;
}

// ---- forward and data gradient ---------------------------------------------------------------
struct DconvArgs {
    const float *a;      // the gathered tensor: x (B, N, N, ca8) forward, dy (B, No, No, ca8) data gradient
    const float *wp;     // k_dpack's rows
    float *out;          // y (B, No, No, cn8) forward, dx (B, N, N, cn8) data gradient
    int M;               // B No^2: the rows of C (per class)
    int N, No, ca8, K, cn, cn8, dgrad;
};

__global__ __launch_bounds__(256) void k_dconv(DconvArgs g) {
    __shared__ float As[DK * DS], Bs[DK * DS];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int m0 = blockIdx.x * DT, n0 = blockIdx.y * DT;
    const int kq = t & 7, lr = t >> 3;          // this thread stages the k quad kq of the tile rows lr and lr + 32
    const int lim = g.dgrad ? g.No : g.N;       // the gathered tensor's grid
    int pb[2], pi[2], pj[2];
    bool pm[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int m = m0 + lr + 32 * p;
        pm[p] = m < g.M;
        const int mm = pm[p] ? m : 0;
        pb[p] = mm / (g.No * g.No);
        const int rem = mm - pb[p] * g.No * g.No;
        pi[p] = rem / g.No;
        pj[p] = rem - pi[p] * g.No;
    }
    float4 va[2], vb[2];
    auto load = [&](int k0) {
        const int k = k0 + kq * 4;
        const int tap = k / g.ca8, c = k - tap * g.ca8;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int yy, xx;
            if (!g.dgrad) {
                yy = 2 * pi[p] - 1 + (tap >> 2);
                xx = 2 * pj[p] - 1 + (tap & 3);
            } else {
                const int ty = tap >> 1, tx = tap & 1;
                yy = pi[p] + (py ? ty : -ty);
                xx = pj[p] + (px ? tx : -tx);
            }
            va[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pm[p] && (unsigned)yy < (unsigned)lim && (unsigned)xx < (unsigned)lim)
                va[p] = *reinterpret_cast<const float4 *>(&g.a[(((size_t)pb[p] * lim + yy) * lim + xx) * g.ca8 + c]);
            const int n = n0 + lr + 32 * p;
            vb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < g.cn) vb[p] = *reinterpret_cast<const float4 *>(&g.wp[((size_t)cls * g.cn + n) * g.K + k]);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ao = (wave & 1) * 32 + li, bo = (wave >> 1) * 32 + li;

    load(0);
    for (int k0 = 0; k0 < g.K; k0 += DK) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = lr + 32 * p;
            As[(kq * 4 + 0) * DS + r] = va[p].x; As[(kq * 4 + 1) * DS + r] = va[p].y;
            As[(kq * 4 + 2) * DS + r] = va[p].z; As[(kq * 4 + 3) * DS + r] = va[p].w;
            Bs[(kq * 4 + 0) * DS + r] = vb[p].x; Bs[(kq * 4 + 1) * DS + r] = vb[p].y;
            Bs[(kq * 4 + 2) * DS + r] = vb[p].z; Bs[(kq * 4 + 3) * DS + r] = vb[p].w;
        }
        __syncthreads();
        if (k0 + DK < g.K) load(k0 + DK);
#pragma unroll
        for (int kk = 0; kk < DK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * kk + h) * DS + ao], Bs[(2 * kk + h) * DS + bo], acc, 0, 0, 0);
    }
    // acc[r]: row (r & 3) + 8 (r >> 2) + 4 h of the wave's quadrant, column li
    const int n = n0 + bo;
    if (n >= g.cn8) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= g.M) continue;
        size_t pix = (size_t)m;
        if (g.dgrad) {
            const int b = m / (g.No * g.No), rem = m - b * g.No * g.No, i = rem / g.No, j = rem - i * g.No;
            pix = ((size_t)b * g.N + 2 * i + py) * g.N + 2 * j + px;
        }
        g.out[pix * g.cn8 + n] = acc[r];
    }
}

// ---- weight gradient -------------------------------------------------------------------------
struct DwgradArgs {
    const float *x, *dy;     // NHWC (B, N, N, cin8), (B, No, No, cout8)
    float *part;             // [share][tile][64 co][64 (tap, ci)]
    int P;                   // B No^2 pixels of dy: the GEMM's K
    int N, No, cin, cin8, cout8, U, ups, nt_n;
};

__global__ __launch_bounds__(256) void k_dwgrad(DwgradArgs g) {
    __shared__ float As[DK * DS], Bs[DK * DS];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, share = blockIdx.y;
    const int cot = tile / g.nt_n, nt = tile - cot * g.nt_n;
    // A = dy: this thread stages the channel quad (t & 15) of the chunk's pixels (t >> 4) and (t >> 4) + 16
    const int aq = (t & 15) * 4, ap = t >> 4;
    const bool alive = cot * DT + aq < g.cout8;
    // B = x at the column's tap: this thread stages column t & 63 of the chunk's pixels (t >> 6) + 4 j
    const int bc = t & 63, bp = t >> 6;
    const int n = nt * DT + bc;
    const bool blive = n < 16 * g.cin;
    const int tap = blive ? n / g.cin : 0, ci = blive ? n - tap * g.cin : 0;
    const int ky = tap >> 2, kx = tap & 3, koff = ky * g.N + kx;

    // The unit's 32 pixels are decomposed once, by 32 lanes, into a table the 64 columns share: the pixel index of tap (0, 0)
    // (input pixel (2i - 1, 2j - 1); used only where the tap is inside the image) and that pixel's two coordinates + 128 in
    // one word.  A pixel beyond P has coordinates -128: every tap of it is outside.  Two tables: unit u + 1's is written
    // while unit u's is still read.
    __shared__ int tbase[2][DK], tyx[2][DK];
    auto table = [&](int u) {
        if (t < DK) {
            const int p = u * DK + t;
            int base = 0, yx = 0;
            if (p < g.P) {
                const int b = p / (g.No * g.No), rem = p - b * g.No * g.No, i = rem / g.No, jj = rem - i * g.No;
                base = (b * g.N + 2 * i - 1) * g.N + 2 * jj - 1;
                yx = ((2 * i - 1 + 128) << 16) | (2 * jj - 1 + 128);
            }
            tbase[u & 1][t] = base;
            tyx[u & 1][t] = yx;
        }
    };
    float4 va[2];
    float vb[8];
    auto load = [&](int u) {
        const int p0 = u * DK;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = p0 + ap + 16 * j;
            va[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (alive && p < g.P) va[j] = *reinterpret_cast<const float4 *>(&g.dy[(size_t)p * g.cout8 + cot * DT + aq]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pl = bp + 4 * j;
            const int base = tbase[u & 1][pl], yx = tyx[u & 1][pl];
            const int yy = (yx >> 16) - 128 + ky, xx = (yx & 0xffff) - 128 + kx;
            vb[j] = 0.f;
            if (blive && (unsigned)yy < (unsigned)g.N && (unsigned)xx < (unsigned)g.N)
                vb[j] = g.x[(size_t)(base + koff) * g.cin8 + ci];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ao = (wave & 1) * 32 + li, bo = (wave >> 1) * 32 + li;

    const int u0 = share * g.ups, u1 = u0 + g.ups < g.U ? u0 + g.ups : g.U;
    table(u0);
    __syncthreads();
    load(u0);
    for (int u = u0; u < u1; ++u) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float *o = &As[(ap + 16 * j) * DS + aq];
            o[0] = va[j].x; o[1] = va[j].y; o[2] = va[j].z; o[3] = va[j].w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[(bp + 4 * j) * DS + bc] = vb[j];
        if (u + 1 < u1) table(u + 1);
        __syncthreads();
        if (u + 1 < u1) load(u + 1);
#pragma unroll
        for (int kk = 0; kk < DK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * kk + h) * DS + ao], Bs[(2 * kk + h) * DS + bo], acc, 0, 0, 0);
    }
    float *o = g.part + ((size_t)share * gridDim.x + tile) * (DT * DT);
#pragma unroll
    for (int r = 0; r < 16; ++r) o[((wave & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * DT + bo] = acc[r];
}

// dw[co][ci][tap] = the shares' slices added in a fixed order (conv_train.hip's k_wgrad_reduce): a workgroup of DRED_WAVES waves
// owns 64 consecutive elements of a slice (one row of a tile); wave q adds the shares q, q + DRED_WAVES, ... in order, then the
// waves' sums are added in order
constexpr int DRED_WAVES = 8;
__global__ __launch_bounds__(64 * DRED_WAVES) void k_dwgrad_reduce(const float *part, float *dw, int S, int nt_n, int cin, int cout,
                                                                  int slice) {
    __shared__ float red[DRED_WAVES][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + e;
    float s = 0.f;
#pragma unroll 4
    for (int sh = q; sh < S; sh += DRED_WAVES) s += part[(size_t)sh * slice + idx];
    red[q][e] = s;
    __syncthreads();
    if (q) return;
    const int col = idx & 63, row = (idx >> 6) & 63, tile = idx >> 12;
    const int cot = tile / nt_n, nt = tile - cot * nt_n;
    const int co = cot * DT + row, n = nt * DT + col;
    if (co >= cout || n >= 16 * cin) return;
    float v = red[0][e];
#pragma unroll
    for (int k = 1; k < DRED_WAVES; ++k) v += red[k][e];
    const int tap = n / cin, ci = n - tap * cin;
    dw[((size_t)co * cin + ci) * 16 + tap] = v;
}

// ---- host side -------------------------------------------------------------------------------
// The weight gradient's partition, a function of (B, N, cin, cout) alone: U units of 32 output pixels go to S shares of `ups`
// consecutive units (the last share may hold fewer), S chosen so that tiles x shares is about 512 workgroups.
struct DwgradPlan { int P, U, ups, S, cot_n, nt_n, tiles; };
static DwgradPlan dwgrad_plan(int64_t B, int N, int cin, int cout) {
    DwgradPlan p = {};
    p.P = (int)(B * (N / 2) * (N / 2));
    p.U = d_cdiv(p.P, DK);
    p.cot_n = d_cdiv(cout, DT);
    p.nt_n = d_cdiv(16 * cin, DT);
    p.tiles = p.cot_n * p.nt_n;
    int want = d_cdiv(512, p.tiles);
    if (want > p.U) want = p.U;
    p.ups = d_cdiv(p.U, want);
    p.S = d_cdiv(p.U, p.ups);
    return p;
}

struct DworkLayout { size_t w, part, floats; };
static DworkLayout dwork_layout(int64_t B, int N, int cin, int cout) {
    const DwgradPlan p = dwgrad_plan(B, N, cin, cout);
    auto al = [](size_t n) { return (n + 63) / 64 * 64; };
    const size_t a = (size_t)cout * 16 * d_up(cin, 8), b = (size_t)16 * cin * d_up(cout, 8);
    DworkLayout L;
    L.w = 0;
    L.part = al(a > b ? a : b);
    L.floats = L.part + al((size_t)p.S * p.tiles * DT * DT);
    return L;
}

static int dconv_shape_check(const char *what, int64_t B, int N, int cin, int cout) {
    QGX_REQUIRE(N >= 2 && N <= 128 && N % 2 == 0, "%s: N = %d, expected an even number 2 ... 128", what, N);
    QGX_REQUIRE(B >= 1 && B <= ((int64_t)1 << 29) / (N * N), "%s: B = %lld, expected 1 ... 2^29 / N^2", what, (long long)B);
    QGX_REQUIRE(cin >= 1 && cin <= 512, "%s: cin = %d, expected 1 ... 512", what, cin);
    QGX_REQUIRE(cout >= 1 && cout <= 512, "%s: cout = %d, expected 1 ... 512", what, cout);
    return QGX_OK;
}
static bool d_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define DCONV_PTR(what, p)                                                                                 \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(d_aligned16(p), "%s: " #p " is not 16-byte aligned", what);                            \
    } while (0)
static int dconv_work_check(const char *what, int64_t B, int N, int cin, int cout, const void *work_dev, size_t work_bytes) {
    QGX_REQUIRE(work_dev, "%s: work_dev is NULL", what);
    QGX_REQUIRE(d_aligned16(work_dev), "%s: work_dev is not 16-byte aligned", what);
    const size_t need = dwork_layout(B, N, cin, cout).floats * sizeof(float);
    QGX_REQUIRE(work_bytes >= need, "%s: work_bytes = %zu, qgx_dconv2d_workspace gives %zu", what, work_bytes, need);
    return QGX_OK;
}

// pack the weights for `dgrad`, then the GEMM: gathered tensor a -> out
static int dconv_run(const float *a, const float *w, float *out, int B, int N, int cin, int cout, int dgrad, float *ws,
                     hipStream_t st) {
    const int cin8 = d_up(cin, 8), cout8 = d_up(cout, 8), No = N / 2;
    const int total = dgrad ? 16 * cin * cout8 : cout * 16 * cin8;
    hipLaunchKernelGGL(k_dpack, dim3((total + 255) / 256), dim3(256), 0, st, w, ws, cin, cout, cin8, cout8, dgrad, total);
    QGX_HIP(hipGetLastError());
    DconvArgs g = {};
    g.a = a; g.wp = ws; g.out = out;
    g.M = B * No * No; g.N = N; g.No = No; g.dgrad = dgrad;
    if (dgrad) { g.ca8 = cout8; g.K = 4 * cout8; g.cn = cin; g.cn8 = cin8; }
    else { g.ca8 = cin8; g.K = 16 * cin8; g.cn = cout; g.cn8 = cout8; }
    hipLaunchKernelGGL(k_dconv, dim3(d_cdiv(g.M, DT), d_cdiv(g.cn8, DT), dgrad ? 4 : 1), dim3(256), 0, st, g);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_dconv2d_workspace(int64_t B, int N, int cin, int cout, size_t *bytes) {
    QGX_REQUIRE(bytes, "qgx_dconv2d_workspace: bytes is NULL");
    if (const int rc = dconv_shape_check("qgx_dconv2d_workspace", B, N, cin, cout)) return rc;
    *bytes = dwork_layout(B, N, cin, cout).floats * sizeof(float);
    return QGX_OK;
}

int qgx_dconv2d_forward(const float *x_dev, const float *w_dev, float *y_dev, int64_t B, int N, int cin, int cout,
                        void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_dconv2d_forward";
    if (const int rc = dconv_shape_check(what, B, N, cin, cout)) return rc;
    DCONV_PTR(what, x_dev); DCONV_PTR(what, w_dev); DCONV_PTR(what, y_dev);
    if (const int rc = dconv_work_check(what, B, N, cin, cout, work_dev, work_bytes)) return rc;
    return dconv_run(x_dev, w_dev, y_dev, (int)B, N, cin, cout, 0, (float *)work_dev, (hipStream_t)stream);
}

int qgx_dconv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout,
                              void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_dconv2d_backward_data";
    if (const int rc = dconv_shape_check(what, B, N, cin, cout)) return rc;
    DCONV_PTR(what, dy_dev); DCONV_PTR(what, w_dev); DCONV_PTR(what, dx_dev);
    if (const int rc = dconv_work_check(what, B, N, cin, cout, work_dev, work_bytes)) return rc;
    return dconv_run(dy_dev, w_dev, dx_dev, (int)B, N, cin, cout, 1, (float *)work_dev, (hipStream_t)stream);
}

int qgx_dconv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, int64_t B, int N, int cin, int cout,
                                void *work_dev, size_t work_bytes, void *stream) {
    const char *what = "qgx_dconv2d_backward_weight";
    if (const int rc = dconv_shape_check(what, B, N, cin, cout)) return rc;
    DCONV_PTR(what, x_dev); DCONV_PTR(what, dy_dev); DCONV_PTR(what, dw_dev);
    if (const int rc = dconv_work_check(what, B, N, cin, cout, work_dev, work_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const DwgradPlan p = dwgrad_plan(B, N, cin, cout);
    const DworkLayout L = dwork_layout(B, N, cin, cout);
    float *ws = (float *)work_dev;
    DwgradArgs g = {};
    g.x = x_dev; g.dy = dy_dev; g.part = ws + L.part;
    g.P = p.P; g.N = N; g.No = N / 2; g.cin = cin; g.cin8 = d_up(cin, 8); g.cout8 = d_up(cout, 8);
    g.U = p.U; g.ups = p.ups; g.nt_n = p.nt_n;
    hipLaunchKernelGGL(k_dwgrad, dim3(p.tiles, p.S), dim3(256), 0, st, g);
    QGX_HIP(hipGetLastError());
    const int slice = p.tiles * DT * DT;
    hipLaunchKernelGGL(k_dwgrad_reduce, dim3(slice / 64), dim3(64 * DRED_WAVES), 0, st, (const float *)(ws + L.part), dw_dev, p.S,
                       p.nt_n, cin, cout, slice);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

}  // extern "C"
