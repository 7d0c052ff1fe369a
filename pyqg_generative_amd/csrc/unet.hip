// DeepInversion U-Net generator body: CGANRegression(generator='DeepInversion'), the DeepInversionGenerator(4, 2) of
// pyqg_generative/tools/deep_inversion.py:44-94 with its blocks res_unit / down / up at :104-160, eval mode, float32,
// circular padding.
//
// Every layer is ONE kernel, k_uconv: an implicit GEMM  out[m, n] = sum_k A[m, k] W[n, k]  on the exact-f32 matrix
// cores (v_mfma_f32_32x32x2_f32), m = output pixel (member, y, x), n = output channel, activations NHWC float32.
//   * K = (tap, input channel) of a 3x3 circular convolution (taps = 9) or the input channel of a pointwise one (taps = 1).
//   * The input transform of the layer is applied while A is staged into LDS: optional 2x2 average pool (down blocks),
//     optional two-source channel concat (up blocks: cat((upsampled, skip), dim=1)), optional eval BatchNorm affine, then
//     optional LeakyReLU(0.2).
//   * A residual unit  conv(bn(x)) + conv1(bn(x))  is two launches.  The first 3x3 convolution folds the unit's second
//     BatchNorm and LeakyReLU into its epilogue; the second carries the 1x1 skip as extra K columns
//     ([im2col(a) | s] . [W_b ; W_1], bias b_b + b_1), s being the unit's input after its own transform.
//   * In-place rule: the LeakyReLUs of res_unit are inplace=True.  With bn='None' (res32_start, res32_end) bn(x) IS x, so
//     the first LeakyReLU overwrites x and the skip computes conv1(LeakyReLU(x)); with BatchNorm bn(x) is a fresh tensor
//     and the skip computes conv1(BN(x)).  The skip source's transform encodes exactly that.
//   * ConvTranspose2d(C, C/2, 2, stride 2) is a pointwise GEMM with 4 C/2 outputs per input pixel whose epilogue
//     scatters them onto the 2x finer grid; conv_end (1x1, 32 -> 2) is a pointwise GEMM with a planar epilogue.
// Summation order: every output sums its K columns chunk by chunk in a fixed order (chunk q = tap-major, then input
// channels, then the skip's channels), inside a chunk in the fixed order of the MFMA sequence.  No split-K: nothing of
// that order depends on the ensemble size B or on the tile shape picked for it, so a member's output is bit-identical
// whatever ensemble it runs in.
#include "common.hpp"
#include <cmath>
#include <new>

namespace qgx {

typedef float uf32x16 __attribute__((ext_vector_type(16)));

// one source of a layer's A operand
struct USrc {
    const float *p0 = nullptr, *p1 = nullptr;   // NHWC; p1: channels c0 .. C-1 of a channel concat (or null)
    const float *scale = nullptr, *shift = nullptr;   // eval BatchNorm as a per-channel affine (or null)
    int C = 0, c0 = 0;       // channels in total, channels held by p0
    int pool = 0;            // 1: 2x2 average pool of a source at twice the output resolution
    int lrelu = 0;           // LeakyReLU(0.2) after the affine
};

enum { UOUT_NHWC = 0, UOUT_UP2 = 1, UOUT_PLANAR = 2 };

struct UConv {
    USrc main, skip;         // skip.C == 0: no skip columns
    const float *w;          // [coutp][K], K = taps * main.C + skip.C
    const float *bias;       // [coutp]
    const float *escale, *eshift;   // epilogue BatchNorm affine (or null)
    int elrelu;
    float *out;
    int B, h, taps, K, cout, mode;
};

__device__ __forceinline__ float4 lrelu4(float4 v) {
    v.x = v.x > 0.f ? v.x : 0.2f * v.x; v.y = v.y > 0.f ? v.y : 0.2f * v.y;
    v.z = v.z > 0.f ? v.z : 0.2f * v.z; v.w = v.w > 0.f ? v.w : 0.2f * v.w;
    return v;
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// four consecutive channels c .. c+3 of source s at pixel (b, y, x) of an h x h grid, transformed
__device__ __forceinline__ float4 load_src(const USrc &s, int b, int y, int x, int c, int h) {
    float4 v;
    if (s.pool) {
        // AvgPool2d(2, 2): (in[2y,2x] + in[2y,2x+1] + in[2y+1,2x] + in[2y+1,2x+1]) / 4, summed in that order
        const int H = 2 * h;
        const size_t o = (((size_t)b * H + 2 * y) * H + 2 * x) * s.C + c;
        const float4 a0 = *reinterpret_cast<const float4 *>(s.p0 + o);
        const float4 a1 = *reinterpret_cast<const float4 *>(s.p0 + o + s.C);
        const float4 a2 = *reinterpret_cast<const float4 *>(s.p0 + o + (size_t)H * s.C);
        const float4 a3 = *reinterpret_cast<const float4 *>(s.p0 + o + (size_t)H * s.C + s.C);
        v = add4(add4(add4(a0, a1), a2), a3);
        v.x *= 0.25f; v.y *= 0.25f; v.z *= 0.25f; v.w *= 0.25f;
    } else {
        const size_t pix = ((size_t)b * h + y) * h + x;
        v = c < s.c0 ? *reinterpret_cast<const float4 *>(s.p0 + pix * s.c0 + c)
                     : *reinterpret_cast<const float4 *>(s.p1 + pix * (s.C - s.c0) + (c - s.c0));
    }
    if (s.scale) {
        const float4 sc = *reinterpret_cast<const float4 *>(s.scale + c), sh = *reinterpret_cast<const float4 *>(s.shift + c);
        v = make_float4(v.x * sc.x + sh.x, v.y * sc.y + sh.y, v.z * sc.z + sh.z, v.w * sc.w + sh.w);
    }
    return s.lrelu ? lrelu4(v) : v;
}

// WM x WN waves (WM * WN = 4), each one 32 x 32 MFMA block: a workgroup tile of TM = 32 WM pixels x TN = 32 WN channels.
// K is consumed in chunks of KC columns (one tap, KC input channels), staged in LDS; the global reads of chunk q + 1
// are issued before the MFMAs of chunk q.  Lane half hf supplies K columns 8g + 4hf + e (e = 0..3) of every group of 8
// with one 16-byte LDS read of A and of B.
template <int WM, int KC>
__global__ __launch_bounds__(256) void k_uconv(UConv a) {
    constexpr int WN = 4 / WM, TM = 32 * WM, TN = 32 * WN, LDK = KC + 4, G4 = KC / 4;
    constexpr int AIT = (TM * G4 + 255) / 256, BIT = (TN * G4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float As[TM * LDK];
    __shared__ __attribute__((aligned(16))) float Bs[TN * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int h = a.h, hh = h * h, M = a.B * hh;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int cpt = a.main.C / KC, nmain = a.taps * cpt, nchunks = nmain + a.skip.C / KC;

    // the pixels this thread stages (fixed over the K loop)
    int pb[AIT], py[AIT], px[AIT];
#pragma unroll
    for (int it = 0; it < AIT; ++it) {
        const int idx = tid + it * 256, m = m0 + idx / G4;
        pb[it] = -1; py[it] = 0; px[it] = 0;
        if (idx < TM * G4 && m < M) { pb[it] = m / hh; const int r = m - pb[it] * hh; py[it] = r / h; px[it] = r - py[it] * h; }
    }
    float4 ra[AIT], rb[BIT];
#pragma unroll
    for (int it = 0; it < BIT; ++it) rb[it] = make_float4(0.f, 0.f, 0.f, 0.f);

    uf32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = As + (wm * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    const float *bp = Bs + (wn * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    for (int q = -1; q < nchunks; ++q) {
        if (q >= 0) {
#pragma unroll
            for (int it = 0; it < AIT; ++it) {
                const int idx = tid + it * 256;
                if (TM * G4 % 256 == 0 || idx < TM * G4) *reinterpret_cast<float4 *>(As + (idx / G4) * LDK + 4 * (idx % G4)) = ra[it];
            }
#pragma unroll
            for (int it = 0; it < BIT; ++it) {
                const int idx = tid + it * 256;
                if (TN * G4 % 256 == 0 || idx < TN * G4) *reinterpret_cast<float4 *>(Bs + (idx / G4) * LDK + 4 * (idx % G4)) = rb[it];
            }
            __syncthreads();
        }
        if (q + 1 < nchunks) {            // the global reads of chunk q + 1, in flight under chunk q's MFMAs
            const int qn = q + 1;
            const bool sk = qn >= nmain;
            const int tap = sk || a.taps == 1 ? 4 : qn / cpt;
            const int cb = sk ? (qn - nmain) * KC : (qn - (qn / cpt) * cpt) * KC;
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            USrc s;                        // field by field (selecting the whole struct by reference puts it in scratch)
            s.p0 = sk ? a.skip.p0 : a.main.p0; s.p1 = sk ? a.skip.p1 : a.main.p1;
            s.scale = sk ? a.skip.scale : a.main.scale; s.shift = sk ? a.skip.shift : a.main.shift;
            s.C = sk ? a.skip.C : a.main.C; s.c0 = sk ? a.skip.c0 : a.main.c0;
            s.pool = sk ? a.skip.pool : a.main.pool; s.lrelu = sk ? a.skip.lrelu : a.main.lrelu;
#pragma unroll
            for (int it = 0; it < AIT; ++it) {
                const int g = (tid + it * 256) % G4;
                ra[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pb[it] >= 0) {
                    int y = py[it] + dy, x = px[it] + dx;
                    y = y < 0 ? y + h : (y >= h ? y - h : y);
                    x = x < 0 ? x + h : (x >= h ? x - h : x);
                    ra[it] = load_src(s, pb[it], y, x, cb + 4 * g, h);
                }
            }
#pragma unroll
            for (int it = 0; it < BIT; ++it) {
                const int idx = tid + it * 256;
                if (TN * G4 % 256 == 0 || idx < TN * G4)
                    rb[it] = *reinterpret_cast<const float4 *>(a.w + (size_t)(n0 + idx / G4) * a.K + (size_t)qn * KC + 4 * (idx % G4));
            }
        }
        if (q < 0) continue;
#pragma unroll
        for (int g8 = 0; g8 < KC / 8; ++g8) {
            const float4 av = *reinterpret_cast<const float4 *>(ap + 8 * g8);
            const float4 bv = *reinterpret_cast<const float4 *>(bp + 8 * g8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: bias (+ BatchNorm affine + LeakyReLU), store.  acc[r] of lane l: pixel row (r&3) + 8(r>>2) + 4(l>>5),
    // channel l&31 of the wave's block
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= a.cout) return;
    const float bias = a.bias[n];
    const float sc = a.escale ? a.escale[n] : 1.f, sh = a.escale ? a.eshift[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= M) continue;
        float v = acc[r] + bias;
        if (a.escale) v = v * sc + sh;
        if (a.elrelu) v = v > 0.f ? v : 0.2f * v;
        if (a.mode == UOUT_NHWC) {
            a.out[(size_t)m * a.cout + n] = v;
        } else {
            const int b = m / hh, rr = m - b * hh, y = rr / h, x = rr - y * h;
            if (a.mode == UOUT_UP2) {        // n = (2 di + dj) co + c: output pixel (2y + di, 2x + dj) of the 2h grid
                const int co = a.cout / 4, t = n / co, c = n - t * co, H = 2 * h;
                a.out[(((size_t)b * H + 2 * y + (t >> 1)) * H + 2 * x + (t & 1)) * co + c] = v;
            } else {
                a.out[((size_t)b * a.cout + n) * hh + rr] = v;
            }
        }
    }
}

// planar (B, 4, N, N) network input -> NHWC (B, N, N, 8), channels 4..7 zero (the first layer's K chunk is 8 wide)
__global__ void k_unet_in(const float *x, float *x8, int npix, int B) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * npix) return;
    const size_t b = i / npix, p = i - b * npix;
    const float *s = x + b * 4 * npix + p;
    float4 *d = reinterpret_cast<float4 *>(x8 + i * 8);
    d[0] = make_float4(s[0], s[npix], s[2 * (size_t)npix], s[3 * (size_t)npix]);
    d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct UConvW { float *w = nullptr, *bias = nullptr, *escale = nullptr, *eshift = nullptr; int K = 0, cout = 0; };
struct UNet {
    UConvW conv32, conv_end, up[4];
    struct Unit { UConvW a, b; float *bscale = nullptr, *bshift = nullptr; int cin = 0, cout = 0; } unit[11];
    std::vector<void *> allocs;
};

// (cin, cout) of the 11 residual units in qgx_unet_weights order
static const int UNIT_CIN[11] = {32, 32, 64, 128, 256, 512, 512, 256, 128, 64, 32};
static const int UNIT_COUT[11] = {32, 64, 128, 256, 512, 512, 256, 128, 64, 32, 32};

static int upload(UNet *u, const std::vector<float> &h, float **dst) {
    float *p = nullptr;
    QGX_HIP(hipMalloc((void **)&p, h.size() * sizeof(float)));
    u->allocs.push_back(p);
    QGX_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = p;
    return QGX_OK;
}
static int coutp_of(int cout) { return (cout + 127) / 128 * 128; }   // every tile width divides it; padded rows are zero

// eval BatchNorm as x s + t: s = gamma / sqrt(var + eps), t = beta - mean s
static int upload_bn(UNet *u, const float *g, const float *be, const float *mu, const float *var, int C, float eps,
                     float **sc, float **sh) {
    std::vector<float> s(C), t(C);
    for (int c = 0; c < C; ++c) {
        s[c] = (float)((double)g[c] / std::sqrt((double)var[c] + (double)eps));
        t[c] = (float)((double)be[c] - (double)mu[c] * (double)s[c]);
    }
    int rc = upload(u, s, sc);
    return rc ? rc : upload(u, t, sh);
}

// 3x3 convolution (cout, cin, 3, 3) with cin padded to cinp, optionally followed by the 1x1 skip (cout, cskip, 1, 1)
static int pack_conv3(UNet *u, UConvW &L, const float *w, const float *b, int cout, int cin, int cinp, const float *w1,
                      const float *b1, int cskip) {
    const int K = 9 * cinp + cskip, cp = coutp_of(cout);
    std::vector<float> W((size_t)cp * K, 0.f), bias(cp, 0.f);
    for (int n = 0; n < cout; ++n) {
        for (int c = 0; c < cin; ++c)
            for (int t = 0; t < 9; ++t) W[(size_t)n * K + t * cinp + c] = w[((size_t)n * cin + c) * 9 + t];
        for (int c = 0; c < cskip; ++c) W[(size_t)n * K + 9 * cinp + c] = w1[(size_t)n * cskip + c];
        bias[n] = b1 ? b[n] + b1[n] : b[n];
    }
    L.K = K; L.cout = cout;
    int rc = upload(u, W, &L.w);
    return rc ? rc : upload(u, bias, &L.bias);
}

// ConvTranspose2d(cin, co, 2, stride 2): (cin, co, 2, 2) -> rows n = (2 di + dj) co + c, K = cin
static int pack_up(UNet *u, UConvW &L, const float *w, const float *b, int cin, int co) {
    const int cout = 4 * co, cp = coutp_of(cout);
    std::vector<float> W((size_t)cp * cin, 0.f), bias(cp, 0.f);
    for (int t = 0; t < 4; ++t)
        for (int c = 0; c < co; ++c) {
            const int n = t * co + c;
            for (int ci = 0; ci < cin; ++ci) W[(size_t)n * cin + ci] = w[((size_t)ci * co + c) * 4 + t];
            bias[n] = b[c];
        }
    L.K = cin; L.cout = cout;
    int rc = upload(u, W, &L.w);
    return rc ? rc : upload(u, bias, &L.bias);
}

void unet_destroy(UNet *u) {
    if (!u) return;
    for (void *p : u->allocs) (void)hipFree(p);
    delete u;
}

int unet_create(const qgx_unet_weights *g, UNet **out) {
    QGX_REQUIRE(g && out && g->conv32_w && g->conv32_b && g->conv_end_w && g->conv_end_b, "qgx_generator_create_unet: null weights");
    UNet *u = new (std::nothrow) UNet();
    if (!u) { set_error("out of host memory"); return QGX_ERR_NOMEM; }
    auto fail = [&](int rc) { unet_destroy(u); return rc; };
    int rc = pack_conv3(u, u->conv32, g->conv32_w, g->conv32_b, 32, 4, 8, nullptr, nullptr, 0);
    if (rc) return fail(rc);
    for (int i = 0; i < 11; ++i) {
        const qgx_unet_res &r = g->res[i];
        auto &U = u->unit[i];
        U.cin = UNIT_CIN[i]; U.cout = UNIT_COUT[i];
        const bool bn = i != 0 && i != 10;          // res32_start and res32_end are bn='None'
        if (!r.conv_a_w || !r.conv_a_b || !r.conv_b_w || !r.conv_b_b || !r.skip_w || !r.skip_b ||
            (bn && !(r.bn_gamma && r.bn_beta && r.bn_mean && r.bn_var && r.bn2_gamma && r.bn2_beta && r.bn2_mean && r.bn2_var)) ||
            (!bn && (r.bn_gamma || r.bn2_gamma))) {
            set_error("qgx_generator_create_unet: residual unit %d: missing tensor (BatchNorm given %s)", i,
                      bn ? "for a BatchNorm unit: all of bn and bn2" : "for a bn='None' unit: must be NULL");
            return fail(QGX_ERR_INVALID);
        }
        if ((rc = pack_conv3(u, U.a, r.conv_a_w, r.conv_a_b, U.cout, U.cin, U.cin, nullptr, nullptr, 0))) return fail(rc);
        if ((rc = pack_conv3(u, U.b, r.conv_b_w, r.conv_b_b, U.cout, U.cout, U.cout, r.skip_w, r.skip_b, U.cin))) return fail(rc);
        if (bn) {
            if ((rc = upload_bn(u, r.bn_gamma, r.bn_beta, r.bn_mean, r.bn_var, U.cin, g->bn_eps, &U.bscale, &U.bshift))) return fail(rc);
            if ((rc = upload_bn(u, r.bn2_gamma, r.bn2_beta, r.bn2_mean, r.bn2_var, U.cout, g->bn_eps, &U.a.escale, &U.a.eshift))) return fail(rc);
        }
    }
    for (int i = 0; i < 4; ++i) {
        QGX_REQUIRE(g->up_w[i] && g->up_b[i], "qgx_generator_create_unet: upsampling %d: null weights", i);
        const int c = 512 >> i;
        if ((rc = pack_up(u, u->up[i], g->up_w[i], g->up_b[i], c, c / 2))) return fail(rc);
    }
    {
        const int cp = coutp_of(2);
        std::vector<float> W((size_t)cp * 32, 0.f), bias(cp, 0.f);
        for (int n = 0; n < 2; ++n) { for (int c = 0; c < 32; ++c) W[(size_t)n * 32 + c] = g->conv_end_w[n * 32 + c]; bias[n] = g->conv_end_b[n]; }
        u->conv_end.K = 32; u->conv_end.cout = 2;
        if ((rc = upload(u, W, &u->conv_end.w)) || (rc = upload(u, bias, &u->conv_end.bias))) return fail(rc);
    }
    *out = u;
    return QGX_OK;
}

bool unet_size_ok(int N) { return N == 32 || N == 48 || N == 64 || N == 96 || N == 128; }

// workspace floats per pixel of the N x N grid (unet_forward's buffers)
static constexpr int WS_PER_PIXEL = 8 + 4 * 32 + 16 + 8 + 4;
size_t unet_workspace_floats(int B, int N) { return (size_t)B * N * N * WS_PER_PIXEL; }

static USrc src(const float *p, int C) { USrc s; s.p0 = p; s.C = C; s.c0 = C; return s; }

// tile shape by the GEMM's M and width (the K order is the same for every shape)
static int launch(UConv &a, hipStream_t st) {
    const int M = a.B * a.h * a.h;
    const int kc = a.main.C % 32 == 0 ? 32 : 8;
    int wm = a.cout <= 32 ? 4 : (M <= 32 ? 1 : 2);
    if (kc == 8) wm = 4;
    const int tm = 32 * wm, tn = 128 / wm;
    dim3 grid((M + tm - 1) / tm, (a.cout + tn - 1) / tn), block(256);
    if (kc == 8) hipLaunchKernelGGL((k_uconv<4, 8>), grid, block, 0, st, a);
    else if (wm == 4) hipLaunchKernelGGL((k_uconv<4, 32>), grid, block, 0, st, a);
    else if (wm == 2) hipLaunchKernelGGL((k_uconv<2, 32>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_uconv<1, 32>), grid, block, 0, st, a);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

static int run(const UConvW &L, const USrc &main, const USrc &skip, int taps, float *out, int B, int h, int elrelu, int mode,
               hipStream_t st) {
    UConv a;
    a.main = main; a.skip = skip;
    a.w = L.w; a.bias = L.bias; a.escale = L.escale; a.eshift = L.eshift; a.elrelu = elrelu;
    a.out = out; a.B = B; a.h = h; a.taps = taps; a.K = L.K; a.cout = L.cout; a.mode = mode;
    return launch(a, st);
}

// residual unit i: x (its input after pooling / concat, as a source without transform) -> out (B, h, h, cout)
static int res_unit(const UNet *u, int i, USrc x, float *T, float *out, int B, int h, hipStream_t st) {
    const auto &U = u->unit[i];
    const bool bn = U.bscale != nullptr;
    USrc xa = x;                      // conv(bn(x)): LeakyReLU(bn(x)) -> conv3x3 -> BN2 -> LeakyReLU (epilogue)
    xa.scale = U.bscale; xa.shift = U.bshift; xa.lrelu = 1;
    int rc = run(U.a, xa, USrc(), 9, T, B, h, 1, UOUT_NHWC, st);
    if (rc) return rc;
    USrc xs = xa;                     // conv1(bn(x)): BN(x) fresh; bn='None': x was overwritten by the in-place LeakyReLU
    xs.lrelu = bn ? 0 : 1;
    return run(U.b, src(T, U.cout), xs, 9, out, B, h, 0, UOUT_NHWC, st);
}

// DeepInversionGenerator.forward (deep_inversion.py:79-94): x planar (B, 4, N, N) -> y planar (B, 2, N, N)
int unet_forward(const UNet *u, const float *x, float *y, float *ws, int B, int N, hipStream_t st) {
    QGX_REQUIRE(unet_size_ok(N), "U-Net generator: N = %d is not supported (32, 48, 64, 96 or 128)", N);
    const size_t P = (size_t)B * N * N;
    float *X8 = ws, *T = X8 + 8 * P, *R1 = T + 32 * P, *R2 = R1 + 32 * P, *im64 = R2 + 32 * P, *im32 = im64 + 32 * P,
          *im16 = im32 + 16 * P, *im8 = im16 + 8 * P;
    hipLaunchKernelGGL(k_unet_in, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, x, X8, N * N, B);
    int rc = run(u->conv32, src(X8, 8), USrc(), 9, R1, B, N, 0, UOUT_NHWC, st);           // conv32
    if (!rc) rc = res_unit(u, 0, src(R1, 32), T, im64, B, N, st);                            // res32_start
    float *skips[4] = {im64, im32, im16, im8};
    const int ch[5] = {32, 64, 128, 256, 512};
    for (int l = 0; l < 4 && !rc; ++l) {                                                     // down64 .. down512
        USrc p = src(skips[l], ch[l]);
        p.pool = 1;
        rc = res_unit(u, 1 + l, p, T, l < 3 ? skips[l + 1] : R1, B, N >> (l + 1), st);
    }
    if (!rc) rc = res_unit(u, 5, src(R1, 512), T, R2, B, N >> 4, st);                        // res512
    for (int l = 0; l < 4 && !rc; ++l) {                                                     // up512 .. up64
        const int h = N >> (4 - l), c = ch[4 - l];
        rc = run(u->up[l], src(R2, c), USrc(), 1, R1, B, h, 0, UOUT_UP2, st);                // upsampling -> (2h, c/2)
        if (rc) break;
        USrc cat = src(R1, c);                                                               // cat((upsampled, skip), dim=1)
        cat.c0 = c / 2; cat.p1 = skips[3 - l];
        rc = res_unit(u, 6 + l, cat, T, R2, B, 2 * h, st);
    }
    if (!rc) rc = res_unit(u, 10, src(R2, 32), T, R1, B, N, st);                             // res32_end
    if (!rc) rc = run(u->conv_end, src(R1, 32), USrc(), 1, y, B, N, 0, UOUT_PLANAR, st);   // conv_end
    return rc;
}

}  // namespace qgx
