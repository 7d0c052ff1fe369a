// The architecture-generic AndrewCNN engine: circular-padded 5x5 / 3x3 convolutions with RUN-TIME channel counts as
// implicit GEMMs on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32), fused bias + ReLU + eval-mode BatchNorm.
//
// Replaces AndrewCNN.forward (cnn_tools.py:125-176) for every net the constructor builds with its default kernels:
// hidden_channels of length 1 ... 7, widths 1 ... 256, batch_norm / bias on or off, div (the divergence stays
// fluxdiv.hip, behind cnn_forward).  The shipped architecture keeps conv.hip's templated kernels; this file is what
// qgx_generator_create_arch hands every other net to.
//
// One kernel, k_convg<NT, MT>, in the data layout and MFMA roles of conv.hip's k_conv: activations NHWC float32 with the
// pixel stride padded to 8 channels, one workgroup of 4 waves on R full-width rows (at most 8 M-tiles of 32 pixels, MT = 2
// per wave; 12 and MT = 3 at 48 x 48 and 96 x 96, whose rows make no 256 pixels), the input patch staged per chunk of at most 32 input channels into LDS with pixel stride 36, weights packed
// on the host as a sequence of K groups [group][coutp][8] that the kernel walks linearly (chunk, tap, 8 channels), zero
// padded in K (to 8) and N (to 32).  NT = 1 or 2 output tiles of 32 channels per workgroup are the compile-time
// accumulator shapes; blockIdx.y picks the slice of output tiles, the chunk and group counts are run-time.
//   * first layer: the planar (B, n_in, N, N) input is staged as an 8-channel pixel (channels n_in ... 7 zero);
//   * hidden layers: NHWC in, NHWC out, channels cout ... cstore - 1 stored as the zeros the zero weights give;
//   * last layer: planar (B, 2 | 4, N, N) out, bias only, lanes of the padded output channels store nothing.
#include "generator.hpp"
#include <vector>

namespace qgx {

#include "conv_types.hpp"

struct ConvGArgs {
    const float *in;       // planar (B, cin, N, N) or NHWC (B, N, N, cinp)
    float *out;            // NHWC (B, N, N, cstore) or planar (B, cstore, N, N)
    const float *w;        // [group][coutp][8], one zero group behind the last (the prefetch reads it)
    const float *bias, *scale, *shift;   // [coutp]
    int N, R, ks;
    int cin;               // planar input: its channels
    int cinp;              // K per tap (input channels padded to 8) = pixel stride of an NHWC input
    int coutp;             // output channels padded to 32
    int cstore;            // channels stored per pixel (NHWC: cout padded to 8, the pixel stride), planar: cout
    int planar_in, final;
};

constexpr int G_CC = 32;              // input channels per staged chunk
constexpr int G_STRIDE = G_CC + 4;    // floats per patch pixel: 16-byte reads of consecutive pixels fall on different banks

// LINEAR (training, conv_train.hip): NHWC out with the bias alone — no ReLU, no BatchNorm affine, scale / shift not read
template <int NT, int MT, bool LINEAR = false>
__global__ __launch_bounds__(256) void k_convg(ConvGArgs a) {
    constexpr int G_MT = MT;          // M-tiles per wave
    float *patch = reinterpret_cast<float *>(conv_smem);
    const int N = a.N, R = a.R, KS = a.ks, P = KS / 2, T = KS * KS;
    const int tiles_per_img = N / R;
    const int b = blockIdx.x / tiles_per_img;
    const int y0 = (blockIdx.x - b * tiles_per_img) * R;
    const int nt0 = blockIdx.y * NT;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int li = lane & 31, h = lane >> 5;
    const int ntiles = R * N / 32;
    const int PR = R + KS - 1;
    const int coutp = a.coutp;

    int py[G_MT], px[G_MT];
    bool act[G_MT];            // wave-uniform: the wave owns a real tile (small ensembles run tiles of fewer than 8 M-tiles)
#pragma unroll
    for (int mt = 0; mt < G_MT; ++mt) {
        int tile = wave + 4 * mt;
        act[mt] = tile < ntiles;
        if (!act[mt]) tile = 0;
        const int p = tile * 32 + li;
        py[mt] = p / N;
        px[mt] = p - py[mt] * N;
    }
    f32x16 acc[G_MT][NT];
#pragma unroll
    for (int mt = 0; mt < G_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    const float4 *wp = reinterpret_cast<const float4 *>(a.w) + (size_t)li * 2 + h;
    float4 Bn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) Bn[nt] = wp[(size_t)(nt0 + nt) * 64];

    const int cinp = a.cinp;
    for (int c0 = 0; c0 < cinp; c0 += G_CC) {
        const int cc = cinp - c0 < G_CC ? cinp - c0 : G_CC;      // a multiple of 8
        const int g8n = cc >> 3;
        __syncthreads();
        if (a.planar_in) {
            // the whole (tiny) input: patch[(pr*N + x)*STRIDE + c], c = 0 ... 7, zero from cin on (cinp = 8: one chunk)
            const int cin = a.cin;
            for (int it = threadIdx.x; it < PR * N * 8; it += 256) {
                const int x = it % N;
                const int pr = (it / N) % PR;
                const int c = it / (N * PR);
                int gy = y0 - P + pr;
                gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
                patch[(pr * N + x) * G_STRIDE + c] = c < cin ? a.in[(((size_t)b * cin + c) * N + gy) * N + x] : 0.f;
            }
        } else {
            const int C4 = cc >> 2;
            for (int it = threadIdx.x; it < PR * N * 8; it += 256) {
                const int c4 = it & 7, pl = it >> 3;
                if (c4 >= C4) continue;
                const int pr = pl / N, x = pl - pr * N;
                int gy = y0 - P + pr;
                gy = gy < 0 ? gy + N : (gy >= N ? gy - N : gy);
                *reinterpret_cast<float4 *>(&patch[pl * G_STRIDE + c4 * 4]) =
                    *reinterpret_cast<const float4 *>(&a.in[(((size_t)b * N + gy) * N + x) * cinp + c0 + c4 * 4]);
            }
        }
        __syncthreads();
        // K loop over (tap, 8-channel group); the A fragment (LDS) and the B fragment (packed weights, L2) of the next step
        // are requested before this step's MFMAs.  The weights are one linear sequence of groups, so the B prefetch runs
        // across taps and chunks (and over the next chunk's staging); the last step of all reads the zero group at the end.
        int ky = 0, kx = 0;
        int aoff[G_MT];
        float4 An[G_MT];
#pragma unroll
        for (int mt = 0; mt < G_MT; ++mt) {
            int col = px[mt] - P;
            col = col < 0 ? col + N : col;
            aoff[mt] = (py[mt] * N + col) * G_STRIDE + 4 * h;
            An[mt] = *reinterpret_cast<const float4 *>(&patch[aoff[mt]]);
        }
        for (int tap = 0; tap < T; ++tap) {
            int nkx = kx + 1, nky = ky;
            if (nkx == KS) { nkx = 0; ++nky; }
            int aoff_n[G_MT];
#pragma unroll
            for (int mt = 0; mt < G_MT; ++mt) {
                int col = px[mt] + nkx - P;
                col = col < 0 ? col + N : (col >= N ? col - N : col);
                aoff_n[mt] = tap == T - 1 ? aoff[mt] : ((py[mt] + nky) * N + col) * G_STRIDE + 4 * h;
            }
            for (int g8 = 0; g8 < g8n; ++g8) {
                float4 A[G_MT], Bf[NT];
#pragma unroll
                for (int mt = 0; mt < G_MT; ++mt) A[mt] = An[mt];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) Bf[nt] = Bn[nt];
                wp += (size_t)coutp * 2;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) Bn[nt] = wp[(size_t)(nt0 + nt) * 64];
#pragma unroll
                for (int mt = 0; mt < G_MT; ++mt)
                    An[mt] = *reinterpret_cast<const float4 *>(&patch[g8 + 1 < g8n ? aoff[mt] + (g8 + 1) * 8 : aoff_n[mt]]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mt = 0; mt < G_MT; ++mt) {
                    if (!act[mt]) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32((&A[mt].x)[e], (&Bf[nt].x)[e], acc[mt][nt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int mt = 0; mt < G_MT; ++mt) aoff[mt] = aoff_n[mt];
            kx = nkx; ky = nky;
        }
    }

    // ---- epilogue: bias (+ ReLU + BatchNorm affine), store.  acc[r] is pixel (r & 3) + 8 (r >> 2) + 4 h of the tile, channel li
    const int cstore = a.cstore;
#pragma unroll
    for (int mt = 0; mt < G_MT; ++mt) {
        if (!act[mt]) continue;
        const int tile = wave + 4 * mt;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = (nt0 + nt) * 32 + li;
            if (co >= cstore) continue;            // padded output channels: nothing past the channels the buffer holds
            const float bias = a.bias[co];
            if constexpr (LINEAR) {
                float *o = a.out + ((size_t)b * N * N + (size_t)y0 * N) * cstore + co;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    o[(size_t)p * cstore] = acc[mt][nt][r] + bias;
                }
            } else if (a.final) {
                float *o = a.out + ((size_t)b * cstore + co) * N * N + (size_t)y0 * N;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    o[p] = acc[mt][nt][r] + bias;
                }
            } else {
                const float sc = a.scale[co], sh = a.shift[co];
                float *o = a.out + ((size_t)b * N * N + (size_t)y0 * N) * cstore + co;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float vv = acc[mt][nt][r] + bias;
                    vv = fmaxf(vv, 0.f);
                    o[(size_t)p * cstore] = vv * sc + sh;
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------
static const int SHIPPED_HID[7] = {128, 64, 32, 32, 32, 32, 32};
static const int SHIPPED_KS[8] = {5, 5, 3, 3, 3, 3, 3, 3};
static int round_up(int v, int m) { return (v + m - 1) / m * m; }

int cnn_arch_check(const qgx_cnn_arch *a, int inet) {
    QGX_REQUIRE(a->n_layers >= 2 && a->n_layers <= 8, "qgx_cnn_arch (net %d): n_layers = %d, expected 2 ... 8", inet, a->n_layers);
    const int nl = a->n_layers;
    QGX_REQUIRE(a->channels[0] == 2 || a->channels[0] == 4, "qgx_cnn_arch (net %d): channels[0] = %d, expected n_in 2 or 4", inet, a->channels[0]);
    for (int l = 1; l < nl; ++l)
        QGX_REQUIRE(a->channels[l] >= 1 && a->channels[l] <= 256, "qgx_cnn_arch (net %d): channels[%d] = %d, a hidden width is 1 ... 256", inet, l, a->channels[l]);
    QGX_REQUIRE(a->channels[nl] == 2 || a->channels[nl] == 4, "qgx_cnn_arch (net %d): channels[%d] = %d, expected n_out 2 (or 4: flux form)", inet, nl, a->channels[nl]);
    for (int l = 0; l < nl; ++l)
        QGX_REQUIRE(a->ksize[l] == 3 || a->ksize[l] == 5, "qgx_cnn_arch (net %d): ksize[%d] = %d, expected 3 or 5", inet, l, a->ksize[l]);
    QGX_REQUIRE(a->batch_norm == 0 || a->batch_norm == 1, "qgx_cnn_arch (net %d): batch_norm = %d, expected 0 or 1", inet, a->batch_norm);
    QGX_REQUIRE(a->bias == 0 || a->bias == 1, "qgx_cnn_arch (net %d): bias = %d, expected 0 or 1", inet, a->bias);
    for (int l = 0; l < nl; ++l) {
        QGX_REQUIRE(a->conv_w[l], "qgx_cnn_arch (net %d): conv_w[%d] is NULL", inet, l);
        QGX_REQUIRE(!a->bias || a->conv_b[l], "qgx_cnn_arch (net %d): conv_b[%d] is NULL, but bias = 1", inet, l);
        if (a->batch_norm && l < nl - 1) {
            QGX_REQUIRE(a->bn_gamma[l], "qgx_cnn_arch (net %d): bn_gamma[%d] is NULL, but batch_norm = 1", inet, l);
            QGX_REQUIRE(a->bn_beta[l], "qgx_cnn_arch (net %d): bn_beta[%d] is NULL, but batch_norm = 1", inet, l);
            QGX_REQUIRE(a->bn_mean[l], "qgx_cnn_arch (net %d): bn_mean[%d] is NULL, but batch_norm = 1", inet, l);
            QGX_REQUIRE(a->bn_var[l], "qgx_cnn_arch (net %d): bn_var[%d] is NULL, but batch_norm = 1", inet, l);
        }
    }
    QGX_REQUIRE(!a->batch_norm || (a->bn_eps > 0.f && a->bn_eps < 1.f), "qgx_cnn_arch (net %d): bn_eps = %g, expected a small positive number (1e-5)", inet, (double)a->bn_eps);
    return QGX_OK;
}

bool cnn_arch_is_shipped(const qgx_cnn_arch *a) {
    if (a->force_generic || a->n_layers != 8 || !a->batch_norm || !a->bias) return false;
    for (int l = 0; l < 7; ++l) if (a->channels[l + 1] != SHIPPED_HID[l]) return false;
    for (int l = 0; l < 8; ++l) if (a->ksize[l] != SHIPPED_KS[l]) return false;
    return true;
}

void cnn_arch_to_weights(const qgx_cnn_arch *a, qgx_cnn_weights *w) {
    w->n_in = a->channels[0]; w->n_out = a->channels[8]; w->bn_eps = a->bn_eps;
    for (int l = 0; l < 8; ++l) { w->conv_w[l] = a->conv_w[l]; w->conv_b[l] = a->conv_b[l]; }
    for (int l = 0; l < 7; ++l) { w->bn_gamma[l] = a->bn_gamma[l]; w->bn_beta[l] = a->bn_beta[l]; w->bn_mean[l] = a->bn_mean[l]; w->bn_var[l] = a->bn_var[l]; }
}

static int upload(float *&dst, const std::vector<float> &h) {
    QGX_HIP(hipMalloc((void **)&dst, h.size() * sizeof(float)));
    QGX_HIP(hipMemcpy(dst, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return QGX_OK;
}

// A failure half-way (hipMalloc, hipMemcpy) leaves the layers packed so far allocated: the creator destroys the handle
// (generator.hip::hand_out), and qgx_generator_destroy's cnn_free_net runs LayerHost::free_device over all 8 layers of every
// net, which frees w, bias, scale and shift — the four allocations made here — and skips the null pointers of the rest.
int cnn_pack_net_arch(NetHost &net, const qgx_cnn_arch *a) {
    const int nl = a->n_layers;
    net.n_in = a->channels[0]; net.n_out = a->channels[nl];
    net.generic = true; net.n_layers = nl; net.batch_norm = a->batch_norm; net.bias = a->bias;
    if (net.flux()) { if (const int rc = fluxdiv_prepare()) return rc; }
    for (int l = 0; l < nl; ++l) {
        LayerHost &L = net.L[l];
        const bool first = l == 0, last = l == nl - 1;
        L.cin = a->channels[l]; L.cout = a->channels[l + 1]; L.ks = a->ksize[l];
        L.cinp = first ? 8 : round_up(L.cin, 8);
        L.coutp = round_up(L.cout, 32);
        L.cstore = last ? L.cout : round_up(L.cout, 8);
        const int T = L.ks * L.ks;
        // the K groups in the order the kernel walks them: chunk of <= 32 channels, tap, 8 channels; + one zero group
        L.ngroups = T * (L.cinp / 8);
        std::vector<float> pw((size_t)(L.ngroups + 1) * L.coutp * 8, 0.f);
        size_t g = 0;
        for (int c0 = 0; c0 < L.cinp; c0 += G_CC) {
            const int cc = L.cinp - c0 < G_CC ? L.cinp - c0 : G_CC;
            for (int t = 0; t < T; ++t)
                for (int g8 = 0; g8 < cc / 8; ++g8, ++g)
                    for (int co = 0; co < L.cout; ++co)
                        for (int e = 0; e < 8; ++e) {
                            const int c = c0 + g8 * 8 + e;
                            if (c < L.cin) pw[(g * L.coutp + co) * 8 + e] = a->conv_w[l][((size_t)co * L.cin + c) * T + t];
                        }
        }
        std::vector<float> bias(L.coutp, 0.f), sc(L.coutp, 1.f), sh(L.coutp, 0.f);
        for (int co = 0; co < L.cout; ++co) {
            if (a->bias) bias[co] = a->conv_b[l][co];
            if (a->batch_norm && !last) {
                // eval-mode BatchNorm as PyTorch evaluates it (conv.hip::pack_layer): y = x*alpha + (beta - mean*alpha)
                const float invstd = 1.0f / sqrtf(a->bn_var[l][co] + a->bn_eps);
                const float alpha = a->bn_gamma[l][co] * invstd;
                sc[co] = alpha;
                sh[co] = a->bn_beta[l][co] - a->bn_mean[l][co] * alpha;
            }
        }
        int rc;
        if ((rc = upload(L.w, pw)) || (rc = upload(L.bias, bias)) || (rc = upload(L.scale, sc)) || (rc = upload(L.shift, sh))) return rc;
    }
    return QGX_OK;
}

// Output tiles of 32 channels per workgroup: 2 where their number is even, else 1 (an odd count of 3, 5 or 7 tiles re-stages
// the patch once per tile rather than multiplying zero columns).  Four tiles per workgroup were compiled and dropped: 165
// VGPRs + 128 accumulator registers leave one wave per SIMD, against three with two tiles (101 + 64).
static int tiles_per_wg(int ntf) { return ntf % 2 == 0 ? 2 : 1; }

// Rows per workgroup: the most full-width rows that make at most 8 M-tiles of 32 pixels (two per wave), 12 (three per wave)
// where N divides 384 and not 256 (48, 96: with 8 the tile would be 6 M-tiles on 4 waves under a 3x halo — measured 1.6x the
// templated kernel on the 5x5 layer at 96 x 96); halved while the launch has fewer than 256 workgroups (small ensembles) —
// the tile shape does not enter the summation order, so the result does not depend on the member count
static int rows_generic(int B, int N, int ny) {
    const int cap = 256 % N == 0 ? 256 : 384;
    int best = 0;
    for (int R = 1; R <= N; ++R) {
        if (N % R || (R * N) % 32) continue;
        if (R * N > cap) break;
        best = R;
    }
    while (best > 1 && best % 2 == 0 && ((best / 2) * N) % 32 == 0 && (long)B * (N / best) * ny < 256) best /= 2;
    return best;
}
static size_t lds_generic(int R, int ks, int N) { return (size_t)(R + ks - 1) * N * G_STRIDE * sizeof(float); }

// What launch_convg asserts, for every layer of the net; no HIP call.  The grids are those of the shipped kernels (16, 32,
// 48, 64, 96, 128: choose_rows' whole row tiles), which is where the engine is tested; 192 would fit the LDS but is refused.
bool cnng_size_ok(const NetHost &net, int B, int N) {
    const int R0 = choose_rows(N);
    if (B < 1 || N < 16 || N > 128 || R0 <= 0 || N % R0) return false;
    if ((int64_t)B * N * N > (int64_t)1 << 29) return false;      // the int arithmetic of the grid size
    for (int l = 0; l < net.n_layers; ++l) {
        const LayerHost &L = net.L[l];
        const int ntf = L.coutp / 32, ny = ntf / tiles_per_wg(ntf);
        const int R = rows_generic(B, N, ny);
        if (R <= 0 || lds_generic(R, L.ks, N) > 160 * 1024) return false;
    }
    return true;
}

static int launch_convg(qgx_generator *g, int layer, const LayerHost &L, bool first, bool last, const float *in, float *out,
                        int B, int N, hipStream_t st) {
    ProfScope prof;
    if (const int prc = prof.begin(g, layer, st)) return prc;
    const int ntf = L.coutp / 32, nt = tiles_per_wg(ntf), ny = ntf / nt;
    const int R = rows_generic(B, N, ny);
    QGX_REQUIRE(R > 0 && N <= 128, "generator (generic engine): unsupported grid size N=%d", N);
    const size_t lds = lds_generic(R, L.ks, N);
    QGX_REQUIRE(lds <= 160 * 1024, "generator (generic engine): LDS patch %zu B too large for N=%d", lds, N);
    ConvGArgs a = {};
    a.in = in; a.out = out; a.w = L.w; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.N = N; a.R = R; a.ks = L.ks; a.cin = L.cin; a.cinp = L.cinp; a.coutp = L.coutp; a.cstore = L.cstore;
    a.planar_in = first; a.final = last;
    dim3 grid(B * (N / R), ny), block(256);
    auto kern = R * N / 32 > 8 ? (nt == 2 ? k_convg<2, 3> : k_convg<1, 3>) : (nt == 2 ? k_convg<2, 2> : k_convg<1, 2>);
    return launch_conv_kernel(kern, grid, block, lds, st, a);
}

// One convolution outside any generator handle (conv_train.hip): NHWC (B, N, N, cinp) in, NHWC (B, N, N, cstore) out,
// out = conv + bias; `w` packed as cnn_pack_net_arch packs a hidden layer ([group][coutp][8], one zero group at the end),
// `bias` [coutp].  The tile shapes are launch_convg's, so the summation order is that of the generator's layers.
bool convg_linear_ok(int64_t B, int N, int coutp, int ks) {
    const int R0 = choose_rows(N);
    if (B < 1 || N < 16 || N > 128 || R0 <= 0 || N % R0 || B * N * N > (int64_t)1 << 29) return false;
    const int ntf = coutp / 32, ny = ntf / tiles_per_wg(ntf);
    const int R = rows_generic((int)B, N, ny);
    return R > 0 && lds_generic(R, ks, N) <= 160 * 1024;
}
int launch_convg_linear(const float *in, float *out, const float *w, const float *bias, int B, int N, int cinp, int coutp,
                        int cstore, int ks, hipStream_t st) {
    QGX_REQUIRE(convg_linear_ok(B, N, coutp, ks), "conv2d (generic engine): N = %d is not supported (B = %d; 16, 32, 48, 64, 96 or 128)", N, B);
    const int ntf = coutp / 32, nt = tiles_per_wg(ntf), ny = ntf / nt;
    const int R = rows_generic(B, N, ny);
    ConvGArgs a = {};
    a.in = in; a.out = out; a.w = w; a.bias = bias; a.scale = nullptr; a.shift = nullptr;
    a.N = N; a.R = R; a.ks = ks; a.cin = cinp; a.cinp = cinp; a.coutp = coutp; a.cstore = cstore;
    a.planar_in = 0; a.final = 0;
    dim3 grid(B * (N / R), ny), block(256);
    auto kern = R * N / 32 > 8 ? (nt == 2 ? k_convg<2, 3, true> : k_convg<1, 3, true>) : (nt == 2 ? k_convg<2, 2, true> : k_convg<1, 2, true>);
    return launch_conv_kernel(kern, grid, block, lds_generic(R, ks, N), st, a);
}

// the n_layers convolutions: x planar (B, n_in, N, N) -> y planar (B, n_out, N, N); activations alternate actA, actB
int cnng_convs(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N, hipStream_t st) {
    QGX_REQUIRE(cnng_size_ok(net, B, N), "generator (generic engine): N = %d is not supported (B = %d; 16, 32, 48, 64, 96 or 128)", N, B);
    const Workspace &w = g->work();
    QGX_REQUIRE(w.actA && w.actB && w.cap_elems >= (size_t)B * N * N && g->actw[0] >= net.act_width(0) && g->actw[1] >= net.act_width(1),
                "generator (generic engine): the activation buffers are not reserved for this net");
    const float *in = x;
    for (int l = 0; l < net.n_layers; ++l) {
        const bool last = l == net.n_layers - 1;
        float *out = last ? y : (l & 1 ? w.actB : w.actA);
        if (const int rc = launch_convg(g, l, net.L[l], l == 0, last, in, out, B, N, st)) return rc;
        in = out;
    }
    return QGX_OK;
}

}  // namespace qgx
