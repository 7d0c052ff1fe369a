// The flux head of AndrewCNN(div=True) (tools/cnn_tools.py:100-123, 170-175): the last convolution of such a net writes the
// fluxes F (B, 4, N, N) = [fx of layer 1, fx of layer 2, fy of layer 1, fy of layer 2], and forward returns
//   y = 10000 irfftn(ik rfftn(fx) + il rfftn(fy)),   float32, ik / il = complex64 of pyqg.QGModel(nx = N)'s grid lines, L = 1e6.
//
// One workgroup per (member, layer), the whole field resident in LDS as ONE complex float32 array z = fx + i fy (at 128 x 128
// a padded field is 132 KB of the 160 KB: a second one does not fit).  Forward 2-D FFT; the spectra of the two real fields are
// separated from Z(l,k) and conj Z(-l,-k) as spectral_pack.hpp does, multiplied and recombined per conjugate pair, in place;
// inverse FFT; the real part is the output.  No atomics, no second kernel, no host call.
//
// What irfftn(ik X + il Y) computes is NOT the naive full-plane multiply: the c2r transform drops the imaginary part of the
// self-conjugate bins, and pyqg's l at the Nyquist row is -N/2 dk while k at the Nyquist column is +N/2 dk.  The equivalent
// Hermitian multipliers on the full plane (l, k in fftfreq order) are
//   Hx(l,k) = i dk k, and 0 on the column k = +-N/2;
//   Hy(l,k) = i dk l for l != N/2; on the row l = N/2: i dk (-N/2) sign(k), and 0 at k = 0 and k = N/2
// (tests/div_restatement.py states both forms and checks that they agree to 1e-12 in float64).
#include "generator.hpp"
#include "fft_lds_f32.hpp"

namespace qgx {

extern __shared__ __attribute__((aligned(16))) unsigned char fluxdiv_smem[];

constexpr int fluxdiv_threads(int N) { return N >= 64 ? 1024 : 256; }
constexpr size_t fluxdiv_lds_bytes(int N) { return (size_t)N * (N + 1) * sizeof(float2) + N * sizeof(float2) + N * sizeof(int); }

template <int N>
__global__ __launch_bounds__(fluxdiv_threads(N)) void k_fluxdiv(const float *__restrict__ F, float *__restrict__ y) {
    constexpr int LD = N + 1, H = N / 2;
    float2 *Z = reinterpret_cast<float2 *>(fluxdiv_smem);      // [N][LD]
    float2 *tw = Z + N * LD;                                     // exp(-2 pi i j / N), j < N
    int *pos = reinterpret_cast<int *>(tw + N);                  // where the forward transform leaves frequency j
    const int b = blockIdx.x >> 1, c = blockIdx.x & 1;
    const float *fx = F + ((size_t)b * 4 + c) * N * N, *fy = fx + 2 * (size_t)N * N;
    for (int i = threadIdx.x; i < N * N / 4; i += blockDim.x) {  // N % 4 == 0: a quad stays in its row
        const float4 a = reinterpret_cast<const float4 *>(fx)[i], d = reinterpret_cast<const float4 *>(fy)[i];
        const int r = 4 * i / N, col = 4 * i - r * N;
        float2 *z = Z + r * LD + col;
        z[0] = make_float2(a.x, d.x); z[1] = make_float2(a.y, d.y); z[2] = make_float2(a.z, d.z); z[3] = make_float2(a.w, d.w);
    }
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        double s, co;
        sincospi(-2.0 * j / N, &s, &co);                         // rounded ONCE from float64
        tw[j] = make_float2((float)co, (float)s);
        pos[j] = fft32::freq_pos(j, N);
    }
    __syncthreads();
    fft32::fft2d_fwd<N>(Z, tw);
    // every conjugate pair {(l,k), (-l,-k)} once: k = 0 .. N/2, and on the two self-paired columns l <= -l (mod N) only
    const double dk = 6.283185307179586 / 1e6;
    for (int w = threadIdx.x; w < N * (H + 1); w += blockDim.x) {
        const int l = w / (H + 1), k = w - l * (H + 1);
        const int lm = l ? N - l : 0, km = k ? N - k : 0;
        if ((k == 0 || k == H) && l > lm) continue;
        float2 *pa = Z + pos[l] * LD + pos[k], *pb = Z + pos[lm] * LD + pos[km];
        const float2 A = *pa, Bc = make_float2(pb->x, -pb->y);
        // X = (A + conj B) / 2, Y = (A - conj B) / (2 i): the spectra of fx and fy at (l, k)
        const float2 X = make_float2(0.5f * (A.x + Bc.x), 0.5f * (A.y + Bc.y));
        const float2 Y = make_float2(0.5f * (A.y - Bc.y), -0.5f * (A.x - Bc.x));
        const float wk = k == H ? 0.f : (float)(dk * (double)k);
        const float wl = l != H ? (float)(dk * (double)(l < H ? l : l - N)) : ((k == 0 || k == H) ? 0.f : (float)(dk * (double)(-H)));
        const float2 t = make_float2(X.x * wk + Y.x * wl, X.y * wk + Y.y * wl);
        const float2 D = make_float2(-t.y, t.x);                 // i t
        *pa = D;
        *pb = make_float2(D.x, -D.y);                            // (a self-paired bin: D = 0 there, both multipliers vanish)
    }
    __syncthreads();
    fft32::fft2d_inv<N>(Z, tw);
    float *out = y + ((size_t)b * 2 + c) * N * N;
    constexpr float inv = 1.0f / (float)(N * N);
    for (int i = threadIdx.x; i < N * N; i += blockDim.x) {
        const int r = i / N, col = i - r * N;
        out[i] = 10000.f * (Z[r * LD + col].x * inv);
    }
}

bool fluxdiv_size_ok(int N) { return N == 16 || N == 32 || N == 48 || N == 64 || N == 96 || N == 128; }

template <int N>
static int launch_fluxdiv(const float *F, float *y, int B, hipStream_t st, bool prepare_only) {
    // above 64 KB of dynamic LDS the cap is raised once per device and host thread (never per launch: host time)
    static thread_local bool raised[16] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    constexpr size_t lds = fluxdiv_lds_bytes(N);
    static_assert(lds <= 160 * 1024, "the padded field must fit in LDS");
    if (!raised[dev & 15]) {
        QGX_HIP(hipFuncSetAttribute((const void *)k_fluxdiv<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised[dev & 15] = true;
    }
    if (prepare_only) return QGX_OK;
    hipLaunchKernelGGL(k_fluxdiv<N>, dim3(2 * B), dim3(fluxdiv_threads(N)), lds, st, F, y);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

static int fluxdiv_dispatch(const float *F, float *y, int B, int N, hipStream_t st, bool prepare_only) {
    switch (N) {
    case 16: return launch_fluxdiv<16>(F, y, B, st, prepare_only);
    case 32: return launch_fluxdiv<32>(F, y, B, st, prepare_only);
    case 48: return launch_fluxdiv<48>(F, y, B, st, prepare_only);
    case 64: return launch_fluxdiv<64>(F, y, B, st, prepare_only);
    case 96: return launch_fluxdiv<96>(F, y, B, st, prepare_only);
    case 128: return launch_fluxdiv<128>(F, y, B, st, prepare_only);
    }
    QGX_REQUIRE(false, "flux-form net: no divergence kernel for N = %d (16, 32, 48, 64, 96 or 128)", N);
}

// at handle creation, outside any captured region: the LDS caps of every size
int fluxdiv_prepare() {
    for (int N : {16, 32, 48, 64, 96, 128})
        if (const int rc = fluxdiv_dispatch(nullptr, nullptr, 0, N, nullptr, true)) return rc;
    return QGX_OK;
}

int fluxdiv_forward(const float *F, float *y, int B, int N, hipStream_t st) {
    QGX_REQUIRE(F && y && B > 0 && B <= INT32_MAX / 2, "fluxdiv_forward: bad argument");
    return fluxdiv_dispatch(F, y, B, N, st, false);
}

}  // namespace qgx
