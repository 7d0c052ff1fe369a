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
#include "fluxdiv_core.hpp"

namespace qgx {

extern __shared__ __attribute__((aligned(16))) unsigned char fluxdiv_smem[];

// the body (load, FFT, pair multiply, inverse, scale, store) is fluxdiv_core.hpp's: the training step's forward in the engine
// layout (fluxdiv_train.hip) is a second instantiation of the same function
template <int N>
__global__ __launch_bounds__(fluxdiv_threads(N)) void k_fluxdiv(const float *__restrict__ F, float *__restrict__ y) {
    fluxdiv_body<N, QGX_FLUX_PLANAR>(F, y, fluxdiv_smem);
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
