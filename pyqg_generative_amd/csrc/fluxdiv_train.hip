// The flux head of a flux-form net in a training step (include/qgx_flux_train.h): y = 10000 div F in the engine layout, and the
// adjoint dF = D^T dy in both layouts.  The arithmetic is fluxdiv_core.hpp's: the forward is the body of the generators'
// k_fluxdiv with the engine's loads and stores, the backward one forward transform of g1 + i g2, a pointwise multiply by
// conj(Hx) or conj(Hy) and one inverse per (sample, direction).  One launch each, no atomics, no workspace.
//
//   k_fluxdiv_engine     workgroup (b, layer):     reads 16 bytes of each F record, writes y1 or y2 and its share of the pads
//   k_fluxdiv_adjoint    workgroup (b, direction): reads 8 bytes of each dy record (engine) or the two planes (planar), writes
//                        (dfx1, dfx2) or (dfy1, dfy2); the direction-x workgroup zeroes channels 4 ... 7
//
// Registers (the compiler's resource usage at -O3 for gfx950) are listed in DESIGN 3.21; no instantiation uses scratch.
#include "generator.hpp"
#include "fluxdiv_core.hpp"

namespace qgx {

extern __shared__ __attribute__((aligned(16))) unsigned char fluxtrain_smem[];

template <int N>
__global__ __launch_bounds__(fluxdiv_threads(N)) void k_fluxdiv_engine(const float *__restrict__ F, float *__restrict__ y) {
    fluxdiv_body<N, QGX_FLUX_ENGINE>(F, y, fluxtrain_smem);
}

template <int N, int LAYOUT>
__global__ __launch_bounds__(fluxdiv_threads(N)) void k_fluxdiv_adjoint(const float *__restrict__ dy, float *__restrict__ dF) {
    fluxdiv_adjoint<N, LAYOUT>(dy, dF, fluxtrain_smem);
}

// one launch of 2 B workgroups; above 64 KB of dynamic LDS the cap of THIS instantiation is raised once per device and host
// thread (never per launch: host time)
template <int N, void (*KERN)(const float *, float *)>
static int launch_flux(const float *in, float *out, int B, hipStream_t st) {
    static thread_local bool raised[16] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    constexpr size_t lds = fluxdiv_lds_bytes(N);
    static_assert(lds <= 160 * 1024, "the padded field must fit in LDS");
    if (!raised[dev & 15]) {
        QGX_HIP(hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised[dev & 15] = true;
    }
    hipLaunchKernelGGL(KERN, dim3(2 * B), dim3(fluxdiv_threads(N)), lds, st, in, out);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}

template <int N>
static int flux_forward_engine(const float *F, float *y, int B, hipStream_t st) {
    return launch_flux<N, k_fluxdiv_engine<N>>(F, y, B, st);
}
template <int N>
static int flux_backward(const float *dy, float *dF, int B, int layout, hipStream_t st) {
    if (layout == QGX_FLUX_PLANAR) return launch_flux<N, k_fluxdiv_adjoint<N, QGX_FLUX_PLANAR>>(dy, dF, B, st);
    return launch_flux<N, k_fluxdiv_adjoint<N, QGX_FLUX_ENGINE>>(dy, dF, B, st);
}

static bool flux_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
#define FLUX_PTR(what, p)                                                                                  \
    do {                                                                                                   \
        QGX_REQUIRE(p, "%s: " #p " is NULL", what);                                                        \
        QGX_REQUIRE(flux_aligned16(p), "%s: " #p " is not 16-byte aligned", what);                         \
    } while (0)

static int flux_check(const char *what, int64_t B, int N, int layout) {
    QGX_REQUIRE(fluxdiv_size_ok(N), "%s: N = %d, expected 16, 32, 48, 64, 96 or 128", what, N);
    QGX_REQUIRE(B >= 1 && B <= INT32_MAX / 2, "%s: B = %lld, expected 1 ... %d", what, (long long)B, INT32_MAX / 2);
    QGX_REQUIRE(layout == QGX_FLUX_PLANAR || layout == QGX_FLUX_ENGINE, "%s: layout = %d, expected QGX_FLUX_PLANAR (0) or QGX_FLUX_ENGINE (1)", what, layout);
    return QGX_OK;
}

}  // namespace qgx

using namespace qgx;

extern "C" {

int qgx_fluxdiv_forward(const float *F_dev, float *y_dev, int64_t B, int N, int layout, void *stream) {
    const char *what = "qgx_fluxdiv_forward";
    if (const int rc = flux_check(what, B, N, layout)) return rc;
    FLUX_PTR(what, F_dev); FLUX_PTR(what, y_dev);
    hipStream_t st = (hipStream_t)stream;
    if (layout == QGX_FLUX_PLANAR) return fluxdiv_forward(F_dev, y_dev, (int)B, N, st);      // the generators' own call
    switch (N) {
    case 16: return flux_forward_engine<16>(F_dev, y_dev, (int)B, st);
    case 32: return flux_forward_engine<32>(F_dev, y_dev, (int)B, st);
    case 48: return flux_forward_engine<48>(F_dev, y_dev, (int)B, st);
    case 64: return flux_forward_engine<64>(F_dev, y_dev, (int)B, st);
    case 96: return flux_forward_engine<96>(F_dev, y_dev, (int)B, st);
    default: return flux_forward_engine<128>(F_dev, y_dev, (int)B, st);
    }
}

int qgx_fluxdiv_backward(const float *dy_dev, float *dF_dev, int64_t B, int N, int layout, void *stream) {
    const char *what = "qgx_fluxdiv_backward";
    if (const int rc = flux_check(what, B, N, layout)) return rc;
    FLUX_PTR(what, dy_dev); FLUX_PTR(what, dF_dev);
    hipStream_t st = (hipStream_t)stream;
    switch (N) {
    case 16: return flux_backward<16>(dy_dev, dF_dev, (int)B, layout, st);
    case 32: return flux_backward<32>(dy_dev, dF_dev, (int)B, layout, st);
    case 48: return flux_backward<48>(dy_dev, dF_dev, (int)B, layout, st);
    case 64: return flux_backward<64>(dy_dev, dF_dev, (int)B, layout, st);
    case 96: return flux_backward<96>(dy_dev, dF_dev, (int)B, layout, st);
    default: return flux_backward<128>(dy_dev, dF_dev, (int)B, layout, st);
    }
}

}  // extern "C"
