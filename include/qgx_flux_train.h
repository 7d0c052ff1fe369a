/* qgx_flux_train.h — the flux head of a flux-form net, AndrewCNN(div=True), as a differentiable operation of the qgx C ABI:
 * y = 10000 divergence(F) and its adjoint (tools/train_ops.py wraps the two calls in a torch.autograd.Function;
 * tools/train_CNN.py's FluxFormCNN ends in it).  Included by qgx.h (which declares the status codes); not meant to be
 * included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle and no workspace.
 *
 * The operator, per sample and layer c = 1, 2 (float32, spectral, pyqg's grid lines at L = 1e6):
 *   y_c = 10000 irfftn(ik rfftn(fx_c) + il rfftn(fy_c)) = 10000 ifft2(Hx fft2(fx_c) + Hy fft2(fy_c))
 * with the Hermitian multipliers Hx, Hy of csrc/fluxdiv.hip's header comment; its adjoint is
 *   dfx_c = 10000 ifft2(conj(Hx) fft2(g_c)),   dfy_c = 10000 ifft2(conj(Hy) fft2(g_c)).
 * The forward is the kernel body the generators run at inference (one device function, instantiated per layout): a net
 * trained through these calls is trained on the forward that its inference computes, bit for bit.
 *
 *   QGX_FLUX_PLANAR   F and dF (B, 4, N, N) = [fx1, fx2, fy1, fy2], y and dy (B, 2, N, N): PyTorch's layout
 *   QGX_FLUX_ENGINE   NHWC (B, N, N, 8), the layout of qgx_conv_train.h: F and dF records [fx1, fx2, fy1, fy2, 0, 0, 0, 0],
 *                     y and dy records [y1, y2, 0, 0, 0, 0, 0, 0].  Of an input record only channels 0 ... 3 (F) or 0, 1 (dy)
 *                     are read; every byte of an output is written exactly once, the pad channels as zero
 * Admitted: N 16, 32, 48, 64, 96 or 128, B >= 1 with 2 B <= INT32_MAX.  Anything else, a null pointer, a misaligned pointer
 * or an unknown layout returns QGX_ERR_INVALID with a message naming the field, before any device call.
 *
 * Results are bitwise repeatable and do not depend on the stream, the batch or the layout: one workgroup owns a (sample, layer)
 * of the forward and a (sample, direction) of the backward, with the whole field in LDS.  There are no atomics. */
#ifndef QGX_FLUX_TRAIN_H
#define QGX_FLUX_TRAIN_H

enum qgx_flux_layout { QGX_FLUX_PLANAR = 0, QGX_FLUX_ENGINE = 1 };

/* y = 10000 divergence(F) */
int qgx_fluxdiv_forward(const float *F_dev, float *y_dev, int64_t B, int N, int layout, void *stream);

/* dF = the adjoint of qgx_fluxdiv_forward applied to dy */
int qgx_fluxdiv_backward(const float *dy_dev, float *dF_dev, int64_t B, int N, int layout, void *stream);

#endif
