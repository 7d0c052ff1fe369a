/* qgx_dconv_train.h — the stride-2 convolution of a DCGAN discriminator and its two gradients: Conv2d(cin, cout, 4, stride=2,
 * padding=1, bias=False) with ZERO padding, the layer operation CGANRegression's critic is made of (tools/train_ops.py wraps
 * the three calls in torch.autograd.Functions whose backwards are each other, so the layer is differentiable twice).
 * Included by qgx.h (which declares the status codes); not meant to be included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle.
 *   x, dx     NHWC float32 (B, N, N, C8(cin)),  C8 = channels rounded up to 8: the engine layout of qgx_conv_train.h
 *   y, dy     NHWC float32 (B, N/2, N/2, C8(cout))
 *             Pad channels must be zero on input (the caller's duty) and are written as zero on output.
 *   w, dw     PyTorch's layout (cout, cin, 4, 4), float32; there is no bias
 *   y[b, co, i, j] = sum over ci, ky, kx of x[b, ci, 2i - 1 + ky, 2j - 1 + kx] w[co, ci, ky, kx], terms outside the image zero
 * Admitted: N even, 2 ... 128; cin and cout 1 ... 512; B >= 1 with B N N <= 2^29.  Anything else, a null or misaligned
 * pointer, or a workspace of fewer bytes than qgx_dconv2d_workspace gives returns QGX_ERR_INVALID with a message naming the
 * field, before any device call.
 *
 * The workspace (one size for the three calls of a shape) holds the weights as the kernels read them and the weight
 * gradient's partial sums; its contents mean nothing between calls, and two calls that share one may not run concurrently.
 *
 * Results are bitwise repeatable and do not depend on the stream.  y sums over (tap, channel) in order; dx is four parity
 * classes of a 2 x 2-tap convolution over dy (row 2i + p of dx receives ky in {1, 3} for p = 0, {2, 0} for p = 1, from the
 * output rows i and i -+ 1) and sums over (tap of the class, channel) in order; dw's sum over the B (N/2)^2 output pixels is
 * cut into shares that are a fixed function of (B, N, cin, cout), a workgroup walks its share in order into its own slice of
 * the workspace, and a second kernel adds the slices in a fixed order.  There are no float atomics. */
#ifndef QGX_DCONV_TRAIN_H
#define QGX_DCONV_TRAIN_H

int qgx_dconv2d_workspace(int64_t B, int N, int cin, int cout, size_t *bytes);

/* y (B, N/2, N/2, cout8) = conv(x (B, N, N, cin8), w; stride 2, zero padding 1) */
int qgx_dconv2d_forward(const float *x_dev, const float *w_dev, float *y_dev, int64_t B, int N, int cin, int cout,
                        void *work_dev, size_t work_bytes, void *stream);

/* dx[b, ci, r, s] = sum over co, ky, kx with r = 2i - 1 + ky, s = 2j - 1 + kx of dy[b, co, i, j] w[co, ci, ky, kx] */
int qgx_dconv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout,
                              void *work_dev, size_t work_bytes, void *stream);

/* dw[co, ci, ky, kx] = sum over b, i, j of dy[b, co, i, j] x[b, ci, 2i - 1 + ky, 2j - 1 + kx] */
int qgx_dconv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, int64_t B, int N, int cin, int cout,
                                void *work_dev, size_t work_bytes, void *stream);

#endif
