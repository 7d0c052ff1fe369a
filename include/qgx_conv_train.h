/* qgx_conv_train.h — a differentiable circular convolution of the qgx C ABI: the layer operation AndrewCNN's training is
 * made of (tools/train_CNN.py wraps the three calls in a torch.autograd.Function).  Included by qgx.h (which declares the
 * status codes); not meant to be included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle.
 *   activations and their gradients   NHWC float32 (B, N, N, C8), C8 = channels rounded up to 8: the generic engine's layout
 *                                     (conv_generic.hip) and torch's channels_last memory of a (B, C8, N, N) tensor.  Channels
 *                                     C ... C8 - 1 must be zero on input (the caller's duty) and are written as zero on output
 *   weights and their gradients       PyTorch's layout: (cout, cin, k, k) and (cout), float32
 * Admitted: N 16, 32, 48, 64, 96 or 128 (the engine's grids), cin and cout 1 ... 256, k 3 or 5, B >= 1 with B N N <= 2^29.
 * Anything else, a null pointer (but those said to be optional), a misaligned pointer or a workspace of fewer bytes than
 * qgx_conv2d_workspace gives returns QGX_ERR_INVALID with a message naming the field, before any device call.
 *
 * The workspace (one size for the three calls of a shape) holds the weights as the convolution kernel reads them, the padded
 * bias and the weight gradient's partial sums; its contents mean nothing between calls, and two calls that share one may not
 * run concurrently.
 *
 * Results are bitwise repeatable and do not depend on the stream: a convolution's sum runs over (chunk of 32 input channels,
 * tap, channel) in order; the weight gradient's sum over the B N N pixels is cut into shares that are a fixed function of
 * (B, N, cin, cout, k), a workgroup walks its share in order into its own slice of the workspace, and a second kernel adds
 * the slices in a fixed order.  There are no float atomics. */
#ifndef QGX_CONV_TRAIN_H
#define QGX_CONV_TRAIN_H

int qgx_conv2d_workspace(int64_t B, int N, int cin, int cout, int k, size_t *bytes);

/* y (B, N, N, cout8) = conv_circular(x (B, N, N, cin8), w) + bias; bias_dev may be NULL (no bias); no activation */
int qgx_conv2d_forward(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t B, int N, int cin,
                       int cout, int k, void *work_dev, size_t work_bytes, void *stream);

/* dx[b, ci, y, x] = sum over co, ky, kx of dy[b, co, y - ky + P, x - kx + P] w[co, ci, ky, kx], P = k / 2: the forward
 * convolution of dy with the flipped, transposed weights */
int qgx_conv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout, int k,
                             void *work_dev, size_t work_bytes, void *stream);

/* dw[co, ci, ky, kx] = sum over b, y, x of dy[b, co, y, x] x[b, ci, y + ky - P, x + kx - P]; db[co] = sum of dy[b, co, y, x]
 * (db_dev may be NULL: not computed) */
int qgx_conv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, float *db_dev, int64_t B, int N, int cin,
                               int cout, int k, void *work_dev, size_t work_bytes, void *stream);

#endif
