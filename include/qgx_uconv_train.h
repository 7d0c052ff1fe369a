/* qgx_uconv_train.h — the circular convolution of the DeepInversion U-Net's training and its two gradients: Conv2d(cin, cout,
 * k, padding=k/2, padding_mode='circular') with k 1 or 3 on any grid from 2 x 2 to 128 x 128 and up to 512 -> 1024 channels:
 * the U-Net's 3 x 3 and 1 x 1 layers at N, N/2, ..., N/16, and its ConvTranspose2d(C, C/2, 2, stride=2) as a 1 x 1 product
 * with 4 C/2 outputs (tools/train_ops.py wraps the three calls in a once-differentiable torch.autograd.Function).
 * Included by qgx.h (which declares the status codes); not meant to be included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle.
 *   activations and their gradients   NHWC float32 (B, N, N, C8), C8 = channels rounded up to 8: the engine layout of
 *                                     qgx_conv_train.h.  Channels C ... C8 - 1 must be zero on input (the caller's duty) and
 *                                     are written as zero on output
 *   weights and their gradients       PyTorch's layout: (cout, cin, k, k) and (cout), float32
 * Admitted: N any integer 2 ... 128, k 1 or 3, cin 1 ... 512, cout 1 ... 1024, B >= 1 with B N N <= 2^29.  At N = 2 the taps
 * ky = 0 and ky = 2 reach the same row, which is what torch's circular padding computes.  Anything else, a null pointer (but
 * those said to be optional), a misaligned pointer or a workspace of fewer bytes than qgx_uconv2d_workspace gives returns
 * QGX_ERR_INVALID with a message naming the field, before any device call.
 *
 * The workspace (one size for the three calls of a shape) holds the weights as the kernels read them and the weight
 * gradient's partial sums; its contents mean nothing between calls, and two calls that share one may not run concurrently.
 *
 * Results are bitwise repeatable and do not depend on the stream.  y sums over (tap, input channel) in order (taps row by
 * row, channels ascending, in steps of two on the matrix cores) and adds the bias last; dx is the same sum over (tap, output
 * channel) of dy with the flipped, transposed weights.  dw's sum over the B N N pixels (b, y, x in order) is cut into units
 * of 32 pixels and the units into S shares of consecutive units, S a fixed function of (B, N, cin, cout, k); a workgroup
 * walks its share in order into its own slice of the workspace, and a second kernel adds the slices in a fixed order: eight
 * partial sums over the shares q, q + 8, ..., then those eight in order.  With S = 1 (a large dw, few pixels) the one share is
 * stored directly and no second kernel runs.  db is one running sum over a share's pixels in order, and the shares' sums are
 * added as dw's are.  There are no float atomics. */
#ifndef QGX_UCONV_TRAIN_H
#define QGX_UCONV_TRAIN_H

int qgx_uconv2d_workspace(int64_t B, int N, int cin, int cout, int k, size_t *bytes);

/* y (B, N, N, cout8) = conv_circular(x (B, N, N, cin8), w) + bias; bias_dev may be NULL (no bias); no activation */
int qgx_uconv2d_forward(const float *x_dev, const float *w_dev, const float *bias_dev, float *y_dev, int64_t B, int N, int cin,
                        int cout, int k, void *work_dev, size_t work_bytes, void *stream);

/* dx[b, ci, y, x] = sum over co, ky, kx of dy[b, co, y - ky + P, x - kx + P] w[co, ci, ky, kx], P = k / 2, indices mod N */
int qgx_uconv2d_backward_data(const float *dy_dev, const float *w_dev, float *dx_dev, int64_t B, int N, int cin, int cout, int k,
                              void *work_dev, size_t work_bytes, void *stream);

/* dw[co, ci, ky, kx] = sum over b, y, x of dy[b, co, y, x] x[b, ci, y + ky - P, x + kx - P]; db[co] = sum of dy[b, co, y, x]
 * (db_dev may be NULL: not computed, nothing written) */
int qgx_uconv2d_backward_weight(const float *x_dev, const float *dy_dev, float *dw_dev, float *db_dev, int64_t B, int N, int cin,
                                int cout, int k, void *work_dev, size_t work_bytes, void *stream);

#endif
