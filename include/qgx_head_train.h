/* qgx_head_train.h — the two ends of a training step of the convolutional nets of the qgx C ABI: the batch gather in front of
 * the first convolution and the loss head behind the last one (tools/train_CNN.py wraps them; MeanVarModel's fit is built on
 * them).  Included by qgx.h (which declares the status codes); not meant to be included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle.
 *   engine layout   NHWC float32 (B, N, N, 8): the layout of qgx_conv_train.h for 1 ... 8 channels; one pixel is a record of 8
 *                   floats, channels C ... 7 zero.  Outputs in this layout get their pad channels WRITTEN as zero
 *   planar          (n, C, N, N) float32, PyTorch's layout of a data set held on the device
 *   idx_dev         int64 (B), or NULL: batch member b is row idx[b] of the planar array (NULL: row b, and then n >= B).
 *                   0 <= idx[b] < n is the CALLER'S DUTY: the indices are on the device and no call reads them back
 *                   (tools/train_CNN.py checks an epoch's permutation on the host before it uploads it)
 * Admitted: N 16, 32, 48, 64, 96 or 128, B >= 1 with B N N <= 2^29, C 1 ... 8, n >= 1.  Anything else, a null pointer (but
 * those said to be optional), a misaligned pointer, an unknown mode or a workspace of fewer bytes than qgx_head_workspace gives
 * returns QGX_ERR_INVALID with a message naming the field, before any device call.
 *
 * The head h of a mode:
 *   QGX_HEAD_MSE            h(y) = y,  h'(y) = 1
 *   QGX_HEAD_SOFTPLUS_MSE   h(y) = y if y > 20, else log1p(exp(y))  (torch's softplus, beta 1, threshold 20),
 *                           h'(y) = 1 if y > 20, else exp(y) / (1 + exp(y))
 * h, h' and the difference h(y) - t are float32.
 *
 * Results are bitwise repeatable and do not depend on the stream: the loss's sum over the B N N pixels is cut into ranges that
 * are a fixed function of (B, N); a workgroup adds the squares of its range in float64, in a fixed order, into its own slot of
 * the workspace, and a second kernel adds the slots in a fixed order and divides once.  There are no float atomics. */
#ifndef QGX_HEAD_TRAIN_H
#define QGX_HEAD_TRAIN_H

enum qgx_head_mode { QGX_HEAD_MSE = 0, QGX_HEAD_SOFTPLUS_MSE = 1 };

/* out (B, N, N, 8) engine layout = src[idx[b]] of the planar src (n, C, N, N): X[idx], the zero fill and the permuted copy in
 * one launch */
int qgx_batch_gather(const float *src_dev, const int64_t *idx_dev, float *out_dev, int64_t n, int64_t B, int N, int C,
                     void *stream);

/* bytes of the workspace of qgx_head_loss: the float64 partial sums, a function of (B, N) alone */
int qgx_head_workspace(int64_t B, int N, size_t *bytes);

/* *loss_dev (one float64) = sum over b, c < C, y, x of (h(y[b, y, x, c]) - t[idx[b], c, y, x])^2 / (B C N N): the difference
 * is float32, its square and every sum float64.  The workspace's contents mean nothing between calls, and two calls that
 * share one may not run concurrently */
int qgx_head_loss(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, double *loss_dev, int64_t B, int N,
                  int C, int64_t n, void *work_dev, size_t work_bytes, void *stream);

/* dy (B, N, N, 8) engine layout = s (h(y) - t) h'(y), the gradient of qgx_head_loss's value times *gout_dev (one float64, the
 * loss's incoming gradient, read on the device): s = float32(gout * 2 / (B C N N)), formed in float64 and rounded once; the
 * products are float32, (s (h(y) - t)) h'(y) in this order.  Recomputed from y and t: the loss call saves nothing */
int qgx_head_grad(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, const double *gout_dev,
                  float *dy_dev, int64_t B, int N, int C, int64_t n, void *stream);

/* out planar (B, C, N, N) = h(y) if t_dev is NULL (the planar forward output of a net; idx_dev and n are then not used), else
 * (t[idx[b]] - h(y))^2 in float32: the squared residuals MeanVarModel's variance net is trained on */
int qgx_head_apply(const float *y_dev, const float *t_dev, const int64_t *idx_dev, int mode, float *out_dev, int64_t B, int N,
                   int C, int64_t n, void *stream);

#endif
