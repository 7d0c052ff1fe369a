/* qgx_train.h — training of ANNModel's pointwise stencil network of the qgx C ABI.  Included by qgx.h (which declares
 * qgx_ann_weights and the status codes); not meant to be included on its own. */
#ifndef QGX_TRAIN_H
#define QGX_TRAIN_H

/* Stencil rows of single-channel images (reference: tools/cnn_tools.py:321-339 xarray_to_stencil), a pure copy:
 *   img_dev  (n_img, N, N) float          rows_dev (R, s * s) float,  R = ceil(N / step)^2 * n_img
 *   row ((j / step) * ceil(N / step) + i / step) * n_img + img, j and i the multiples of step below N, holds at feature
 *   dy * s + dx the value at ((j + dy - s / 2) mod N, (i + dx - s / 2) mod N) of image img.
 * s = 1 gives the reference's target rows.  QGX_ERR_INVALID before any device call: null pointers, n_img < 1, N < 1, an
 * even s or one outside 1 ... 7, step < 1. */
int qgx_ann_rows(const float *img_dev, int64_t n_img, int N, int s, int step, float *rows_dev, void *stream);

/* The trainer owns, on `device`, the parameters (initialised from `init`, every shape qgx_generator_create_ann admits), the
 * gradient, Adam's first and second moments, Adam's step count and the work space of the per-workgroup partial sums.
 * Parameters, gradient and moments are packed in state-dict order: layers.0.weight (out, in), layers.0.bias, layers.2.weight,
 * ...; qgx_ann_trainer_size gives the number of floats. */
typedef struct qgx_ann_trainer qgx_ann_trainer;
enum qgx_ann_trainer_what { QGX_TRAIN_PARAMS = 0, QGX_TRAIN_GRAD = 1, QGX_TRAIN_M = 2, QGX_TRAIN_V = 3 };
int qgx_ann_trainer_create(const qgx_ann_weights *init, int device, qgx_ann_trainer **out);
int qgx_ann_trainer_destroy(qgx_ann_trainer *t);
int64_t qgx_ann_trainer_size(const qgx_ann_trainer *t);            /* floats of one packed vector; -1: null handle */

/* Loss and gradient of one batch: rows idx_dev[0 .. n) (int64) of x_rows_dev (R, s * s) and y_rows_dev (R) float; inputs
 * row / x_scale, targets y / y_scale (float32 divisions, ann_model.py:40-43); loss = mean over the batch of (net(x) - y)^2
 * (scale_invariant: net(x) = |x|^2 layers(x / |x|); a zero stencil gives NaN as in torch).  The handle's gradient receives
 * d loss / d theta.  loss_acc_dev (two doubles, or NULL): [0] += sum over the rows of (net(x) - y)^2, [1] += n, so an epoch's
 * loss is read back once.  The values of idx_dev are the CALLER's responsibility: they are not checked against R (an index
 * outside 0 ... R - 1 reads outside the row buffers).
 * Results are bitwise repeatable and do not depend on the stream: the batch is cut into fixed tiles of rows, a tile's
 * sums run over its rows in order, a workgroup adds its tiles in order, and the workgroups' partial sums are added in a
 * fixed order; there are no float atomics.
 * _adam: one torch.optim.Adam step with torch's defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) on the
 * gradient as it stands, in torch's order: bias corrections as host doubles, denom = sqrt(v) / sqrt(bc2) + eps,
 * p -= (lr / bc1) m / denom.  _step: _grad then _adam, bitwise, in two launches and with no host synchronisation.
 * _loss: forward only (evaluate_test); idx_dev may be NULL for rows 0 ... n - 1; loss_acc_dev as above and required.
 * Calls on one handle may not run concurrently.
 * QGX_ERR_INVALID before any device call: null pointers (but those said to be optional), n < 1, a non-finite or
 * non-positive scale, a non-finite or negative lr. */
int qgx_ann_trainer_grad(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                         int64_t n, float x_scale, float y_scale, double *loss_acc_dev, void *stream);
int qgx_ann_trainer_adam(qgx_ann_trainer *t, double lr, void *stream);
int qgx_ann_trainer_step(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                         int64_t n, float x_scale, float y_scale, double lr, double *loss_acc_dev, void *stream);
int qgx_ann_trainer_loss(qgx_ann_trainer *t, const float *x_rows_dev, const float *y_rows_dev, const int64_t *idx_dev,
                         int64_t n, float x_scale, float y_scale, double *loss_acc_dev, void *stream);

/* Packed vector `what` (enum qgx_ann_trainer_what) to / from `host` (qgx_ann_trainer_size floats); both synchronise with the
 * device.  _write with adam_steps >= 0 also sets Adam's step count (the number of steps taken so far); adam_steps < 0 leaves
 * it.  QGX_ERR_INVALID before any device call: null pointers, `what` out of range. */
int qgx_ann_trainer_read(qgx_ann_trainer *t, int what, float *host);
int qgx_ann_trainer_write(qgx_ann_trainer *t, int what, const float *host, int64_t adam_steps);

#endif
