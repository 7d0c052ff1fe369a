/* qgx_latent_train.h — the latent step of a conditional VAE's training (CVAERegression: tools/train_CVAE.py wraps it), between
 * the encoder's last convolution and the decoder's first: the reparameterised sample z = eps std + mu, the decoder's input
 * record, the KL divergence to the standard normal prior with its two variance diagnostics, and the gradient of all that with
 * respect to the encoder's output.  Included by qgx.h (which declares the status codes); not meant to be included on its own.
 *
 * All pointers are device pointers, 16-byte aligned.  Every call runs on the caller's stream and synchronises nothing; no
 * call keeps state, there is no handle.  The layouts are those of qgx_head_train.h:
 *   engine layout   NHWC float32 (B, N, N, 8): one pixel is a record of 8 floats.  Outputs in this layout get their pad
 *                   channels WRITTEN as zero
 *   planar          (n, C, N, N) float32, PyTorch's layout of a data set held on the device
 *   idx_dev         int64 (B), or NULL: batch member b is row idx[b] of the planar set x (NULL: row b, and then n >= B).
 *                   0 <= idx[b] < n is the CALLER'S DUTY: the indices are on the device and no call reads them back
 * Admitted: N 16, 32, 48, 64, 96 or 128, B >= 1 with B N N <= 2^29, n >= 1.  Anything else, a null pointer (but those said to
 * be optional), a misaligned pointer or a workspace of fewer bytes than qgx_latent_workspace gives returns QGX_ERR_INVALID
 * with a message naming the field, before any device call.
 *
 * The records:
 *   enc      the encoder's output, channels [mu1, mu2, logvar1, logvar2, 0, 0, 0, 0]
 *   dec_in   the decoder's input,  channels [x1, x2, z1, z2, 0, 0, 0, 0]
 * eps is planar (B, 2, N, N), or it is drawn: eps[b, c, y, x] is element c N N + y N + x of the 2 N N standard normals of
 * Philox4x32-10 with counter (quad, step mod 2^32, b, step >> 32) and key (seed mod 2^32, seed >> 32), four normals per quad:
 * the layout of qgx_noise_normal with member_offset 0 and n_per_member = 2 N N.  The forward and the backward of one step are
 * given the same (seed, step) and draw the same eps: nothing but enc is kept between the two calls.
 *
 * Arithmetic: std = expf(0.5f logvar), var = std std, z = eps std + mu, and every term below, are float32.  Every sum is
 * float64 from its first add.  Results are bitwise repeatable and do not depend on the stream: the pixels are cut into ranges
 * that are a fixed function of (B, N); a workgroup adds the terms of its range in a fixed order into its own slot of the
 * workspace, and a second kernel adds the slots in a fixed order.  There are no float atomics. */
#ifndef QGX_LATENT_TRAIN_H
#define QGX_LATENT_TRAIN_H

/* bytes of the workspace of qgx_latent_forward: four float64 partial sums per range, a function of (B, N) alone */
int qgx_latent_workspace(int64_t B, int N, size_t *bytes);

/* dec_in (B, N, N, 8) = [x[idx[b]], z, 0, 0, 0, 0] of the planar set x (n, 2, N, N), and stats_dev (three float64):
 *   stats[0]  loss_KL    = sum over b, c, y, x of 0.5f (mu^2 + var - 1 - logvar) / B
 *   stats[1]  var_latent = mean of var
 *   stats[2]  var_aggr   = the unbiased variance of all 2 B N N values of mu, plus var_latent
 * enc_dev NULL is the prior: mu = 0, logvar = 0 (z is eps, bit for bit); stats_dev and the workspace are then not used and may
 * be NULL.  eps_dev NULL: eps is drawn from (seed, step).  The workspace's contents mean nothing between calls, and two calls
 * that share one may not run concurrently */
int qgx_latent_forward(const float *enc_dev, const float *x_dev, const int64_t *idx_dev, const float *eps_dev, uint64_t seed,
                       uint64_t step, float *dec_in_dev, double *stats_dev, int64_t B, int N, int64_t n, void *work_dev,
                       size_t work_bytes, void *stream);

/* d_enc (B, N, N, 8) = [d_mu1, d_mu2, d_logvar1, d_logvar2, 0, 0, 0, 0], the gradient with respect to enc of
 * <d_dec_in, dec_in> + g loss_KL: dz is channels 2, 3 of d_dec_in (B, N, N, 8), g = *gout_kl_dev (one float64, read on the
 * device), s = float32(g / B), formed in float64 and rounded once, and
 *   d_mu     = dz + s mu
 *   d_logvar = 0.5f dz eps std + 0.5f s (var - 1)
 * with eps read from eps_dev, or drawn again from (seed, step) if it is NULL */
int qgx_latent_backward(const float *enc_dev, const float *eps_dev, uint64_t seed, uint64_t step, const float *d_dec_in_dev,
                        const double *gout_kl_dev, float *d_enc_dev, int64_t B, int N, void *stream);

#endif
