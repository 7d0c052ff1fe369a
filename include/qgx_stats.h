/* qgx_stats.h — the derived flow fields behind dataset_statistics / dataset_smart_read of the qgx C ABI.  Included by qgx.h
 * (which declares qgx_model and the status codes); not meant to be included on its own. */
#ifndef QGX_STATS_H
#define QGX_STATS_H

/* The derived fields of velocity snapshots (reference: pyqg_generative/tools/comparison_tools.py:305-324
 * relative_vorticity, KE, Ens, Vabs and :314-315 KE_time), per (snapshot, layer) plane of u, v (S, 2, N, N), both float
 * (is_double = 0) or both double (1), every one of them computed in float64:
 *   omega_dev  (S, 2, N, N) double         ddx(v) - ddy(u), spectral on the plan's grid: what qgx_rfft2 -> qgx_spec_curl ->
 *                                          qgx_irfft2 give (the 2h harmonics of a self-conjugate row / column do not
 *                                          contribute to the derivative across them)
 *   ke_dev     (S, 2, N, N) input dtype    (u^2 + v^2) / 2
 *   ens_dev    (S, 2, N, N) double         omega^2 / 2
 *   vabs_dev   (S, 2, N, N) input dtype    sqrt(u^2 + v^2)
 *   ke_sum_dev (S, 2) double               sum over the plane of (u^2 + v^2) / 2, of the float64 values before rounding
 * Every output may be NULL: it is then neither computed nor written.  plan: a model handle of the fields' grid (plan_only
 * is enough, as for qgx_rfft2); it supplies N, L and the transform tables, and on the grids without an LDS-resident
 * transform (N > 96) its batched transforms and their work fields: such a call may not run concurrently with another call
 * on the same handle.  There the planes go through the plan in chunks of its member count, one plane (u and v) per
 * member; on the other grids the plan's member count does not matter.  A plane's results depend on that plane's u and v
 * alone — a NaN stays in its plane — and are bitwise the same on every call and every stream (fixed partitions, a
 * fixed-order workgroup reduction, no float atomics).
 * work_dev: qgx_flow_features_workspace(plan, S) bytes (0 on the LDS-resident grids: work_dev may then be NULL); its
 * contents before the call are not read.
 * QGX_ERR_INVALID before any device call for null plan / u / v / bytes, S < 1 (or 2 S past 2^31 - 1), is_double not 0 / 1,
 * all five outputs NULL, or a work space below what _workspace reports. */
int qgx_flow_features_workspace(const qgx_model *plan, int64_t S, size_t *bytes);
int qgx_flow_features(qgx_model *plan, const void *u_dev, const void *v_dev, int is_double, int64_t S,
                      double *omega_dev, void *ke_dev, double *ens_dev, void *vabs_dev, double *ke_sum_dev,
                      void *work_dev, size_t work_bytes, void *stream);

#endif
