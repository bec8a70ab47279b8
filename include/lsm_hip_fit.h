/*
 * liblsm_hip.so — streaming ridge fit (SPEC.md §7): the statistics a standard scaler and a ridge readout are functions of,
 * updated on the device from the feature rows of one step.  One launch adds a block of rows to the lower triangle of X^T X,
 * to the per-class sums of x, to the class counts and to the column ranges; the rows themselves need not be kept.  Every
 * value is specified to the bit: a NumPy restatement (tests/fit_restatement.py) reproduces each output byte.
 *
 * The statistics, caller-owned DEVICE buffers that the caller initialises (zeros for the first three, +inf for col_min,
 * -inf for col_max); D = n_keys * n_out in the key-major row order d = k * n_out + o of the feature rows:
 *   gram          (D, D) float64 row-major, 8-byte aligned; only entries with j <= i are read or written
 *   class_sums    (n_classes, D) float64, 8-byte aligned
 *   class_counts  (n_classes) int64, 8-byte aligned
 *   col_min, col_max  (D) float32, 4-byte aligned
 * For r = 0 .. n_rows - 1 in ascending order, with x = features[r] and y = labels[r]; a row whose y lies outside
 * [0, n_classes) is skipped entirely:
 *   gram[i][j]       = gram[i][j] + (double)x_i * (double)x_j          for every j <= i  (the product of two float32 values is
 *                      exact in float64: a fused multiply-add and a multiply followed by an add round alike)
 *   class_sums[y][d] = class_sums[y][d] + (double)x_d
 *   class_counts[y]  = class_counts[y] + 1
 *   col_min[d]       = x_d < col_min[d] ? x_d : col_min[d]
 *   col_max[d]       = x_d > col_max[d] ? x_d : col_max[d]             a NaN is never taken
 * Every accumulator continues from the stored value in row order, so a run of launches over rows cut anywhere leaves the
 * bytes of one launch over all of them.  The device checks no feature: a non-finite one gives the IEEE results of the lines
 * above.
 *
 * The conventions are those of lsm_hip.h: 0 or a negative LSM_ERR_* code with a thread-local message (lsm_last_error());
 * asynchronous on `stream`; no allocation, no synchronisation, capturable into a HIP graph, and no device value is ever read
 * on the host.  Launches on the same statistics must be ordered by the caller (one stream, or events).
 */
#ifndef LSM_HIP_FIT_H
#define LSM_HIP_FIT_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shape of the launch as built: a workgroup owns a LSM_FIT_TILE x LSM_FIT_TILE tile of the triangle and stages
 * LSM_FIT_STAGE_ROWS feature rows at a time.  No result depends on either; the tests place their edge cases by them. */
#define LSM_FIT_TILE 64
#define LSM_FIT_STAGE_ROWS 16

/* 1 when the launch below serves these sizes, else 0: n_keys in [1, 8], n_out >= 1, D = n_keys * n_out <= 16384, n_classes
 * in [1, 64].  Host only. */
int lsm_fit_supported(int n_keys, int n_out, int n_classes);

/* Add n_rows rows to the statistics.
 *   features  (n_rows, n_keys * n_out) float32, 4-byte aligned
 *   labels    (n_rows) int32, DEVICE memory, 4-byte aligned
 * Refusals, in this order and before anything is launched (LSM_ERR_ARG): n_rows < 0; sizes that lsm_fit_supported refuses
 * (n_keys, then n_out, then D, then n_classes); a NULL gram, class_sums, class_counts, col_min or col_max; a gram, class_sums
 * or class_counts that is not 8-byte aligned; a features, labels, col_min or col_max that is not 4-byte aligned.  n_rows == 0
 * then returns 0 and launches nothing; a NULL features or labels is refused after that. */
int lsm_fit_accumulate_f32(const float *features, const int32_t *labels, int n_rows, int n_keys, int n_out, int n_classes,
                           double *gram, double *class_sums, int64_t *class_counts, float *col_min, float *col_max,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_FIT_H */
