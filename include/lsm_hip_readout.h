/*
 * liblsm_hip.so — readout scores (SPEC.md §6): a standard scaler and a linear readout applied to feature rows on the device,
 * class scores (float64) and labels (int32) out.  Two launches: one over feature rows that already exist (clip rows of
 * lsm_reservoir_run, the fused step, the ragged routes), and one over the segment records of streams, which folds the
 * records of every sliding window, forms its features in registers, scales them and accumulates the class scores without
 * ever writing the feature row.  Every value is specified to the bit: a NumPy restatement (tests/readout_restatement.py)
 * reproduces each output byte.
 *
 * The model, all float64 in DEVICE memory, 8-byte aligned: mean (D), scale (D), coef (n_classes, D) row-major, intercept
 * (n_classes); D = n_keys * n_out in the key-major row order d = k * n_out + o of the feature rows; 1 <= n_classes <= 64.
 *   z_d      = ((double)x_d - mean_d) / scale_d                       a true division
 *   p_l      = sum, in this order, over o = l, l + 64, ... < n_out and within o over k = 0 .. n_keys - 1 of
 *              z_d * coef[c][d], one float64 accumulator per lane l = 0 .. 63 that starts at +0.0, product and sum rounded
 *   tree     for s = 32, 16, 8, 4, 2, 1: p_l = p_l + p_{l+s}, l < s
 *   logit_c  = intercept_c + p_0
 *   label    = -1 when a logit of the row is NaN, else the smallest c whose logit no other logit exceeds
 * The device checks no model value: a scale of 0 or a non-finite entry gives the IEEE results of the lines above.
 *
 * The conventions are those of lsm_hip.h: 0 or a negative LSM_ERR_* code with a thread-local message (lsm_last_error());
 * caller-owned DEVICE buffers, HOST key_ids; asynchronous on `stream`; no allocation, no synchronisation, capturable into a
 * HIP graph, and no device value is ever read on the host -- the kernel clamps the counts it is given.
 */
#ifndef LSM_HIP_READOUT_H
#define LSM_HIP_READOUT_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the two launches below serve a model of these sizes, else 0: n_keys in [1, 8], n_out in [1, 8192], n_classes in
 * [1, 64].  There is no further limit (no LDS image, no workspace).  Host only. */
int lsm_readout_supported(int n_keys, int n_out, int n_classes);

/* Scores of rows that already exist.
 *   features     (n_rows, n_keys * n_out) float32, 4-byte aligned
 *   logits_out   (n_rows, n_classes) float64, 8-byte aligned, or NULL
 *   labels_out   (n_rows) int32, 4-byte aligned, or NULL; not both NULL
 * Refusals, in this order and before anything is launched (LSM_ERR_ARG): n_rows < 0; sizes that lsm_readout_supported
 * refuses (n_keys, then n_out, then n_classes); a NULL mean, scale, coef or intercept; logits_out and labels_out both NULL; a
 * pointer that is not aligned to its element.  n_rows == 0 then returns 0 and launches nothing; a NULL features is refused
 * after that. */
int lsm_readout_rows_f32(const double *mean, const double *scale, const double *coef, const double *intercept,
                         const float *features, int n_rows, int n_keys, int n_out, int n_classes, double *logits_out,
                         int32_t *labels_out, void *stream);

/* Scores of the sliding windows of segment records: lsm_segment_features_ragged (lsm_hip_streams.h) and lsm_readout_rows_f32
 * in one launch that writes no feature row.  records, n_segments, clip_segments, segment_steps, window_segments, hop_segments,
 * key_ids and n_keys are lsm_segment_features_ragged's, with the same clamping and window rule; n_out is the handle's.
 *   clip_segments  (n_clips) int32, DEVICE memory, 4-byte aligned, or NULL: every clip has all n_segments records
 *   logits_out     (n_clips, W, n_classes) float64, 8-byte aligned, or NULL;  W = (n_segments - window_segments) / hop_segments + 1
 *   labels_out     (n_clips, W) int32, 4-byte aligned, or NULL; not both NULL
 * Row w < W_b of clip b receives, byte for byte, what lsm_readout_rows_f32 gives on lsm_segment_features_ragged's row; rows at
 * w >= W_b are left as they are.
 * Refusals, in this order and before anything is launched (LSM_ERR_ARG): a NULL handle; n_clips < 0 or n_segments < 1;
 * segment_steps < 1; window_segments outside [1, n_segments]; hop_segments < 1; window_segments * segment_steps > 65535; n_keys
 * outside [1, 8] or a NULL key_ids; a key id outside [0, 8); n_classes outside [1, 64]; a NULL mean, scale, coef or intercept;
 * logits_out and labels_out both NULL; a records pointer that is not 16-byte aligned or another pointer that is not aligned
 * to its element.  n_clips == 0 then returns 0 and launches nothing; a NULL records and a handle of another device than the
 * current one are refused after that. */
int lsm_readout_windows(const lsm_reservoir *h, const double *mean, const double *scale, const double *coef,
                        const double *intercept, const void *records, int n_clips, int n_segments,
                        const int32_t *clip_segments, int segment_steps, int window_segments, int hop_segments,
                        const int32_t *key_ids, int n_keys, int n_classes, double *logits_out, int32_t *labels_out,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_READOUT_H */
