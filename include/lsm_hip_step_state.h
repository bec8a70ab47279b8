/*
 * liblsm_hip.so — the one-launch step (lsm_hip_step.h) with carried state and time segments (SPEC.md §4f).
 * lsm_step_fused_f64 starts every clip from reset and keeps one feature record per output neuron.  The entry points here run
 * the same workgroup -- the lane-pair gammatone front end of a clip, its raster bits handed over in LDS, the dense-row time
 * loop -- with the reservoir half in the form lsm_reservoir_run_from and lsm_reservoir_run_segments launch: the clip's
 * SPEC.md §4a state block is loaded behind the front end and stored after the last step, and the §4b segment records are
 * closed on the way.  A long recording cut into windows, or a step whose features are wanted per time segment, is then ONE
 * launch per window / step: no uint8 raster is written or read, no event ties launches of two streams, and no second launch
 * folds the records into rows.
 *
 *   lsm_step_fused_state_supported   1 when the two entry points below serve this shape, 0 when they do not (the caller makes
 *       the separate launches), negative on a bad argument.  The served set is lsm_step_fused_supported's and so is the LDS
 *       bound: the state forms add no byte to the image.
 *   lsm_step_fused_from_f64   lsm_step_fused_f64's parameters with `first_step`, `state_in` and `state_out` in front of
 *       `key_ids`, as lsm_reservoir_run_from has them: the steps done before this launch, the DEVICE state blocks
 *       (n_clips x lsm_reservoir_state_bytes) read and written; either may be NULL (reset / not saved) and they may be the
 *       same buffer.  Bit for bit lsm_gammatone_spikes_f64 followed by lsm_reservoir_run_from: features_out holds the
 *       features of [0, first_step + time_bins * n_thr), stats_out the totals of the whole run, state_out the block byte for
 *       byte.  n_keys may be 0 (features_out is then not written and may be NULL).  With both states NULL (first_step 0) the
 *       launch is lsm_step_fused_f64's, and so are the bytes.
 *   lsm_step_fused_segments_f64   the same parameters with `segment_steps`, `records_out` and `segment_rows_out` in front of
 *       `stream`.  Bit for bit the front end followed by lsm_reservoir_run_segments: records_out receives
 *       (n_clips, T / segment_steps, n_out) records of 16 bytes on segment-local times (T = time_bins * n_thr), features_out
 *       the cumulative features (NULL with n_keys = 0), the state as above.  segment_rows_out, when not NULL, receives the
 *       G = T / segment_steps tumbling feature rows of every clip, (n_clips, G, n_keys * n_out) float32 key-major: row g is
 *       the feature row of segment g alone over segment_steps steps, which is what lsm_segment_features gives on records_out
 *       with window_segments = hop_segments = 1.  The workgroup writes them from its own records after its last step.
 *
 * Refusals, in this order: the front end's (lsm_gammatone_spikes_f64's); the reservoir's, in lsm_reservoir_run_segments'
 * order and words -- segment_steps < 1, time_bins * n_thr not a multiple of segment_steps, records_out NULL or not 16-byte
 * aligned, first_step < 0, first_step + T > 65535, first_step > 0 without state_in, a state pointer that is not 16-byte
 * aligned, n_keys outside [0, 8], a key id outside [0, 8), NULL features_out with n_keys > 0 --; the form's own --
 * segment_rows_out not 4-byte aligned, segment_rows_out with n_keys = 0 --; then LSM_ERR_UNSUPPORTED ("shape not served ...
 * make the separate launches") for a shape lsm_step_fused_state_supported answers with 0.  A refused call launches nothing.
 *
 * There is no masked and no ragged state step: such a step keeps its separate launches.
 *
 * Conventions as in lsm_hip.h: 0 or a negative LSM_ERR_* code with a thread-local message (lsm_last_error()); caller-owned
 * DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, capturable into a HIP graph.
 */
#ifndef LSM_HIP_STEP_STATE_H
#define LSM_HIP_STEP_STATE_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lsm_step_fused_state_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                                   int n_thr, int redundancy, int coef_flags);

int lsm_step_fused_from_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                            int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on,
                            const double *thr_off, int n_thr, int redundancy, void *workspace, long workspace_bytes,
                            int coef_flags, int first_step, const void *state_in, void *state_out, const int32_t *key_ids,
                            int n_keys, float *features_out, int32_t *stats_out, void *stream);

int lsm_step_fused_segments_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                const double *coefs_dev, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                const double *thr_on, const double *thr_off, int n_thr, int redundancy, void *workspace,
                                long workspace_bytes, int coef_flags, int first_step, const void *state_in, void *state_out,
                                const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out, int segment_steps,
                                void *records_out, float *segment_rows_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_STEP_STATE_H */
