/*
 * liblsm_hip.so — one launch per step: the lane-pair gammatone front end and the dense-row reservoir of a clip in one
 * workgroup.  A step of the hot path is lsm_gammatone_spikes_f64 followed by lsm_reservoir_run; where HIP
 * has few hardware queues (GPU_MAX_HW_QUEUES <= 4) the two launches of several steps in flight wait for each other at the
 * heads of shared queues.  lsm_step_fused_f64 is the same step as ONE launch: a workgroup of 4 waves filters and encodes its
 * clip exactly as the lane-pair form of lsm_gammatone_spikes_f64 does, keeps the raster bits in LDS, turns them into the
 * reservoir's input bit rows there, and runs the time loop of lsm_reservoir_run's dense-row kernel on them.  No uint8 raster
 * is written or read, and no event ties two launches.  The feature rows and stats_out are, bit for bit, those of the two
 * launches.
 *
 *   lsm_step_fused_supported   1 when lsm_step_fused_f64 serves this shape, 0 when it does not (the caller then makes the two
 *       launches), negative on a bad argument.  Served: a gammatone front end whose lane-pair layout has 4 waves per clip
 *       (97..128 filters, redundancy 1, so at most 128 input channels), on the fast coefficient path (coef_flags bits 0 and
 *       1) with 3 live windows (2 * hop < nwin <= 3 * hop); a reservoir whose launch inside a pipeline (waves_per_clip = -1) is
 *       the dense-row kernel with 4 waves per clip, 1, 2 or 4 neuron slots per lane, coloured input masks and a refractory
 *       period of 2; time_bins * n_thr steps that fit the reservoir's plan.  The entry point has no spike matrix, membrane
 *       trace, state, segments, masks or ragged counts: a step that needs one of them takes the two launches.
 *   lsm_step_fused_f64   the step.  The front-end parameters are lsm_gammatone_spikes_f64's without the raster and the launch
 *       flags (the workspace is lsm_gammatone_spikes_workspace bytes, as there), the reservoir's are lsm_reservoir_run's
 *       without the raster, the spike matrix, the trace and waves_per_clip.  LSM_ERR_UNSUPPORTED for a shape that
 *       lsm_step_fused_supported answers with 0; otherwise the refusals of the two entry points, the front end's first.
 *
 * A caller that brackets its reservoir launches with an event pair (HotPath(time_reservoir=True), bench.py --full) brackets
 * the whole fused launch: under it the pair measures front end and reservoir of the step together.
 *
 * Conventions as in lsm_hip.h: 0 or a negative LSM_ERR_* code with a thread-local message (lsm_last_error()); caller-owned
 * DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, capturable into a HIP graph.
 */
#ifndef LSM_HIP_STEP_H
#define LSM_HIP_STEP_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lsm_step_fused_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins, int n_thr,
                             int redundancy, int coef_flags);

int lsm_step_fused_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                       int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on, const double *thr_off,
                       int n_thr, int redundancy, void *workspace, long workspace_bytes, int coef_flags,
                       const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_STEP_H */
