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
 *       period of 2; time_bins * n_thr steps that fit the reservoir's plan.  The entry points have no spike matrix, membrane
 *       trace, state or segments: a step that needs a spike matrix or a trace takes the two launches, one that carries
 *       state or closes time segments has entry points of its own (lsm_hip_step_state.h).
 *   lsm_step_fused_form_supported   the same question for one form of the step: `form` 0 the plain step (the answer of
 *       lsm_step_fused_supported), 1 the masked step (served wherever the plain one is), 2 the ragged step, which
 *       additionally needs hop == 160 (the one hop the ragged front end is offered for, lsm_hip_ragged.h).  The LDS bound is
 *       the same for all three: no form adds a byte to the image.  Another `form` is a bad argument.  The ragged launch also
 *       needs ncols == time_bins - 2, which the query is not given: on hop 160 that is every front end whose rows hold
 *       n_samples = 160 * time_bins samples under a 400-sample window, and the launch answers another ncols with
 *       LSM_ERR_UNSUPPORTED.
 *   lsm_step_fused_f64   the step.  The front-end parameters are lsm_gammatone_spikes_f64's without the raster and the launch
 *       flags (the workspace is lsm_gammatone_spikes_workspace bytes, as there), the reservoir's are lsm_reservoir_run's
 *       without the raster, the spike matrix, the trace and waves_per_clip.  LSM_ERR_UNSUPPORTED for a shape that
 *       lsm_step_fused_supported answers with 0; otherwise the refusals of the two entry points, the front end's first.
 *   lsm_step_fused_masked_f64   the step under SpecAugment masks (SPEC.md 1.13): lsm_step_fused_f64's parameters with
 *       `freq_mask` and `time_mask` in front of `stream`, DEVICE words laid out as lsm_hip_mask.h says -- clip b's filter f at
 *       bit f % 32 of freq_mask[b * ceil(n_filters / 32) + f / 32], its time bin j likewise in rows of ceil(time_bins / 32)
 *       words; bits at or beyond n_filters / time_bins are ignored; either pointer may be NULL (no mask of that kind).  The
 *       masked value is +0.0 before the latches.  Rows and stats_out are, bit for bit, those of
 *       lsm_gammatone_spikes_masked_f64 followed by lsm_reservoir_run.  With both pointers NULL the launch is
 *       lsm_step_fused_f64's, and with all bits clear the bytes are.  Own refusal, behind the two halves': a pointer that is
 *       not 4-byte aligned.  Served shapes: form 1.
 *   lsm_step_fused_ragged_f64   the step on clips of different lengths (SPEC.md 1.14, 4c): lsm_step_fused_f64's parameters
 *       with `clip_bins` behind `time_bins`, a DEVICE array of n_clips counts that no host code reads and the kernel clamps
 *       as lsm_hip_ragged.h says: below 3 (1 and 2 included) counts as 0, above time_bins as time_bins.  Clip b filters and
 *       encodes its own clip_bins[b] bins, as lsm_gammatone_spikes_ragged_f64 does, and the reservoir half runs
 *       clip_bins[b] * n_thr steps with the features of that many steps (key 1 divides by them, not by the stride): bit for bit
 *       the rows and stats_out of that launch followed by lsm_reservoir_run_ragged on its clip_steps_out, and those of the
 *       clip alone in a front end and a run of its own length.  The count never leaves the workgroup: no clip_steps_out, no
 *       state block.  A clip of 0 bins leaves its feature row and its stats_out row untouched.  Own refusals, behind the two
 *       halves', in this order: clip_bins NULL, not 4-byte aligned, time_bins < 3, n_samples < hop * time_bins.  Served
 *       shapes: form 2 with ncols == time_bins - 2.  A batch is ragged or masked: there is no masked ragged step.
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

int lsm_step_fused_form_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                                  int n_thr, int redundancy, int coef_flags, int form);

int lsm_step_fused_masked_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                              int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on,
                              const double *thr_off, int n_thr, int redundancy, void *workspace, long workspace_bytes,
                              int coef_flags, const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out,
                              const uint32_t *freq_mask, const uint32_t *time_mask, void *stream);

int lsm_step_fused_ragged_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                              int n_filters, int nwin, int hop, int ncols, int time_bins, const int32_t *clip_bins,
                              const double *thr_on, const double *thr_off, int n_thr, int redundancy, void *workspace,
                              long workspace_bytes, int coef_flags, const int32_t *key_ids, int n_keys, float *features_out,
                              int32_t *stats_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_STEP_H */
