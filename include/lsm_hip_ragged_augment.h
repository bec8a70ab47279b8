/*
 * liblsm_hip.so — augmentation for clips of different lengths (SPEC.md §1.16): the noise mixer (§1.10, lsm_hip_mix.h) and the
 * masks inside the spike encoders (§1.13, lsm_hip_mask.h) on the ragged launches of §1.14 (lsm_hip_ragged.h) and on the ragged
 * one-launch step (lsm_hip_step.h).  A batch may be ragged AND masked, and its rows may be mixed at each clip's own length.
 * Every definition is "the clip alone": what a clip gets is, byte for byte, what the unragged entry point gives for that clip
 * in a launch of its own shape.
 *
 * Ragged noise mixer.  Rows of n_samples, clip b has n_b = clamp(clip_samples[b], 0, n_samples) samples, and the batch form of
 * lsm_hip_mix.h holds with n := n_b everywhere:
 *     s = clamp(shift[b], -n_b, n_b);  x[i] = a * audio[b, i - s] where 0 <= i - s < n_b, else +0.0, for 0 <= i < n_b
 *     v[i] = noise[r, (o + i) mod L] for i < n_b;  Px = P(x) and Pv = P(v) over k + l < n_b, in the 256-lane structure
 *     g and y[i] for i < n_b as there;  out[b, i] = +0.0 for n_b <= i < n_samples, WRITTEN
 *     n_b = 0:  Px = Pv = +0.0, g = 0, the row all zeros
 * For n_b >= 1 the first n_b samples of out[b], gain_out[b] and power_out[b] equal lsm_mix_f32 on audio[b, :n_b] alone at
 * n_samples = n_b.  Samples of audio[b] at or behind n_b influence nothing and may hold anything, NaN included (reverberation
 * with n_out = n_in on the padded row leaves its tail there: lsm_reverb_f32 is causal, so its first n_b output samples are the
 * clip-alone samples, bit for bit).
 *
 * Masks on ragged launches.  Frequency bit f is §1.13's.  Time bit j names bin j of clip b's own T_b bins; the mask rows keep
 * the launch's stride, ceil(time_bins / 32) words per clip (ceil(n_filters / 32) for freq_mask), and bits at or behind T_b are
 * ignored.  Maximum, floor, minimum, the flat test and the zoom are those of the unmasked clip at its own length (§1.14); a
 * masked cell is +0.0 before the latches.  Clip b's raster (and norm_out) is what the masked unragged entry point gives for the
 * clip alone, on a front end built for its T_b bins, with the first n_filters and T_b bits of the clip's mask rows.  With both
 * mask pointers NULL exactly the ragged twin's launch is made; with all bits clear the bytes are the same.  A clip of 0 bins
 * keeps §1.14's behaviour.
 *
 *   lsm_gammatone_spikes_ragged_masked_f64, lsm_spec_to_spikes_ragged_masked_f64 / _f32
 *       the ragged twin's parameter list with freq_mask, time_mask in front of the stream.  The gammatone entry serves every
 *       layout its twin does (lane pair, one chain, two chains).
 *   lsm_step_fused_ragged_masked_f64
 *       lsm_step_fused_ragged_f64 with the two mask pointers: feature rows and stats_out equal, bit for bit,
 *       lsm_gammatone_spikes_ragged_masked_f64 followed by lsm_reservoir_run_ragged.
 *   lsm_step_fused_ragged_masked_supported
 *       lsm_step_fused_supported's parameters: 1 where the step above is served -- wherever form 2 (ragged) of
 *       lsm_step_fused_form_supported is -- else 0, or a negative code for a bad argument.
 *
 * The conventions are those of lsm_hip_mix.h and lsm_hip_ragged.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernels clamp every count.  Refusals, all before anything is launched:
 * lsm_mix_ragged_f32 makes lsm_mix_f32's in its order, then LSM_ERR_ARG for a NULL clip_samples, then for a clip_samples that
 * is not 4-byte aligned; the masked ragged entry points make their ragged twin's, then LSM_ERR_ARG for a mask pointer that is
 * not 4-byte aligned.
 */
#ifndef LSM_HIP_RAGGED_AUGMENT_H
#define LSM_HIP_RAGGED_AUGMENT_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lsm_mix_f32's list with clip_samples behind n_samples: DEVICE int32 (n_clips), 4-byte aligned, required. */
int lsm_mix_ragged_f32(const float *audio, int n_clips, int n_samples, const int32_t *clip_samples, const float *noise,
                       int n_noise_rows, int noise_len, const int32_t *noise_row, const int32_t *noise_offset,
                       const int32_t *shift, const float *scale, const double *ratio, float *out, double *gain_out,
                       double *power_out, void *stream);

/* freq_mask (n_clips, ceil(n_filters / 32)), time_mask (n_clips, ceil(time_bins / 32)): DEVICE uint32, 4-byte aligned, or NULL */
int lsm_gammatone_spikes_ragged_masked_f64(const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                                           int n_filters, int nwin, int hop, int ncols, int time_bins,
                                           const int32_t *clip_bins, const double *thr_on, const double *thr_off, int n_thr,
                                           int redundancy, uint8_t *raster, int32_t *clip_steps_out, void *workspace,
                                           long workspace_bytes, int coef_flags, int launch_flags, const uint32_t *freq_mask,
                                           const uint32_t *time_mask, void *stream);

int lsm_spec_to_spikes_ragged_masked_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins,
                                         const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                         const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                                         uint8_t *raster, double *norm_out, const uint32_t *freq_mask,
                                         const uint32_t *time_mask, void *stream);

int lsm_spec_to_spikes_ragged_masked_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins,
                                         const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                         const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                                         uint8_t *raster, float *norm_out, const uint32_t *freq_mask,
                                         const uint32_t *time_mask, void *stream);

int lsm_step_fused_ragged_masked_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop,
                                           int time_bins, int n_thr, int redundancy, int coef_flags);

int lsm_step_fused_ragged_masked_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                     const double *coefs_dev, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                     const int32_t *clip_bins, const double *thr_on, const double *thr_off, int n_thr,
                                     int redundancy, void *workspace, long workspace_bytes, int coef_flags,
                                     const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out,
                                     const uint32_t *freq_mask, const uint32_t *time_mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_RAGGED_AUGMENT_H */
