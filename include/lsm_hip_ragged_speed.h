/*
 * liblsm_hip.so — speed perturbation for clips of different lengths (SPEC.md §1.18): lsm_hip_speed.h's launch on rows of one
 * stride whose clips have their own lengths, the first stage of the augmentation recipe on the ragged route (§1.14 - 1.16).
 * The definition is "the clip alone": what a clip gets is, byte for byte, what lsm_speed_f32 gives for that clip in a launch
 * of its own shape.  A speed factor changes a clip's length; the new length is an integer the kernel computes and writes
 * where the ragged launches read their counts, so that it never has to reach the host -- and the host can compute the same
 * integer from the plan (lsm_speed_ragged_length).
 *
 * Rows of n_in samples, clip b has n_b = clamp(clip_samples[b], 0, n_in) samples; r is its design row under lsm_hip_speed.h's
 * rules (design_row NULL: row 0; r >= n_designs: the last design; r < 0: unperturbed).
 *   0 <= r   n'_b = min(ceil(n_b * up / down), n_out), in 64-bit arithmetic.  out[b, m] = z_c[m + delay] for m < n'_b, z_c the
 *            causal sample of lsm_hip_speed.h with every sample outside [0, n_b) counted as +0.0: lsm_speed_f32 on
 *            audio[b, :n_b] alone with n_in = n_b and n_out = n'_b, and so scipy.signal.resample_poly's outputs.
 *   r < 0    n'_b = min(n_b, n_out);  out[b, m] is the input's bits for m < n'_b, an int16 sample s widened as
 *            (float)s * 2^-15.
 * Every element of out[b] from n'_b to n_out is WRITTEN as +0.0: the clip alone has no ring-out tail.  n_b = 0 gives an
 * all-zero row and n'_b = 0.  A slowed clip that outgrows the row is cut at n_out.  Samples of audio[b] at or behind n_b are
 * never read and may hold anything, NaN included.
 *   clip_samples_out[b] = n'_b
 *   clip_bins_out[b]    = min(ceil(n'_b / 160), time_bins): what lsm_hip_ragged.h's encoders, the ragged one-launch step,
 *                         lsm_mix_ragged_f32 (as 160 * bins) and lsm_reservoir_run_ragged's producers take unread; they count
 *                         1 and 2 bins as 0.
 *
 * The conventions are those of lsm_hip_speed.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernel clamps every row and every length it is given.
 */
#ifndef LSM_HIP_RAGGED_SPEED_H
#define LSM_HIP_RAGGED_SPEED_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n'_b of a clip of n_b samples (below 0: 0) on a design (up, down) in a row of n_out: min(ceil(n_b * up / down), n_out) in
 * 64-bit arithmetic -- the one inline function the kernel calls; up = down = 1 is the unperturbed clip.  LSM_ERR_ARG for up or
 * down < 1 or n_out < 0.  Host only. */
int lsm_speed_ragged_length(int n_b, int up, int down, int n_out);

/* lsm_speed_f32's parameter list with
 *   clip_samples      behind n_in: DEVICE int32 (n_clips), 4-byte aligned, required
 *   clip_samples_out  in front of the stream: DEVICE int32 (n_clips), 4-byte aligned, or NULL
 *   clip_bins_out     DEVICE int32 (n_clips), 4-byte aligned, or NULL;  time_bins: the bins of a row of what follows, read only
 *                     with clip_bins_out */
int lsm_speed_ragged_f32(const void *audio, int sample_format, int n_clips, int n_in, const int32_t *clip_samples,
                         const double *taps_dev, int n_taps_total, const int32_t *designs, int n_designs,
                         const int32_t *design_row, int n_out, float *out, int32_t *clip_samples_out, int32_t *clip_bins_out,
                         int time_bins, void *stream);

/* lsm_speed_ragged_f32 refuses, in this order and before anything is launched: what lsm_speed_f32 refuses, in its order and
 * with its codes and words; a NULL clip_samples, then a clip_samples that is not 4-byte aligned; a clip_samples_out, then a
 * clip_bins_out that is not 4-byte aligned; with a clip_bins_out, time_bins < 3, then n_out < 160 * time_bins.  LSM_ERR_ARG
 * for each of its own. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_RAGGED_SPEED_H */
