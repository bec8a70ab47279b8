/*
 * liblsm_hip.so — silence trimming in front of the ragged front end (SPEC.md §1.15): an endpoint detector that finds, per
 * clip and on the device, where the speech is, moves it to the start of its row and hands the ragged launches
 * (lsm_hip_ragged.h, lsm_reservoir_run_ragged, lsm_step_fused_ragged_f64) its number of bins, so that they filter and
 * integrate speech and not the silence around it.  The count never has to reach the host.  Every value is specified to the
 * bit: a NumPy restatement (tests/trim_restatement.py) reproduces each output byte.
 *
 * The hop is 160 samples.  Clip b has len_b = min(max(clip_samples[b], 0), n_samples) valid samples (clip_samples NULL:
 * n_samples) and NB_b = min(ceil(len_b / 160), time_bins) bins; a sample at an index >= len_b counts as +0.0 and is never
 * read, so it may hold anything, NaN included.
 *
 *   energy   e_j = sum over i = 0 .. 159, ascending, of (double)x[160 j + i]^2: one float64 accumulator that starts at +0.0
 *            (the product of two float32 values is exact in float64: only the order is pinned).
 *   active   bin j is active iff e_j > E * ratio, E = max e_j over j < NB_b: one float64 multiply, a strict compare.
 *   whole    first = 0, bins = NB_b when NB_b < 3, when no bin is active (an all-zero clip), or when an e_j, j < NB_b, is not
 *            finite (the front end's own NaN/Inf rule then applies unchanged).
 *   trimmed  otherwise lo = max(first_active - pad_bins, 0), hi = min(last_active + pad_bins, NB_b - 1); if
 *            hi - lo + 1 < m = min(min_bins, NB_b): need = m - (hi - lo + 1), g = min(need, NB_b - 1 - hi), hi += g,
 *            lo -= need - g.  first = lo, bins = hi - lo + 1.
 *
 * audio_out row b holds samples [160 * first, 160 * (first + bins)) of the clip at its start, indices >= len_b as +0.0, and
 * every remaining element of the row is WRITTEN as +0.0: a trimmed clip is, byte for byte, a slice of the input.
 *
 * The conventions are those of lsm_hip_ragged.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, capturable
 * into a HIP graph.  clip_samples is read by the kernel only and CLAMPED, so that no value of an int32 can make it address
 * outside the launch's buffers.
 */
#ifndef LSM_HIP_TRIM_H
#define LSM_HIP_TRIM_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Dynamic LDS bytes of a launch: 8 * time_bins for the energies and a tile of 64 bins at a pitch of 161 words.  Negative
 * (LSM_ERR_ARG) for time_bins outside 3 .. 4096.  Host only. */
int lsm_trim_lds_bytes(int time_bins);

/*   audio           (n_clips, n_samples) float32, 4-byte aligned
 *   clip_samples    (n_clips) int32, 4-byte aligned, or NULL: n_samples for every clip
 *   ratio           the activity threshold as a share of the clip's loudest bin, 0 <= ratio < 1: 10^(-top_db / 10), or 0
 *                   for "digital silence only"
 *   pad_bins        bins kept on either side of the active span;  min_bins 3 .. time_bins: the fewest bins a trimmed clip has
 *   audio_out       (n_clips, n_samples_out) float32, 4-byte aligned, never audio; n_samples_out >= 160 * time_bins
 *   clip_first_out  (n_clips) int32 or NULL: first;  clip_bins_out  (n_clips) int32 or NULL: bins
 *   energy_out      (n_clips, time_bins) float64, 8-byte aligned, or NULL: e_j for j < NB_b, +0.0 behind */
int lsm_trim_silence_f32(const float *audio, int n_clips, int n_samples, int time_bins, const int32_t *clip_samples,
                         double ratio, int pad_bins, int min_bins, float *audio_out, int n_samples_out,
                         int32_t *clip_first_out, int32_t *clip_bins_out, double *energy_out, void *stream);

/* lsm_trim_silence_f32 refuses, in this order and before anything is launched: n_clips < 0 or n_samples < 1; time_bins < 3
 * (LSM_ERR_ARG) or > 4096 (LSM_ERR_UNSUPPORTED: the energies and the endpoint reductions of a clip live in one workgroup's
 * LDS); a ratio that is not finite or lies outside [0, 1); pad_bins < 0; min_bins outside [3, time_bins]; a NULL audio or
 * audio_out; audio_out == audio; n_samples_out < 160 * time_bins; a pointer that is not aligned to its element.  LSM_ERR_ARG
 * unless said otherwise.  n_clips == 0 then returns 0 and launches nothing. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_TRIM_H */
