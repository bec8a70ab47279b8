/*
 * liblsm_hip.so — clips of different lengths in one front-end launch (ragged audio, SPEC.md §1.14).  The counterpart of
 * lsm_reservoir_run_ragged (lsm_hip.h) in front of it: a batch whose clips each have their own number of time bins goes
 * through the front end in the launches a batch of equal clips takes, and every clip's raster is, byte for byte, the raster
 * of a launch over that clip alone.
 *
 * A launch has STRIDES and every clip has COUNTS.  The strides are the twin's shape parameters (n_samples, ncols, n_frames,
 * time_bins): they say where clip b's rows lie in the batch's buffers and size the scratch and the LDS.  The counts say how
 * much of those rows is the clip: DEVICE int32 arrays of n_clips entries, 4-byte aligned, read by the kernels only -- the
 * library never reads device memory to check one, and never synchronises.  The kernels therefore CLAMP what they find:
 *
 *     bins   T_b   min(max(v, 0), time_bins); 1 and 2 count as 0.  A clip is 0 bins (empty) or 3 .. time_bins bins.
 *     cols         min(max(v, 0), ncols); a clip without a column is empty.
 *     frames       min(max(v, 0), n_frames).
 *
 * so that no value of an int32 can make a kernel address outside the launch's buffers.
 *
 * Clip b's raster rows keep the launch's length time_bins * n_thr.  The clip owns bytes [0, T_b * n_thr) of each of its rows:
 * they are the rows of the twin called on this clip alone with (cols_b, T_b) for (ncols, time_bins) -- minimum, maximum and
 * the 80 dB floor over the clip's own values, the resize ratio, the "last bin outside the input is +0.0" rule (SPEC.md 1.2),
 * the no-zoom case cols_b == T_b and the flat test all per clip.  The remaining bytes of the row are WRITTEN as 0, and an
 * empty clip has all-zero rows.  Input beyond a clip's counts (samples from hop * T_b on, columns from cols_b on, frames from
 * frames_b on) influences nothing and may hold anything, NaN included.
 *
 *   lsm_spec_to_spikes_ragged_f64 / _f32
 *       lsm_spec_to_spikes_* with clip_cols, clip_bins after time_bins.  db is (n_clips, n_filters, ncols), raster
 *       (n_clips, n_filters * redundancy, time_bins * n_thr), norm_out (n_clips, n_filters, time_bins): ncols and time_bins
 *       are strides.  norm_out is written as 0 past T_b.
 *   lsm_power_to_db_ragged_f32
 *       lsm_power_to_db_f32 on rows: power and db_out are (n_clips, n_mels, n_frames); the reference maximum, the NaN rule
 *       and the top_db floor cover frames < clip_frames[b] only; columns from there on are written as 0.
 *   lsm_gammatone_spikes_ragged_f64
 *       lsm_gammatone_spikes_f64 -- one launch, filterbank to raster -- with clip_bins after time_bins and clip_steps_out after
 *       raster.  audio is (n_clips, n_samples) with n_samples >= hop * time_bins; clip b is the first hop * T_b samples of its
 *       row and has cols_b = T_b - (time_bins - ncols) columns (a clip that would have none is empty), so with nwin = 400,
 *       hop = 160 and ncols = time_bins - 2 a clip of T_b bins has the T_b - 2 columns of gtgram on 160 * T_b samples.  The
 *       last sample filtered is (cols_b - 1) * hop + nwin - 1.  clip_steps_out: DEVICE int32 (n_clips), 4-byte aligned, or
 *       NULL; receives T_b * n_thr, the `lengths` of lsm_reservoir_run_ragged, on the same stream and without a host round
 *       trip.  The workspace is lsm_gammatone_spikes_workspace(n_clips, n_filters, ncols) bytes with the stride ncols; the
 *       layout (lsm_gammatone_spikes_layout answers for both), launch_flags and coef_flags are the twin's.
 *
 * Masks (SPEC.md §1.13, lsm_hip_mask.h) are NOT offered on the ragged entry points: a batch is ragged or masked.
 *
 * The conventions are those of lsm_hip_mask.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation.  The twin's
 * refusals (LSM_ERR_ARG, LSM_ERR_UNSUPPORTED) apply unchanged, to the strides, and in the twin's order; after them, and
 * before anything is launched, LSM_ERR_ARG for, in this order: a NULL count array; a count array that is not 4-byte aligned;
 * time_bins < 3; n_samples < hop * time_bins (the gammatone entry).
 */
#ifndef LSM_HIP_RAGGED_H
#define LSM_HIP_RAGGED_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lsm_spec_to_spikes_ragged_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins,
                                  const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor, const double *thr_on,
                                  const double *thr_off, int n_thr, int redundancy, uint8_t *raster, double *norm_out,
                                  void *stream);

int lsm_spec_to_spikes_ragged_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins,
                                  const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor, const float *thr_on,
                                  const float *thr_off, int n_thr, int redundancy, uint8_t *raster, float *norm_out,
                                  void *stream);

int lsm_power_to_db_ragged_f32(const float *power, int n_clips, int n_mels, int n_frames, const int32_t *clip_frames,
                               float amin, float top_db, float *db_out, void *stream);

int lsm_gammatone_spikes_ragged_f64(const float *audio, int n_clips, int n_samples, const double *coefs_dev, int n_filters,
                                    int nwin, int hop, int ncols, int time_bins, const int32_t *clip_bins,
                                    const double *thr_on, const double *thr_off, int n_thr, int redundancy, uint8_t *raster,
                                    int32_t *clip_steps_out, void *workspace, long workspace_bytes, int coef_flags,
                                    int launch_flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_RAGGED_H */
