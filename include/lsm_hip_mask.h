/*
 * liblsm_hip.so — SpecAugment-style frequency and time masks inside the spike encoders (SPEC.md §1.13).  Each function is
 * its unmasked twin of lsm_hip.h with `freq_mask, time_mask` inserted before `stream`; every other parameter, the workspace
 * size, the layout choice (lsm_gammatone_spikes_layout answers for both) and launch_flags are the twin's.
 *
 * Per clip c two bit sets: fm_c, one bit per filter row f < n_filters (before redundancy), and tm_c, one bit per time bin
 * j < time_bins.  With S the clip's normalised, resized spectrogram (what norm_out shows):
 *     S'[f, j] = +0.0 if fm_c[f] or tm_c[j] else S[f, j]
 * and the raster is the hysteresis encoder on S'.  Maximum, floor, minimum, the flat test and the resize are those of the
 * unmasked clip; the mask replaces a value where the "last bin outside the input is +0.0" rule does.  The value 0.0 is compared
 * with the thresholds like any other.  norm_out, where a function has it, shows S'.  A NumPy restatement
 * (tests/mask_restatement.py) reproduces each output byte.
 *
 *   freq_mask      DEVICE memory, (n_clips, ceil(n_filters / 32)) uint32, 4-byte aligned, or NULL: no frequency mask.
 *                  Row f is bit f & 31 of word f >> 5; bits at or beyond n_filters are ignored.
 *   time_mask      DEVICE memory, (n_clips, ceil(time_bins / 32)) uint32, 4-byte aligned, or NULL: no time mask.
 *                  Bin j is bit j & 31 of word j >> 5; bits at or beyond time_bins are ignored.
 *
 * With both NULL, or all bits clear, the output is byte for byte the twin's.
 *
 * The conventions are those of lsm_hip_speed.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host.  The twin's refusals apply unchanged and in the twin's order; after them, and before
 * anything is launched, LSM_ERR_ARG for a mask pointer that is not 4-byte aligned.
 */
#ifndef LSM_HIP_MASK_H
#define LSM_HIP_MASK_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lsm_spec_to_spikes_masked_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins, int apply_floor,
                                  const double *thr_on, const double *thr_off, int n_thr, int redundancy, uint8_t *raster,
                                  double *norm_out, const uint32_t *freq_mask, const uint32_t *time_mask, void *stream);

int lsm_spec_to_spikes_masked_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins, int apply_floor,
                                  const float *thr_on, const float *thr_off, int n_thr, int redundancy, uint8_t *raster,
                                  float *norm_out, const uint32_t *freq_mask, const uint32_t *time_mask, void *stream);

int lsm_gammatone_spikes_masked_f64(const float *audio, int n_clips, int n_samples, const double *coefs_dev, int n_filters,
                                    int nwin, int hop, int ncols, int time_bins, const double *thr_on, const double *thr_off,
                                    int n_thr, int redundancy, uint8_t *raster, void *workspace, long workspace_bytes,
                                    int coef_flags, int launch_flags, const uint32_t *freq_mask, const uint32_t *time_mask,
                                    void *stream);

int lsm_mel_spikes_masked_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop, int n_frames,
                              const double *window_dev, const double *twiddle_dev, const float *basis_dev,
                              const int32_t *lo_dev, const int32_t *hi_dev, int n_mels, float amin, float top_db,
                              int time_bins, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                              uint8_t *raster, void *workspace, long workspace_bytes, const uint32_t *freq_mask,
                              const uint32_t *time_mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_MASK_H */
