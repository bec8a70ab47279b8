/*
 * liblsm_hip.so — noise mixer in front of the front ends (SPEC.md §1.10): a zero-filled time shift, a level, and a row of a
 * noise bank added at a requested signal-to-noise ratio, for batches of clips and for streams cut anywhere.  Every value is
 * specified to the bit: a NumPy restatement (tests/mix_restatement.py) reproduces each output byte.
 *
 * The arithmetic is float64 without FMA, samples are float32 widened to float64, results are rounded once to float32.
 *
 * Row power P(u) of u[0..n):
 *     p[l] = +0.0 for l = 0..255;  for k = 0, 256, ... ascending and every l with k + l < n:  p[l] = p[l] + u[k+l]*u[k+l]
 *     for s = 128, 64, ..., 1:  p[l] = p[l] + p[l+s] for l < s;   P = p[0]
 *
 * Batch form, clip b of n samples, noise bank (M, L):
 *     s = clamp(shift[b], -n, n);  a = (double)scale[b];  x[i] = a * audio[b, i - s] where 0 <= i - s < n, else +0.0
 *     r = clamp(noise_row[b], 0, M - 1);  o = noise_offset[b] mod L, non-negative;  v[i] = noise[r, (o + i) mod L]
 *     Px = P(x), Pv = P(v), q = ratio[b]  (the host's 10**(-snr_db / 10))
 *     !(q > 0) or !(Pv > 0):  g = 0 and y[i] = (float)x[i]           -- the noise values do not reach y
 *     otherwise:              g = sqrt((Px * q) / Pv) and y[i] = (float)(x[i] + g * v[i])
 *
 * Streamed form, stream b, a row of stride H, its first c = clamp(count[b], 0, H) samples:
 *     a = (double)scale[b];  g = gain[b];  r = clamp(noise_row[b], 0, M - 1);  p = pos_in[b] mod L, non-negative
 *     g == 0:    y[i] = (float)(a * x[i])                            -- the noise is not read
 *     otherwise: y[i] = (float)(a * x[i] + g * noise[r, (p + i) mod L])
 *     pos_out[b] = (p + c) mod L;  the samples behind c are left as they are.  The position is a stream's whole state.
 *
 * The conventions are those of lsm_hip_adaptive.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernels clamp every row, offset, shift, count and position they are given.
 */
#ifndef LSM_HIP_MIX_H
#define LSM_HIP_MIX_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* power_out[j] = P(x[j, :]) for the n_rows rows of x (n_rows, n_samples).  x 4-byte, power_out 8-byte aligned. */
int lsm_mix_power_f32(const float *x, int n_rows, int n_samples, double *power_out, void *stream);

/* The batch form: audio and out (n_clips, n_samples), noise (n_noise_rows, noise_len), all float32 and 4-byte aligned.
 *   noise_row, noise_offset, shift   (n_clips) int32, 4-byte aligned, or NULL: 0 for every clip
 *   scale                            (n_clips) float32, 4-byte aligned, or NULL: 1 for every clip
 *   ratio                            (n_clips) float64, 8-byte aligned
 *   out                              must not be audio: a shift reads across what it would write
 *   gain_out                         (n_clips) float64 or NULL: g
 *   power_out                        (n_clips, 2) float64 or NULL: {Px, Pv} */
int lsm_mix_f32(const float *audio, int n_clips, int n_samples, const float *noise, int n_noise_rows, int noise_len,
                const int32_t *noise_row, const int32_t *noise_offset, const int32_t *shift, const float *scale,
                const double *ratio, float *out, double *gain_out, double *power_out, void *stream);

/* The streamed form: audio and out (n_streams, n_cols) float32, 4-byte aligned; out may be audio.
 *   count      (n_streams) int32 or NULL: every stream mixes all n_cols samples
 *   gain       (n_streams) float64, 8-byte aligned
 *   scale      (n_streams) float32 or NULL: 1
 *   noise_row  (n_streams) int32 or NULL: 0
 *   pos_in     (n_streams) int32 or NULL: 0, every stream starts
 *   pos_out    (n_streams) int32 or NULL; may be pos_in */
int lsm_mix_stream_f32(const float *audio, int n_streams, int n_cols, const float *noise, int n_noise_rows, int noise_len,
                       const int32_t *count, const double *gain, const float *scale, const int32_t *noise_row,
                       const int32_t *pos_in, int32_t *pos_out, float *out, void *stream);

/* All three return LSM_ERR_ARG, before anything is launched, for n_samples (n_cols) outside [1, 2^24], noise_len < 1,
 * n_noise_rows < 1, a negative row count, a misaligned pointer, and -- with a positive row count -- a NULL x, audio, noise,
 * ratio, gain, out or power_out of lsm_mix_power_f32; lsm_mix_f32 also for out == audio.  A row count of 0 returns LSM_OK. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_MIX_H */
