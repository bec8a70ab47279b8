/*
 * liblsm_hip.so — polyphase FIR resampler (SPEC.md §1.8): float32 or int16 mono PCM at a device's rate in, float32 at the
 * front end's rate out.  A batch form with scipy.signal.resample_poly's centred alignment, and a causal streamed form that
 * continues from a saved per-stream history: a stream cut into calls at any block boundaries gives, byte for byte, the samples
 * and the final state of its one uncut run.
 *
 * The design lives on the host (frontend.resample_table): hp, the prototype filter behind its leading zeros, n_taps float64
 * values in DEVICE memory; up / down, the rate ratio in lowest terms; delay, the batch form's shift in output samples.  The
 * causal sample z[m] of a signal x is, with p = m * down and k0 = p mod up,
 *     acc = +0.0;  for k = k0, k0 + up, ... < n_taps:  acc = acc + hp[k] * x[(p - k) / up];   z[m] = (float)acc
 * in float64 without FMA; x is widened from float32, an int16 sample s is first (float)s * 2^-15; a sample outside the signal
 * is +0.0 and still goes through the multiply and the add.
 *
 * The conventions are those of lsm_hip_audio.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernels clamp the counts they are given.
 */
#ifndef LSM_HIP_RESAMPLE_H
#define LSM_HIP_RESAMPLE_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's state block, a multiple of 16: the stream's last Hs = (n_taps - 1) / up input samples as float32
 * (at least 16 bytes).  A block of zeros is the start of a stream.  0 for n_taps < 1 or up < 1. */
long lsm_resample_state_bytes(int n_taps, int up);

/* Batch form: out[c, m] = z_c[m + delay] for m < n_out, z_c the causal samples of clip c's n_in samples.
 *   audio          (n_clips, n_in) float32 (sample_format 0, 4-byte aligned) or int16 (sample_format 1, 2-byte aligned)
 *   taps_dev       n_taps float64, 8-byte aligned
 *   delay          0 <= delay * down < n_taps; resample_table's D = (half + pre) / down gives resample_poly's alignment
 *   n_out          any length >= 1: ceil(n_in * up / down) is resample_poly's, a smaller one gives its first samples, and
 *                  outputs whose taps lie past the clip's end see zeros there
 *   out            (n_clips, n_out) float32, 4-byte aligned; nothing else is written */
int lsm_resample_f32(const void *audio, int sample_format, int n_clips, int n_in, const double *taps_dev, int n_taps,
                     int up, int down, int delay, int n_out, float *out, void *stream);

/* Streamed form: advance n_streams streams.  n_blocks (G) is the row stride of the call in blocks of `down` input samples:
 * audio is (n_streams, G * down), out (n_streams, G * up), and stream b runs k_b = clamp(stream_blocks[b], 0, G) blocks on
 * the first k_b * down samples of its row, continued from its state block; it writes its first k_b * up samples -- the next
 * samples of the stream's z, nothing skipped and no position stored -- and leaves the rest of its row as it is.
 *   stream_blocks  (n_streams) int32, DEVICE memory, 4-byte aligned, or NULL: every stream runs all G blocks
 *   state_in       (n_streams, lsm_resample_state_bytes) or NULL (= all zeros = every stream starts), 16-byte aligned
 *   state_out      or NULL; may be state_in.  k_b = 0: the stream's state_in block byte for byte */
int lsm_resample_stream_f32(const void *audio, int sample_format, int n_streams, int n_blocks, const double *taps_dev,
                            int n_taps, int up, int down, const int32_t *stream_blocks, const void *state_in,
                            void *state_out, float *out, void *stream);

/* Both return LSM_ERR_ARG, before anything is launched, for up == down, gcd(up, down) != 1, up or down < 1, n_taps < 1, a
 * sample_format other than 0 and 1, a delay that does not fit n_taps, a NULL audio, taps_dev or out, a misaligned pointer,
 * a count below 1 (n_clips, n_in, n_out, n_streams, n_blocks), and for the limits of one call: more than 65 535 rows, or
 * n_blocks * down or n_blocks * up above 2^31 - 1.  LSM_ERR_UNSUPPORTED for a table that does not fit a CU's LDS laid out by
 * phase: up * (ceil(n_taps / up) | 1) * 8 bytes > 160 KB. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_RESAMPLE_H */
