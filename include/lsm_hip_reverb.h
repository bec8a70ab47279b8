/*
 * liblsm_hip.so — reverberation in front of the noise mixer (SPEC.md §1.11): every clip or stream convolved with a row of a
 * bank of room impulse responses, for batches of clips and for streams cut anywhere.  Every value is specified to the bit: a
 * NumPy restatement (tests/reverb_restatement.py) reproduces each output byte.
 *
 * Bank rir (M, K) float32, 1 <= K <= 16384, and rir_len (M) int32 or NULL (K everywhere).  Row r uses the taps
 * h[r, 0 .. len_r), len_r = clamp(rir_len[r], 1, K); a tap at or behind len_r is never read.
 *
 * One sample:
 *     acc = +0.0;  for k = 0, 1, ... < len_r ascending:  acc = acc + (double)h[r, k] * (double)x[i - k];  y[i] = (float)acc
 * in float64, rounded once.  The product of two float32 values is exact in float64, so a fused multiply-add gives the same
 * bits and is what the kernels use.  A sample before the signal's start, or (batch form) at or past its end, is +0.0 and
 * goes through the multiply and the add like any other.
 *
 * Row choice: r = rir_row[b] (NULL: row 0).  r < 0 is a dry row: y is a bitwise copy of x (-0.0 and NaN payloads kept).
 * r >= M is clamped to M - 1.
 *
 * Batch form: audio (n_clips, n_in), out (n_clips, n_out) with any n_out >= 1: n_out = n_in is convolve(x, h)[:n_in],
 * n_out = n_in + K - 1 the full tail.  A dry clip's samples behind n_in are +0.0.
 *
 * Streamed form: stream b convolves the first c = clamp(count[b], 0, n_cols) samples of its row of [history | new
 * samples]; the samples of out behind c are left as they are.  The state of a stream is its last K - 1 input samples as
 * float32 -- K of the bank, not the row's length, so a stream may change its row between pushes -- in a block of
 * lsm_reverb_state_bytes(K) bytes (rounded up to 16, never below 16); all zeros is a stream's start.  c = 0 leaves the
 * block as it is, or copies it when state_out is another buffer.  A dry stream copies its samples and still updates its
 * history.
 *
 * The conventions are those of lsm_hip_mix.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernels clamp every row, length and count they are given.
 */
#ifndef LSM_HIP_REVERB_H
#define LSM_HIP_REVERB_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's state block for a bank of n_taps taps per row; 0 for n_taps outside [1, 16384]. */
long lsm_reverb_state_bytes(int n_taps);

/* The batch form.  audio, rir and out float32, rir_len and rir_row int32, all 4-byte aligned.
 *   n_in      1 .. 2^24;  n_out >= 1;  n_clips <= 65535
 *   rir_len   (n_rir_rows) or NULL: n_taps everywhere
 *   rir_row   (n_clips) or NULL: row 0 for every clip
 *   out       must not be audio */
int lsm_reverb_f32(const float *audio, int n_clips, int n_in, const float *rir, int n_rir_rows, int n_taps,
                   const int32_t *rir_len, const int32_t *rir_row, int n_out, float *out, void *stream);

/* The streamed form.  audio and out (n_streams, n_cols) float32, n_cols 1 .. 2^24, n_streams <= 65535.
 *   count      (n_streams) int32 or NULL: every stream convolves all n_cols samples
 *   state_in   n_streams blocks, 16-byte aligned, or NULL: every stream starts
 *   state_out  n_streams blocks, 16-byte aligned, or NULL: the state is dropped; may be state_in (a kernel of its own
 *              behind the convolution shifts the history)
 *   out        must not be audio */
int lsm_reverb_stream_f32(const float *audio, int n_streams, int n_cols, const float *rir, int n_rir_rows, int n_taps,
                          const int32_t *rir_len, const int32_t *rir_row, const int32_t *count, const void *state_in,
                          void *state_out, float *out, void *stream);

/* Both return LSM_ERR_ARG, before anything is launched, for n_taps outside [1, 16384], n_rir_rows < 1, n_in (n_cols) outside
 * [1, 2^24], n_out < 1, a row count outside [0, 65535], a misaligned pointer, and -- with a positive row count -- a NULL
 * audio, rir or out, or out == audio.  A row count of 0 returns LSM_OK. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_REVERB_H */
