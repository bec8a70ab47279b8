/*
 * liblsm_hip.so — streamed mel front end (SPEC.md §1.7): audio streams in, spike columns out.  One call advances every
 * stream by a number of whole hops of its own, continued from a saved per-stream state, and emits the centred STFT frames
 * those hops completed as raster columns, one time bin per frame; a stream cut into calls at any hop boundaries gives, byte
 * for byte, the raster, power values, dB values and final state of its one uncut run.
 *
 * The conventions are those of lsm_hip_audio.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers, HOST threshold tables; asynchronous on `stream`; no allocation, no
 * synchronisation, and no device value is ever read on the host -- the kernels clamp the counts they are given.
 */
#ifndef LSM_HIP_MEL_STREAM_H
#define LSM_HIP_MEL_STREAM_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's opaque state block, a multiple of 16: the stream's last Hs = (Lg - 1) * hop + n_fft / 2 samples,
 * Lg = ceil((n_fft / 2) / hop), the latch bits of every filter and the count of hops seen (saturating at Lg - 1: the frames
 * that would be centred before the stream's first sample never become columns).  A block of zeros is the start of a stream.
 * 0 for n_mels < 1, n_fft != 2048, hop < n_fft / 16 or hop > n_fft / 2. */
long lsm_mel_stream_state_bytes(int n_mels, int n_fft, int hop);

/* Bytes of the scratch one call needs (the power values of its frames); 0 for n_streams < 0, n_mels < 1 or n_hops < 1. */
long lsm_mel_stream_workspace(int n_streams, int n_mels, int n_hops);

/* Advance n_streams streams.  n_hops (H) is the row stride of the call: audio is (n_streams, H * hop) float32, and stream b
 * runs h_b = clamp(stream_hops[b], 0, H) hops on the first h_b * hop samples of its row, continued from its state block.
 * Frame t of a stream is its samples [t * hop - n_fft / 2, t * hop + n_fft / 2), zeros before the stream's start; window,
 * transform and mel projection are lsm_mel_power_f32's, value for value.
 *   window_dev, twiddle_dev, basis_dev, lo_dev, hi_dev, n_mels   the tables of lsm_mel_power_f32
 *   stream_hops   (n_streams) int32, DEVICE memory, 4-byte aligned, or NULL: every stream runs all H hops
 *   db_lo, db_hi  the calibration range in ABSOLUTE dB, db_lo < db_hi, both finite, rounded to float32 once and fixed for the
 *                 stream's life: a frame's value is v = 10 * log10(max(1e-10, S)) (NaN for a NaN power value), floored at
 *                 db_hi - 80, and normalised as (v - db_lo) / (db_hi - db_lo + 1e-8), all in float32; values outside [0, 1]
 *                 are not clipped
 *   thr_on, thr_off   HOST tables of n_thr (1..8) float32 on- and off-thresholds, as lsm_encode_hysteresis_f32's
 *   state_in      (n_streams, lsm_mel_stream_state_bytes) or NULL (= all zeros = every stream starts), 16-byte aligned
 *   state_out     or NULL; may be state_in.  h_b = 0: the stream's state_in block byte for byte
 *   raster_out    (n_streams, n_mels * redundancy, H * n_thr) uint8, required, 4-byte aligned: byte [channel, c * n_thr + k]
 *                 is latch k after column c.  A stream that had seen s hops and runs h_b more completes
 *                 cols_b = complete(s + h_b) - complete(s) frames, complete(n) = max(0, n - Lg + 1); it writes the first
 *                 cols_b * n_thr bytes of its rows, the rest is left as it is
 *   power_out, db_out   or NULL; (n_streams, n_mels, H) float32: the frames' mel power and their un-floored dB values v,
 *                 written the same way
 *   workspace     lsm_mel_stream_workspace(n_streams, n_mels, H) bytes, 16-byte aligned; calls that may overlap (different
 *                 `stream`s) need one each
 * LSM_ERR_ARG, before anything is written, for n_fft != 2048, hop outside [n_fft / 16, n_fft / 2], n_mels < 1, n_hops < 1,
 * !(db_lo < db_hi) or a bound that is not finite (as float32 values too), a NULL raster_out, a workspace that is too small,
 * a misaligned pointer, n_thr outside [1, 8], redundancy < 1, and for the limits of one call: n_streams outside
 * [0, 65535] (one grid row per stream) and n_hops * hop > 2^31 - 1 samples per row.  n_streams = 0 is LSM_OK and does nothing. */
int lsm_mel_stream_f32(const float *audio, int n_streams, int n_hops, int n_fft, int hop, const double *window_dev,
                       const double *twiddle_dev, const float *basis_dev, const int32_t *lo_dev, const int32_t *hi_dev,
                       int n_mels, const int32_t *stream_hops, double db_lo, double db_hi, const float *thr_on,
                       const float *thr_off, int n_thr, int redundancy, const void *state_in, void *state_out,
                       uint8_t *raster_out, float *power_out, float *db_out, void *workspace, long workspace_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_MEL_STREAM_H */
