/*
 * liblsm_hip.so — streamed gammatone front end (SPEC.md §1.6): audio streams in, spike columns out.  One launch advances
 * every stream by a number of whole hops of its own, continued from a saved per-stream state, and emits the spectrogram
 * columns those hops completed as raster columns; a stream cut into launches at any hop boundaries gives, bit for bit, the
 * raster of its one uncut run.
 *
 * The conventions are those of lsm_hip_streams.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers, HOST threshold tables; asynchronous on `stream`; no allocation, no
 * synchronisation, and no device value is ever read on the host -- the kernel clamps the counts it is given.
 */
#ifndef LSM_HIP_AUDIO_H
#define LSM_HIP_AUDIO_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's opaque state block, a multiple of 16: per channel the eight filter doubles, the
 * ceil(nwin / hop) - 1 window sums open across a launch boundary, the latch bits and the count of hops seen (saturating at
 * ceil(nwin / hop) - 1: the windows that would have begun before the stream's first sample never close as columns).  A block
 * of zeros is the start of a stream.  0 for n_filters < 2, hop < 1, nwin < hop or nwin > 4 * hop. */
long lsm_gammatone_stream_state_bytes(int n_filters, int nwin, int hop);

/* Advance n_streams streams.  n_hops (H) is the row stride of the launch: audio is (n_streams, H * hop) float32, and stream b
 * runs h_b = clamp(stream_hops[b], 0, H) hops on the first h_b * hop samples of its row, continued from its state block.
 *   coefs         (n_filters, 10) float64 as lsm_gammatone_spec_f64's; coef_flags likewise
 *   stream_hops   (n_streams) int32, DEVICE memory, 4-byte aligned, or NULL: every stream runs all H hops
 *   db_lo, db_hi  the calibration range, db_lo < db_hi, both finite, fixed for the stream's life: a column's value is
 *                 v = 20 * log10(col + 1e-9), floored at db_hi - 80, and normalised as (v - db_lo) / (db_hi - db_lo + 1e-8);
 *                 values outside [0, 1] are not clipped
 *   thr_on, thr_off   HOST tables of n_thr (1..8) on- and off-thresholds, as lsm_encode_hysteresis_f64's
 *   state_in      (n_streams, lsm_gammatone_stream_state_bytes) or NULL (= all zeros = every stream starts), 16-byte aligned
 *   state_out     or NULL; may be state_in.  h_b = 0: the stream's state_in block byte for byte
 *   raster_out    (n_streams, n_filters * redundancy, H * n_thr) uint8, required, 4-byte aligned: byte [channel, c * n_thr + k]
 *                 is latch k after column c.  A stream that had seen s hops and runs h_b more completes
 *                 cols_b = complete(s + h_b) - complete(s) columns, complete(n) = 0 for n * hop < nwin, else
 *                 (n * hop - nwin) / hop + 1; it writes the first cols_b * n_thr bytes of its rows, the rest is left as it is
 *   spec_out, db_out   or NULL; (n_streams, n_filters, H) float64: the columns and their dB values, written the same way
 * LSM_ERR_ARG for n_filters < 2, nwin > 4 * hop, nwin < hop, n_hops < 1, !(db_lo < db_hi) or a bound that is not finite, a
 * misaligned pointer, a NULL raster_out, n_thr outside [1, 8] and redundancy < 1. */
int lsm_gammatone_stream_f64(const float *audio, int n_streams, int n_hops, const double *coefs, int n_filters, int nwin,
                             int hop, const int32_t *stream_hops, double db_lo, double db_hi, const double *thr_on,
                             const double *thr_off, int n_thr, int redundancy, const void *state_in, void *state_out,
                             uint8_t *raster_out, double *spec_out, double *db_out, int coef_flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_AUDIO_H */
