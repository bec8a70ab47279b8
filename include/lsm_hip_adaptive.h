/*
 * liblsm_hip.so — adaptive-range spike encoder for streamed front ends (SPEC.md §1.9): the dB columns a streamed front end
 * completed (the db_out of lsm_gammatone_stream_f64 or lsm_mel_stream_f32) are normalised with the minimum and maximum of the
 * stream's last window_cols columns -- the causal form of the reference's per-clip range -- and go through the hysteresis
 * encoder of SPEC.md §1.3, continued from a saved per-stream state.  A stream cut into calls anywhere gives, byte for byte, the
 * raster, the ranges and the final state of its one uncut run.
 *
 * Per column c of a stream (counted from its start), in the dB array's type T and in this order, without FMA:
 *     cmax[c] = max_f v[f, c], cmin[c] = min_f v[f, c]      taken with > and <: a NaN is skipped; none left: -inf and +inf
 *     hi = max cmax, mn = min cmin over columns max(0, c - window_cols + 1) .. c
 *     fl = hi - 80;  lo = mn > fl ? mn : fl
 *     (hi - lo) < 1e-8:  norm = 0 for every filter of the column
 *     otherwise          vf = v < fl ? fl : v;  norm = (vf - lo) / ((hi - lo) + 1e-8)
 * then per threshold k the latch of §1.3 on norm (a NaN leaves it as it is), byte [channel, c * n_thr + k].
 *
 * The conventions are those of lsm_hip_audio.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers, the threshold tables in HOST memory; asynchronous on `stream`; no
 * allocation, no synchronisation, and no device value is ever read on the host -- the kernel clamps the counts it is given.
 */
#ifndef LSM_HIP_ADAPTIVE_H
#define LSM_HIP_ADAPTIVE_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's state block, a multiple of 16: the cmin and the cmax of the at most window_cols - 1 carried columns
 * (oldest first, unused slots zero) as elem_bytes-wide floats, a latch word per filter and the count of carried columns.  A
 * block of zeros is the start of a stream.  0 for arguments the encoder refuses: n_filters outside [1, 16384], window_cols
 * outside [1, 4096], elem_bytes other than 4 (float) and 8 (double). */
long lsm_adaptive_state_bytes(int n_filters, int window_cols, int elem_bytes);

/* Advance n_streams streams.  n_cols (H) is the row stride of the call: db is (n_streams, n_filters, H), raster_out
 * (n_streams, n_filters * redundancy, H * n_thr), lo_out / hi_out (n_streams, H).  Stream b encodes its first
 * k_b = clamp(stream_cols[b], 0, H) columns, continued from its state block, and leaves the rest of its rows as they are.
 *   db             8-byte aligned; the un-floored dB values of SPEC.md §1.6
 *   stream_cols    (n_streams) int32, DEVICE memory, 4-byte aligned, or NULL: every stream encodes all H columns
 *   thr_on/thr_off n_thr HOST values each (frontend.threshold_tables), n_thr in [1, 8]
 *   state_in       (n_streams, lsm_adaptive_state_bytes) or NULL (= all zeros = every stream starts), 16-byte aligned
 *   state_out      or NULL; may be state_in.  k_b = 0: the stream's state_in block byte for byte
 *   raster_out     4-byte aligned
 *   lo_out/hi_out  or NULL: the range (lo, hi) column c was normalised with, written like the raster */
int lsm_adaptive_encode_f64(const double *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols,
                            int window_cols, const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                            const void *state_in, void *state_out, uint8_t *raster_out,
                            double *lo_out, double *hi_out, void *stream);

/* The same in float32 (4-byte aligned db, lo_out, hi_out): the absolute dB values of SPEC.md §1.7. */
int lsm_adaptive_encode_f32(const float *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols,
                            int window_cols, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                            const void *state_in, void *state_out, uint8_t *raster_out,
                            float *lo_out, float *hi_out, void *stream);

/* Both return LSM_ERR_ARG, before anything is launched, for n_filters outside [1, 16384], window_cols outside [1, 4096],
 * n_cols < 1, n_streams < 0, n_thr outside [1, 8], redundancy < 1, a NULL threshold table, a NULL raster_out, a NULL db with
 * n_streams > 0, and a misaligned pointer.  n_streams == 0 returns LSM_OK. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_ADAPTIVE_H */
