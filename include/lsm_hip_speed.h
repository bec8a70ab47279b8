/*
 * liblsm_hip.so — speed perturbation in front of the reverberation (SPEC.md §1.12): every clip of a batch played at its own
 * speed, in one launch.  A clip played s times faster is the clip resampled from 16000 * s Hz to 16000 Hz, so the arithmetic
 * is that of lsm_hip_resample.h's batch form, over a bank of up to 16 designs.  Every value is specified to the bit: a NumPy
 * restatement (tests/speed_restatement.py) reproduces each output byte.
 *
 * Bank: the designs' taps (frontend.resample_table) one behind the other, n_taps_total float64 values in DEVICE memory, and
 * `designs`, n_designs rows of five int32 in HOST memory: up, down, n_taps, delay, tap_offset -- design r uses
 * taps_dev[tap_offset .. tap_offset + n_taps).  The rows are read on the host, checked, and travel to the kernel by value.
 *
 * Row choice: r = design_row[c] (NULL: row 0).
 *   0 <= r      design min(r, n_designs - 1):  out[c, m] = z_c[m + delay] for m < n_out, z_c the causal sample of
 *               lsm_hip_resample.h on that design: float64, no FMA, taps in ascending k, a sample outside [0, n_in) is +0.0
 *               and still multiplied and added, one rounding to float32.  The first ceil(n_in * up / down) outputs are
 *               scipy.signal.resample_poly's; behind them the filter rings out over zeros; from
 *               m >= ceil((n_in + Hs) * up / down), Hs = (n_taps - 1) / up, every output is +0.0.
 *               PRECONDITION: every tap is finite (a NaN or an infinite tap times +0.0 is NaN; the kernel stores +0.0 there).
 *   r < 0       an unperturbed clip: out[c, m] is the input's bits for m < min(n_in, n_out), an int16 sample s widened as
 *               (float)s * 2^-15; +0.0 behind.
 *
 * The conventions are those of lsm_hip_reverb.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernel clamps every row it is given.
 */
#ifndef LSM_HIP_SPEED_H
#define LSM_HIP_SPEED_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LDS bytes a launch over these designs takes (the largest table laid out by phase, up * (ceil(n_taps / up) | 1) * 8);
 * 0 if any design would be refused, or n_designs lies outside [1, 16].  Host only. */
long lsm_speed_lds_bytes(const int32_t *designs, int n_designs);

/*   audio          (n_clips, n_in) float32 (sample_format 0, 4-byte aligned) or int16 (sample_format 1, 2-byte aligned)
 *   taps_dev       n_taps_total float64, 8-byte aligned
 *   designs        HOST memory, (n_designs, 5): up, down, n_taps, delay, tap_offset;  n_designs 1 .. 16
 *   design_row     DEVICE memory, (n_clips) int32, 4-byte aligned, or NULL: row 0 for every clip
 *   out            (n_clips, n_out) float32, 4-byte aligned, never audio; nothing else is written */
int lsm_speed_f32(const void *audio, int sample_format, int n_clips, int n_in, const double *taps_dev, int n_taps_total,
                  const int32_t *designs, int n_designs, const int32_t *design_row, int n_out, float *out, void *stream);

/* lsm_speed_f32 returns LSM_ERR_ARG, before anything is launched, for n_designs outside [1, 16]; for a design with up or
 * down < 1, up == down, gcd(up, down) != 1, n_taps < 1, a delay outside 0 <= delay * down < n_taps, tap_offset < 0 or
 * tap_offset + n_taps > n_taps_total; for a sample_format other than 0 and 1; a NULL audio, taps_dev, designs or out; a
 * misaligned pointer; out == audio; a count below 1 (n_clips, n_in, n_out, n_taps_total); and n_clips > 65 535.
 * LSM_ERR_UNSUPPORTED for a design whose table does not fit a CU's LDS: more than 160 KB. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_SPEED_H */
