/*
 * liblsm_hip.so — stream endpointing (SPEC.md §1.17): open-ended audio streams cut into utterances on the device.  Every push
 * advances each stream by the whole hops it delivers from a caller-owned state block, and emits the utterances that closed in
 * it into slots laid out as a ragged batch: the slot array and its bin counts go to the ragged launches (lsm_hip_ragged.h,
 * lsm_reservoir_run_ragged, lsm_step_fused_ragged_f64) and to the readout unread.  Every value is specified to the bit: a
 * NumPy restatement (tests/endpoint_restatement.py) reproduces each output byte, and a stream pushed in any split of whole
 * hops gives the utterances of its uncut run.
 *
 * The hop is 160 samples.  Per stream, bins are numbered n = 0, 1, ... from the stream's start (a fresh state block).
 *
 *   energy   e_n = sum over i = 0 .. 159, ascending, of (double)x[160 n + i]^2, one float64 accumulator from +0.0 (lsm_hip_trim.h);
 *            e^_n = e_n if it is finite, else +0.0.
 *   active   E_n = max e^_i over max(0, n - W + 1) <= i <= n.  Bin n is active iff e^_n > E_n * ratio and e^_n > floor: one
 *            float64 multiply, two strict compares.
 *   machine  once per bin, in order; avail starts at 0.
 *              idle:    if active_n: s = max(n - P, avail); f = last = n; mode = speech (then the speech checks, same bin)
 *              speech:  if active_n: last = n
 *                       if n - last == G:      close(end = last + P, cut = 0); avail = end + 1; mode = idle
 *                       elif n - s + 1 == M:   close(end = n, cut = 1);        avail = n + 1;   mode = idle
 *              close:   bins = end - s + 1; KEPT iff cut, or last - f + 1 >= A; otherwise dropped (a click)
 *   finish   a stream whose finish flag is non-zero ends behind the hops of this launch: an open utterance closes with
 *            end = min(last + P, last bin seen), cut = 0 and the flushed flag, by the same keep rule, and the stream's
 *            state_out block is all zeros.
 *   emitted  a kept utterance is the samples [160 s, 160 (end + 1)) of the stream's timeline, moved as words: -0.0 and NaN
 *            payloads survive.  Kept utterances take the stream's slots 0, 1, ... in the order they close.
 *
 * The conventions are those of lsm_hip_audio.h and lsm_hip_trim.h: 0 or a negative LSM_ERR_* code with a thread-local message
 * (lsm_last_error()); caller-owned DEVICE buffers; asynchronous on `stream`; no allocation, no synchronisation, capturable
 * into a HIP graph; no device value is read on the host.  stream_hops, finish and the state block are read by the kernel only
 * and CLAMPED (csrc/endpoint_body.h), so that no value they can hold makes it address outside the launch's buffers.  A state
 * block means what it says only under the window_bins and max_bins it was made with.
 */
#ifndef LSM_HIP_ENDPOINT_H
#define LSM_HIP_ENDPOINT_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of one stream's state block, a multiple of 16: a 64-byte header (64-bit bin counter, the machine's integers), the last
 * window_bins - 1 values e^, the last max_bins bins of audio.  ALL ZEROS IS A FRESH STREAM.  Negative (LSM_ERR_ARG) for
 * window_bins outside 1 .. 1024 or max_bins outside 3 .. 4096.  Host only. */
long lsm_endpoint_state_bytes(int window_bins, int max_bins);

/* 2 + (n_hops - 1) / min(hang_bins + 1, max_bins): the slots per stream a launch needs at least.  One open utterance may
 * close at once; every later one needs an active bin plus hang_bins quiet ones, or max_bins bins; a finish adds one.  Negative
 * (LSM_ERR_ARG) for n_hops outside 1 .. 4096, hang_bins outside 1 .. 1024 or max_bins outside 3 .. 4096.  Host only.
 * Where max_bins >= hang_bins + 3 and max_bins - hang_bins - 1 < pad_bins < 2 hang_bins + 1 - max_bins, a forced cut can
 * follow a close by silence after max(max_bins - pad_bins, max_bins + pad_bins - hang_bins) bins, fewer than the divisor
 * above (SPEC.md §1.17): such a caller passes max_utts = 2 + (n_hops - 1) / that figure.  A kept utterance that finds its
 * stream's slots full is dropped; nothing is written outside them. */
int lsm_endpoint_max_utterances(int n_hops, int hang_bins, int max_bins);

/*   audio            (n_streams, n_hops * 160) float32, 4-byte aligned
 *   stream_hops      (n_streams) int32 or NULL (n_hops everywhere): stream b runs h_b = min(max(v, 0), n_hops) hops, the first
 *                    160 h_b samples of its row
 *   finish           (n_streams) int32 or NULL (no stream ends): non-zero ends the stream behind its h_b hops
 *   ratio            0 <= ratio < 1;  floor  finite, >= 0;  window_bins  W, 1 .. 1024;  pad_bins  P, 0 <= P < M
 *   hang_bins        G, max(P, 1) .. 1024;  min_span_bins  A, 3 .. M;  max_bins  M, 3 .. 4096
 *   state_in         (n_streams, lsm_endpoint_state_bytes) or NULL: every stream is fresh
 *   state_out        the same shape, or NULL: the state is not kept; may be state_in.  A stream with h_b = 0 and no finish
 *                    has its block copied byte for byte
 *   max_utts         slots per stream, >= lsm_endpoint_max_utterances(n_hops, hang_bins, max_bins)
 *   utt_audio_out    (n_streams, max_utts, 160 * M) float32, never audio: slot u < the stream's count holds the utterance at
 *                    the start of its row and the rest of the row is WRITTEN as +0.0; slots at or behind the count are left
 *                    as they are
 *   utt_bins_out     (n_streams, max_utts) int32: bins of the emitted slots, 0 WRITTEN for every other slot -- the
 *                    n_streams * max_utts slots are a ragged batch whose empty clips ride along
 *   utt_first_out    (n_streams, max_utts) int64 or NULL: s of the emitted slots, the others left as they are
 *   utt_flags_out    (n_streams, max_utts) int32 or NULL: bit 0 cut, bit 1 flushed, written like utt_first_out
 *   utt_count_out    (n_streams) int32 or NULL: the emitted slots of each stream
 *   energy_out       (n_streams, n_hops) float64 or NULL: e_n of this push's bins; bins at or behind h_b are left as they are
 *   active_out       (n_streams, n_hops) uint8 or NULL: 1 for an active bin, 0 otherwise, written like energy_out */
int lsm_endpoint_stream_f32(const float *audio, int n_streams, int n_hops, const int32_t *stream_hops, const int32_t *finish,
                            double ratio, double floor, int window_bins, int pad_bins, int hang_bins, int min_span_bins,
                            int max_bins, const void *state_in, void *state_out, int max_utts, float *utt_audio_out,
                            int32_t *utt_bins_out, int64_t *utt_first_out, int32_t *utt_flags_out, int32_t *utt_count_out,
                            double *energy_out, uint8_t *active_out, void *stream);

/* lsm_endpoint_stream_f32 refuses, in this order and before anything is launched: n_streams < 0; n_hops < 1 (LSM_ERR_ARG) or
 * > 4096 (LSM_ERR_UNSUPPORTED: a push's energies and copy records live in one workgroup's LDS); a ratio that is not finite or
 * lies outside [0, 1); a floor that is not finite or is negative; window_bins outside 1 .. 1024; max_bins outside 3 .. 4096;
 * pad_bins outside [0, max_bins); hang_bins outside [max(pad_bins, 1), 1024]; min_span_bins outside [3, max_bins]; max_utts
 * below lsm_endpoint_max_utterances(n_hops, hang_bins, max_bins); a NULL
 * audio, utt_audio_out or utt_bins_out; utt_audio_out == audio; a pointer that is not aligned to its element (the state blocks:
 * 16 bytes).  LSM_ERR_ARG unless said otherwise.  n_streams == 0 then returns 0 and launches nothing. */

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_ENDPOINT_H */
