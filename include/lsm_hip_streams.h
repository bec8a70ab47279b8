/*
 * liblsm_hip.so — open-ended streams (SPEC.md §4d): sliding-window features of streams at any positions, advancing by any
 * number of whole segments, in one ragged launch, with no limit on a stream's length.
 *
 * The conventions are those of lsm_hip.h: 0 or a negative LSM_ERR_* code with a thread-local message (lsm_last_error());
 * caller-owned DEVICE buffers, HOST key_ids; asynchronous on `stream`; no allocation, no synchronisation, and no device
 * value is ever read on the host -- the kernels clamp the counts they are given.
 */
#ifndef LSM_HIP_STREAMS_H
#define LSM_HIP_STREAMS_H

#include "lsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A stream launch: lsm_reservoir_run_segments that keeps no cumulative feature record and whose clips run a number of whole
 * segments of their own.  n_steps is the row stride of the launch -- spikes_u8 is (n_clips, C, n_steps), the spike matrix and
 * the membrane trace (n_clips, n_steps, N) --, G = n_steps / segment_steps, and clip b runs G_b = clamp(clip_segments[b], 0, G)
 * segments, L_b = G_b * segment_steps steps, continued from its state_in block as lsm_reservoir_run_from continues.
 *   clip_segments  (n_clips) int32, DEVICE memory, 4-byte aligned, or NULL: every clip runs all G segments
 *   state_in       (n_clips, lsm_reservoir_state_bytes) or NULL (= all zeros = reset()); its feature-record block is not read
 *   state_out      or NULL; may be state_in.  Clip b with G_b >= 1: the state after its last step -- potentials, countdowns,
 *                  last step's spikes, "fired at least once", the spike total modulo 2^32 -- with the feature-record block
 *                  written as zeros.  G_b = 0: its state_in block byte for byte (zeros when state_in is NULL; nothing when
 *                  state_out == state_in)
 *   records_out    (n_clips, G, n_out) x 16 bytes, 16-byte aligned, required: record g < G_b of clip b is
 *                  lsm_reservoir_run_segments' record of its steps [g * segment_steps, (g + 1) * segment_steps) of this launch,
 *                  on times local to the segment; records at g >= G_b are left as they are
 *   spike_matrix_out, v_trace_out   or NULL; clip b: rows 0 .. L_b - 1 are written, rows from L_b on are left as they are
 *   stats_out      or NULL; (n_clips, 2) {neurons that fired at least once, spike total as a 32-bit pattern} since the state
 *                  was last all zeros; the row of a clip with G_b = 0 is left as it is
 *   order_workspace   as lsm_reservoir_run_from's; the clips are ranked by their input spikes at t < L_b
 * Clip b is, bit for bit, that clip alone in a segmented launch of L_b steps; input bytes at t >= L_b influence nothing.  There
 * is no first_step and there are no cumulative features: nothing in the launch depends on where a clip is on its own timeline,
 * so streams at different positions share a launch, records of consecutive launches concatenate per clip in that clip's own
 * order, and a stream has no length limit.  What remains are the limits of one launch (n_steps <= 65535 and the plan's LDS
 * image: lsm_reservoir_plan, lsm_reservoir_max_steps) and of one window (below).
 * LSM_ERR_ARG for segment_steps < 1, n_steps % segment_steps != 0, a NULL or misaligned records_out, a misaligned
 * clip_segments, a state pointer that is not 16-byte aligned, and the argument checks of lsm_reservoir_run_from. */
int lsm_reservoir_run_stream(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                             int segment_steps, const int32_t *clip_segments, const void *state_in, void *state_out,
                             void *records_out, uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                             int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream);

/* lsm_segment_features over records of which every clip has a valid count of its own: records is (n_clips, n_segments, n_out)
 * x 16 bytes, clip b's first Gv_b = clamp(clip_segments[b], 0, n_segments) records are valid, and it has
 * W_b = (Gv_b - window_segments) / hop_segments + 1 windows (none when Gv_b < window_segments).
 *   clip_segments  (n_clips) int32, DEVICE memory, 4-byte aligned, required
 *   features_out   (n_clips, W, n_keys * n_out) float32, key-major rows, W = (n_segments - window_segments) / hop_segments + 1:
 *                  row w < W_b of clip b is lsm_segment_features' row; rows at w >= W_b are left as they are
 * LSM_ERR_ARG for a NULL or misaligned clip_segments, window_segments * segment_steps > 65535, and lsm_segment_features'
 * refusals. */
int lsm_segment_features_ragged(const lsm_reservoir *h, const void *records, int n_clips, int n_segments,
                                const int32_t *clip_segments, int segment_steps, int window_segments, int hop_segments,
                                const int32_t *key_ids, int n_keys, float *features_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_STREAMS_H */
