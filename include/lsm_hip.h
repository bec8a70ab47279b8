/*
 * liblsm_hip.so — C ABI of the MI355X (gfx950) hot path of the LSM speech pipeline.
 *
 * The reference (adelitoo/lsm-speech-classifier) is pure Python and has no FFI of its own; the
 * seam this library sits behind is the set of Python call sites listed per function below
 * (file:line under /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative LSM_ERR_* code; lsm_last_error() gives
 *     the thread-local message of the last failure on the calling thread;
 *   - every pointer named *_dev / audio / db / spikes / *_out is DEVICE memory owned by the
 *     caller (e.g. torch.Tensor.data_ptr()); tables named coefs / thr_* / key_ids and every
 *     argument of lsm_reservoir_create are HOST memory, copied during the call;
 *   - every launch function takes a hipStream_t as `void *stream` and is asynchronous on it;
 *     none of them allocates, frees or synchronises, and after a kernel's first use its launch is the
 *     only runtime call made (safe under hipGraph capture: tests/test_gpu_graph.py);
 *   - the only device memory the library owns is inside an lsm_reservoir handle;
 *   - no global mutable state: distinct handles/streams may be used from distinct threads.
 */
#ifndef LSM_HIP_H
#define LSM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_OK 0
#define LSM_ERR_ARG (-1)
#define LSM_ERR_HIP (-2)
#define LSM_ERR_NOMEM (-3)
#define LSM_ERR_UNSUPPORTED (-4)

int lsm_version(void);                 /* major*10000 + minor*100 + patch of the package version the library was built as */
/* "LSM_BUILD_ID=<24 hex digits>": hash of every source and header of csrc/, this header, the compiler flags and the
 * version, linked in by lsm-speech-classifier_amd/build.py.  The Python loader refuses a library whose id is not the one
 * of the tree it sits in (a stale binary cannot pass for a build of the sources beside it). */
const char *lsm_build_id(void);
const char *lsm_last_error(void);
int lsm_device_count(void);

/* ---- front end ------------------------------------------------------------------------- */

/* Replaces gammatone.gtgram.gtgram(wave, fs, window_time, hop_time, channels, f_min) as called
 * at create_dataset.py:51-58, plus the dB conversion of create_dataset.py:59.
 *   audio   (n_clips, n_samples) float32, device
 *   coefs   (n_filters, 10) float64, HOST-side values uploaded by the caller to DEVICE memory:
 *           rows [A0, A11, A12, A13, A14, A2, B0, B1, B2, gain], low -> high centre frequency
 *   spec_out (n_clips, n_filters, ncols) float64 or NULL: sqrt(mean of squared filter output)
 *   db_out   (n_clips, n_filters, ncols) float64 or NULL: 20*log10(spec + 1e-9)
 * nwin/hop are in samples (400/160 for the reference call), nwin <= 4*hop.
 * coef_flags (properties of the coefficient table the HOST has verified; 0 is always valid):
 *   bit 0  every A2 is exactly 0  -> the x*A2 products (signed zeros) are not evaluated
 *   bit 1  no gain has an all-ones significand -> y/gain through the exact Markstein FMA sequence
 *   bit 2  A0/B0 is the same float64 for every channel (lsm_gammatone_spikes_f64 only: the product with the sample
 *          is then formed once for the two channels a lane carries) */
int lsm_gammatone_spec_f64(const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                           int n_filters, int nwin, int hop, int ncols, double *spec_out,
                           double *db_out, int coef_flags, void *stream);

/* The whole gammatone front end of one clip in ONE launch: replaces the per-clip body of the loop at
 * create_dataset.py:143-157 -- audio_to_spectrogram (gammatone branch, :49-78: gtgram, dB, max-80 floor,
 * min-max normalise with eps 1e-8, flat input -> zeros, scipy zoom(order=1) to time_bins columns, crop),
 * convert_spectrogram_to_spikes_hysteresis (:81-98) and create_pure_redundancy (:101-104).  Same results,
 * bit for bit, as lsm_gammatone_spec_f64 followed by lsm_spec_to_spikes_f64(apply_floor = 1), without the
 * (n_clips, n_filters, ncols) float64 hand-off between two launches.
 *   audio, coefs_dev, nwin/hop/ncols, coef_flags   as lsm_gammatone_spec_f64
 *   thr_on/thr_off/n_thr/redundancy/raster         as lsm_spec_to_spikes_f64 (raster must not be NULL)
 *   workspace   DEVICE scratch of at least lsm_gammatone_spikes_workspace(n_clips, n_filters, ncols) bytes,
 *               8-byte aligned, owned by the caller, contents undefined before and after the call
 *   launch_flags bit 0: low-latency layout -- one channel group per wave instead of two: twice the waves, each half
 *               as long (for a launch onto an idle GPU: 1.47 instead of 2.43 ms per 256 clips x 128 filters, 12 % more
 *               CU time); above 512 filters the flag is ignored (the one-chain layout would need more than 8 waves
 *               per clip).  bit 1: no LDS reservation -- a launch of at most one workgroup per CU normally reserves
 *               half a CU's LDS so that overlapping launches spread one workgroup per CU; beside a kernel whose
 *               workgroups need most of the LDS themselves (the ring-row reservoir kernel) the caller sets this bit and
 *               the launch asks for what it uses (27 KB per 4-wave workgroup at 4 thresholds x 100 bins).
 *               Results do not depend on the flags.  0 = the throughput layout with the reservation.  Where the
 *               lane pair applies (lsm_gammatone_spikes_layout() == 0) bit 0 changes nothing and no LDS is reserved.
 * Returns LSM_ERR_UNSUPPORTED for more than 1024 filters (use the two split entry points). */
long lsm_gammatone_spikes_workspace(int n_clips, int n_filters, int ncols);
/* The layout lsm_gammatone_spikes_f64 launches for n_clips x n_filters with these launch_flags on the current device and
 * this process's hardware queues (GPU_MAX_HW_QUEUES, 4 where unset): 0 = lane pair (32 channels per wave, filter
 * sections 1-2 and 3-4 on the two halves of a wave; 2..256 filters with at most 4 queues, unless the batch fills every
 * SIMD without it), 1 / 2 = one / two 64-channel groups per lane.  LSM_ERR_ARG for a bad shape, LSM_ERR_UNSUPPORTED where
 * lsm_gammatone_spikes_f64 refuses.  Informational: results do not depend on the layout. */
int lsm_gammatone_spikes_layout(int n_clips, int n_filters, int launch_flags);
int lsm_gammatone_spikes_f64(const float *audio, int n_clips, int n_samples, const double *coefs_dev,
                             int n_filters, int nwin, int hop, int ncols, int time_bins,
                             const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                             uint8_t *raster, void *workspace, long workspace_bytes, int coef_flags,
                             int launch_flags, void *stream);

/* Replaces create_dataset.py:60 (apply_floor: max-80 dB floor), :62-78 (min-max normalise with
 * eps 1e-8, flat input -> zeros, scipy zoom(order=1) to time_bins columns, crop), :81-98
 * (hysteresis encoder) and :101-104 (row repeat), one clip per workgroup.
 *   db      (n_clips, n_filters, ncols) device
 *   thr_on  n_thr ON thresholds sorted DESCENDING, thr_off the matching `thr - gap` values, both
 *           already rounded to the spectrogram dtype by the caller (HOST memory, <= 8 entries)
 *   raster  (n_clips, n_filters*redundancy, time_bins*n_thr) uint8 or NULL
 *   norm_out (n_clips, n_filters, time_bins) or NULL: the normalised, resized spectrogram
 * The resize (taken when ncols != time_bins) is scipy.ndimage.zoom's, its boundary included: where the last bin's
 * coordinate (double)(time_bins-1) * zf, zf = (double)(ncols-1) / (double)(time_bins-1), is greater than (double)(ncols-1),
 * it lies outside the input and the last bin's normalised value is +0.0 for every row, NaN rows included, before the
 * threshold comparisons (SPEC.md 1.2; e.g. 105 or 58 columns to 100 bins).  The one-launch entry points
 * (lsm_gammatone_spikes_f64, lsm_mel_spikes_f32) do the same.
 * LSM_ERR_ARG when the latch bit rows (64 rows x max(n_thr, 1) x ceil(time_bins / 32) words, twice, + 128 bytes) exceed
 * 160 KB of LDS: 8 thresholds fit up to 1248 time bins. */
int lsm_spec_to_spikes_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins,
                           int apply_floor, const double *thr_on, const double *thr_off, int n_thr,
                           int redundancy, uint8_t *raster, double *norm_out, void *stream);
int lsm_spec_to_spikes_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins,
                           int apply_floor, const float *thr_on, const float *thr_off, int n_thr,
                           int redundancy, uint8_t *raster, float *norm_out, void *stream);

/* Replaces librosa.feature.melspectrogram(y, sr=16000, n_mels, hop_length) as called at
 * create_dataset.py:44-47 (n_fft must be 2048, librosa's default): centred zero-padded frames,
 * float64 window x float32 frame, float64 FFT stored as complex64, |.|^2 in float32, mel basis.
 *   window_dev (n_fft) f64, twiddle_dev (n_fft/2, 2) f64 {cos, -sin}, basis_dev (n_mels, n_fft/2+1)
 *   f32, lo_dev/hi_dev (n_mels) i32 non-zero bin range of each filter: DEVICE tables built by the host;
 *   window_dev and twiddle_dev 16-byte aligned (the kernel fetches them two doubles at a time).
 *   Filter m sums basis[m, f] * P[f] over its half-open range lo[m] <= f < hi[m] and reads nothing of its row outside it;
 *   every range must satisfy 0 <= lo <= hi <= n_fft/2+1 (lo == hi: an empty filter, +0.0).  The ranges are device arrays
 *   and are NOT checked: a range outside these limits reads outside the basis and the spectrum.
 *   power_out (n_clips, n_mels, n_frames) float32, n_frames = 1 + n_samples / hop */
int lsm_mel_power_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop,
                      int n_frames, const double *window_dev, const double *twiddle_dev,
                      const float *basis_dev, const int32_t *lo_dev, const int32_t *hi_dev,
                      int n_mels, float *power_out, void *stream);

/* The whole mel front end of a batch in ONE launch: melspectrogram (as lsm_mel_power_f32) -> power_to_db(ref=max) ->
 * min-max normalise -> resize to time_bins columns -> hysteresis encoder -> row repeat (create_dataset.py:43-48 and
 * :62-104 per clip).  Rasters equal those of lsm_mel_power_f32 + lsm_power_to_db_f32 + lsm_spec_to_spikes_f32 bit for
 * bit (same code).  The workgroup that finishes a clip's last frame finishes the clip; nothing waits.
 *   workspace        caller-owned, 256-byte aligned, >= lsm_mel_spikes_workspace(n_clips, n_mels, n_frames) bytes;
 *                    its first n_clips*4 bytes (one counter per clip) must be ZERO on entry and are zero again when
 *                    the launch has finished (allocate once with zeros, reuse for ever -- stream-ordered launches only)
 *   raster           (n_clips, n_mels*redundancy, time_bins*n_thr) uint8
 * LSM_ERR_UNSUPPORTED when the latch bit rows of the finishing workgroup (64 rows x n_thr x ceil(time_bins / 32) words, twice)
 * exceed the kernel's 68 KB of LDS (more than ~1000 time bins at 4 thresholds; any number of filters fits): use the three
 * split entry points. */
long lsm_mel_spikes_workspace(int n_clips, int n_mels, int n_frames);
int lsm_mel_spikes_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop, int n_frames,
                       const double *window_dev, const double *twiddle_dev, const float *basis_dev,
                       const int32_t *lo_dev, const int32_t *hi_dev, int n_mels, float amin, float top_db,
                       int time_bins, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                       uint8_t *raster, void *workspace, long workspace_bytes, void *stream);

/* Replaces librosa.power_to_db(S, ref=np.max) (create_dataset.py:48) per clip, float32:
 * 10*log10(max(amin, S)) - 10*log10(max(amin, max S)), floored at -top_db. */
int lsm_power_to_db_f32(const float *power, int n_clips, int n_per_clip, float amin, float top_db,
                        float *db_out, void *stream);

/* Replaces convert_spectrogram_to_spikes_hysteresis (create_dataset.py:81-98) on an already
 * normalised spectrogram: spec (n_rows, n_bins) -> out (n_rows, n_bins*n_thr) uint8. */
int lsm_encode_hysteresis_f64(const double *spec, int n_rows, int n_bins, const double *thr_on,
                              const double *thr_off, int n_thr, uint8_t *out, void *stream);
int lsm_encode_hysteresis_f32(const float *spec, int n_rows, int n_bins, const float *thr_on,
                              const float *thr_off, int n_thr, uint8_t *out, void *stream);

/* Bit-packed rasters: the packed variant of File 1 (same content as the X_spikes
 * array written by /root/reference/create_dataset.py:168-176, 8x smaller on disk and over PCIe).
 * raster (n_rows, n_steps) uint8, any non-zero byte is a spike; packed (n_rows, ceil(n_steps/8)) uint8,
 * time step 8q+k of a row in bit k of its byte q (numpy.packbits(..., bitorder="little")), unused
 * high bits of the last byte zero.  Unpacking writes 0/1 bytes.  The raster must be 8-byte aligned when
 * n_steps is a multiple of 8 (it then moves as 64-bit words). */
int lsm_raster_pack_bits(const uint8_t *raster, long n_rows, int n_steps, uint8_t *packed, void *stream);
int lsm_raster_unpack_bits(const uint8_t *packed, long n_rows, int n_steps, uint8_t *raster, void *stream);

/* ---- reservoir ------------------------------------------------------------------------- */

typedef struct lsm_reservoir lsm_reservoir;

/* Replaces SNN(simulation_params=...) (extract_lsm_features.py:188): uploads one reservoir's
 * wiring (built on the host per SPEC.md §2) to the current device.  All arrays are HOST memory.
 *   csc_ptr (N+1), csc_post (nnz, ascending within a column), csc_w (nnz): synapses grouped by
 *           PRESYNAPTIC neuron j;  leak (N);  in_tgt (n_channels, in_fanout) target neurons of
 *           each input channel;  out_idx (n_out) strictly ascending output neurons.
 * Limits: num_neurons <= 8192, n_channels <= 65535, n_out <= num_neurons, every in_tgt entry in [0, num_neurons).
 *   refractory     any value >= 0; stored as min(refractory, 65535), which is the same simulation for the at most 65535
 *                  steps of a run (a neuron that fires is held through the end of the clip either way) and fits the
 *                  16-bit countdown of the ring-row kernels
 *   burst_isi_max  any int (an interval counts as a burst when it is <= burst_isi_max: none does for a value <= 0)
 *   in_tgt         a channel may name a neuron more than once: every entry adds w_in.  Such a map is served from the
 *                  input-entry lists (no channel masks or bit planes), so it has no pair-block layout (set_kernel mode 5
 *                  is refused). */
int lsm_reservoir_create(lsm_reservoir **out, int num_neurons, int n_channels,
                         const int32_t *csc_ptr, const int32_t *csc_post, const float *csc_w,
                         const float *leak, const int32_t *in_tgt, int in_fanout, float w_in,
                         const int32_t *out_idx, int n_out, float theta, int refractory,
                         int burst_isi_max);
int lsm_reservoir_destroy(lsm_reservoir *h);

/* Kernel used by lsm_reservoir_run for this handle: 0 = choose (register accumulation over dense
 * presynaptic rows; over ring rows -- dense ring window + list of the synapses outside it -- for ring-like
 * reservoirs whose dense table exceeds the L2 caches), 1 = sparse CSC scatter through LDS, 2 = dense rows
 * (for a reservoir that mode 0 serves with ring rows the dense table is built by THIS call: it allocates and
 * synchronises, once),
 * 3 = ring rows (refused when the reservoir is not ring-like or has fewer than ~700 neurons), 4 = ring rows
 * restricted to the layouts with contiguous quad ownership (tests; 3 prefers the strided ones), 5 = ring rows in pair
 * blocks only (128-neuron blocks, two neurons per lane; refused when the reservoir has no pair-block layout: more than
 * 256 channels; 129 to 256 channels without bit positions in which the channels feeding one neuron differ mod 32 (e.g.
 * more than 32 channels onto one neuron); a channel that names a neuron twice; or no block count and window that fit 4, 8
 * or 16 waves), 6 = ring rows in quads only (never pair blocks).  Modes 0 and 3 take pair blocks where they were measured
 * faster: at least three blocks per wave and at most 128 channels; above 128 channels pair blocks run by name (5) only
 * (DESIGN.md 3c).  All produce bit-identical results (SPEC.md §3).  num_neurons <= 8192. */
int lsm_reservoir_set_kernel(lsm_reservoir *h, int mode);

/* The kernel lsm_reservoir_run would launch for this handle now: 1 sparse, 2 dense rows, 3 ring rows -- for the
 * reference's 400 time steps and waves_per_clip = 0; lsm_reservoir_plan answers for any launch. */
int lsm_reservoir_kernel_in_use(const lsm_reservoir *h);

/* Replaces, for a whole batch, the per-clip loop body of extract_all_features
 * (extract_lsm_features.py:78-87): reset -> set_input_spike_times -> simulate ->
 * extract_features_from_spikes -> nan_to_num -> concatenate in key order.
 *   spikes_u8   (n_clips, n_channels, n_steps) uint8, device (File-1 layout, create_dataset.py:168)
 *   key_ids     n_keys entries (HOST) from {0 spike_counts, 1 spike_variances, 2 mean_spike_times,
 *               3 first_spike_times, 4 last_spike_times, 5 mean_isi, 6 isi_variances,
 *               7 burst_counts} (FEATURE_SETS, extract_lsm_features.py:19-28)
 *   features_out     (n_clips, n_keys*n_out) float32, device
 *   spike_matrix_out (n_clips, n_steps, N) uint8 or NULL   (lsm.spike_matrix, :113-116)
 *   v_trace_out      (n_clips, n_steps, N) float32 or NULL (membrane potential after each step)
 *   stats_out        (n_clips, 2) int32 or NULL: per clip {neurons that fired at least once, spikes of the
 *                    whole reservoir} -- what run_network_diagnostics (:119-133) derives from lsm.spike_matrix
 *                    (participation, dead neurons, mean spikes per neuron), accumulated inside the kernel
 *   waves_per_clip   0 = choose for a lone launch of this batch size; -1 = choose for a launch that shares
 *                    the GPU with other kernels of an overlapped pipeline; else 1, 2, 4, 8 or 16
 * Fails (LSM_ERR, "no ... layout") when no layout's per-clip LDS image fits a CU's 160 KB: roughly
 * 10*N + 16*n_out + n_steps*ceil(n_channels/32)*4 bytes for ring rows (e.g. N = 8000 with more than ~4500 output
 * neurons); every BASELINE configuration fits (N = 8000, n_out = 3200, 256 channels: 145 KB).  n_steps <= 65535 (the
 * feature records hold spike counts and times in 16 bits); the LDS image grows by 4 * ceil(n_channels / 32) bytes per step,
 * so long clips of many channels are refused the same way well before that (lsm_reservoir_plan tells without launching). */
int lsm_reservoir_run(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                      const int32_t *key_ids, int n_keys, float *features_out,
                      uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                      int waves_per_clip, void *stream);

/* lsm_reservoir_run with the clips of the batch STARTED longest first.  A clip's time in the kernel grows with its
 * activity, which follows its input spike count (rank correlation 0.99 at N = 4000; clips of one batch differ ninefold);
 * a launch with more clips than the chip holds at once is otherwise as long as whichever clip starts last.  Two small
 * launches on the same stream count every clip's input spikes and rank them into `workspace` (caller-owned device memory,
 * lsm_reservoir_order_workspace(n_clips) bytes, private to this call until the stream has passed it); workgroup g of the
 * LIF kernel then takes the clip with the g-th most input spikes.  Every output is the one lsm_reservoir_run writes, at the
 * same place (row b belongs to clip b).  Batches of at most one clip per compute unit are launched as they are. */
long lsm_reservoir_order_workspace(int n_clips);
int lsm_reservoir_run_ordered(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                              const int32_t *key_ids, int n_keys, float *features_out,
                              uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                              int waves_per_clip, void *workspace, long workspace_bytes, void *stream);

/* Continuation (SPEC.md §4a): a launch that starts from a saved state and saves its own, so that a run split at any step
 * gives, bit for bit, what the unsplit run gives -- clips longer than one launch's LDS image holds, and streams taken
 * window by window.  lsm_reservoir_run and lsm_reservoir_run_ordered are untouched by it (an implicit reset() per launch).
 *
 * State: per clip one block of lsm_reservoir_state_bytes(h) bytes (a multiple of 16), clip b at byte b * that, DEVICE
 * memory owned by the caller, 16-byte aligned.  With NP = num_neurons rounded up to 64:
 *     uint32 header[4]          {spikes of the whole reservoir so far, 0, 0, 0}
 *     float  v[NP]              membrane potentials (entries past num_neurons: 0)
 *     uint16 ref[NP]            refractory countdowns
 *     uint32 last_spikes[NP/32] bit i: neuron i fired at the last step done
 *     uint32 ever_fired[NP/32]  bit i: neuron i fired at least once
 *     uint32 feat[n_out][4]     per output neuron {n | bursts << 16, first | last << 16, S1, Q} (SPEC.md §4, absolute times)
 * The layout does not depend on the kernel, the waves per clip or the layout a launch ran with: consecutive launches may
 * differ in all of them.  ALL ZEROS IS reset().
 *
 * lsm_reservoir_run_from runs steps [first_step, first_step + n_steps) of every clip:
 *   first_step   HOST value: the steps done before (what the state holds); the library never reads device memory to check it
 *   state_in     state after step first_step - 1, or NULL: reset (first_step must then be 0)
 *   state_out    receives the state after step first_step + n_steps - 1, or NULL; may equal state_in (each clip's block is
 *                read at the start and written at the end of the same workgroup)
 *   features_out features of steps [0, first_step + n_steps) -- spike times are absolute, spike_variances uses
 *                T = first_step + n_steps --, or NULL with n_keys = 0
 *   spike_matrix_out, v_trace_out   (n_clips, n_steps, N): this launch's steps only
 *   stats_out    totals of [0, first_step + n_steps)
 *   order_workspace   NULL: clips start in index order; else as lsm_reservoir_run_ordered's workspace
 * Everything else as lsm_reservoir_run, including the refusals of the plan for n_steps (lsm_reservoir_max_steps gives the
 * longest launch the plan accepts: chunks of at most that serve any clip).  LSM_ERR_ARG for first_step < 0,
 * first_step + n_steps > 65535, first_step > 0 without state_in, a state pointer that is not 16-byte aligned.  With both
 * states NULL it is lsm_reservoir_run. */
long lsm_reservoir_state_bytes(const lsm_reservoir *h);
int lsm_reservoir_run_from(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                           int first_step, const void *state_in, void *state_out,
                           const int32_t *key_ids, int n_keys, float *features_out,
                           uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                           int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream);

/* Segments and windows (SPEC.md §4b): lsm_reservoir_run_from with the feature bookkeeping cut every segment_steps steps.
 * Segment g of the launch covers its steps [g * segment_steps, (g + 1) * segment_steps); records_out receives, per clip,
 * segment and output neuron, the record of the state block's packing {n | bursts << 16, first | last << 16, S1, Q} over
 * the neuron's spikes inside that segment, on times local to the segment (0 .. segment_steps - 1):
 *   records_out  (n_clips, n_steps / segment_steps, n_out) x 16 bytes, DEVICE memory owned by the caller, 16-byte
 *                aligned, required
 * The dynamics are one uncut run: state_out, the cumulative features_out (absolute times; NULL with n_keys = 0),
 * stats_out, the spike matrix and the membrane trace are lsm_reservoir_run_from's, bit for bit.  Records of consecutive
 * launches cut at a segment boundary concatenate along the segment axis.  lsm_reservoir_plan and lsm_reservoir_max_steps
 * answer for a segmented launch as for an unsegmented one (the LDS image is the same).  LSM_ERR_ARG for
 * segment_steps < 1, n_steps % segment_steps != 0, a NULL or misaligned records_out, and lsm_reservoir_run_from's refusals.
 *
 * lsm_segment_features turns records into feature rows: window w of window_segments segments starts at segment
 * w * hop_segments, there are W = (n_segments - window_segments) / hop_segments + 1 of them, and a window's row is, bit for
 * bit, the feature row of the (window_segments * segment_steps, N) slice of the spike matrix it covers (§4a's merge folded
 * over its records, then §4's features with T = window_segments * segment_steps):
 *   records       (n_clips, n_segments, n_out) x 16 bytes as written above (launches concatenated along the segment axis)
 *   features_out  (n_clips, W, n_keys * n_out) float32, key-major rows
 * LSM_ERR_ARG for segment_steps < 1, window_segments < 1 or > n_segments, hop_segments < 1,
 * window_segments * segment_steps > 65535, n_keys outside [1, 8], a misaligned records pointer. */
int lsm_reservoir_run_segments(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                               int segment_steps, int first_step, const void *state_in, void *state_out, void *records_out,
                               const int32_t *key_ids, int n_keys, float *features_out,
                               uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                               int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream);
int lsm_segment_features(const lsm_reservoir *h, const void *records, int n_clips, int n_segments, int segment_steps,
                         int window_segments, int hop_segments, const int32_t *key_ids, int n_keys, float *features_out,
                         void *stream);

/* Ragged batches (SPEC.md §4c): lsm_reservoir_run_from whose clips run a number of steps of their own.  n_steps is the row
 * stride of the launch -- spikes_u8 is (n_clips, C, n_steps), the spike matrix and the membrane trace (n_clips, n_steps, N) --
 * and clip b runs L_b = clamp(clip_steps[b], 0, n_steps) steps: it is, bit for bit, lsm_reservoir_run_from over steps
 * [first_step, first_step + L_b) of that clip alone.
 *   clip_steps   (n_clips) int32, DEVICE memory, 4-byte aligned, or NULL: every clip runs n_steps (the call is then
 *                lsm_reservoir_run_from).  The kernels clamp every value into [0, n_steps], so no value can address outside
 *                the launch's buffers; the library never reads device memory to check one (as with first_step)
 *   first_step   HOST value, one for the whole launch
 *   features_out clip b: features of steps [0, first_step + L_b), spike_variances with T = first_step + L_b
 *   stats_out, state_out   clip b: after step first_step + L_b - 1
 *   spike_matrix_out, v_trace_out   clip b: rows 0 .. L_b - 1 are written, rows from L_b on are left as they are
 *   order_workspace   as lsm_reservoir_run_from's; the clips are ranked by their input spikes at t < L_b
 * Input bytes at t >= L_b influence nothing.  A clip with L_b = 0 is not touched: its feature row, statistics row and
 * matrix rows keep what they held, and its state_out block receives its state_in block byte for byte (zeros when state_in
 * is NULL; nothing happens when state_out == state_in).  A clip that ran fewer than n_steps steps has ended: later launches
 * of the same run must give it 0 steps (the library cannot check that; SNN.run_batch(lengths=...) does).
 * The plan and the LDS image are those of n_steps: lsm_reservoir_plan and lsm_reservoir_max_steps answer as for an unragged
 * launch, and every refusal of lsm_reservoir_run_from applies unchanged; LSM_ERR_ARG also for a clip_steps pointer that is
 * not 4-byte aligned.  Segments (§4b) are not offered on this entry. */
int lsm_reservoir_run_ragged(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                             const int32_t *clip_steps, int first_step, const void *state_in, void *state_out,
                             const int32_t *key_ids, int n_keys, float *features_out,
                             uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                             int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream);

/* Largest n_steps lsm_reservoir_plan accepts for (n_clips, waves_per_clip), at most 65535; < 0 when it accepts none. */
int lsm_reservoir_max_steps(const lsm_reservoir *h, int n_clips, int waves_per_clip);

/* Layout that lsm_reservoir_run would use: waves per clip, 64-neuron slots per lane, LDS bytes. */
int lsm_reservoir_layout(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip,
                         int *wpc_out, int *slots_out, int *lds_bytes_out);

/* The whole decision lsm_reservoir_run makes for (handle, batch, steps, waves_per_clip) -- run, layout and
 * kernel_in_use all go through it: kernel (1 sparse, 2 dense rows, 3 ring rows), waves per clip, slots per lane,
 * LDS bytes per clip, and the bytes of the weight table that kernel gathers its rows from (dense rows: N x ld x 4;
 * ring rows: windows + this layout's lists; sparse: the CSC arrays).  Any out pointer may be NULL.  In auto mode a
 * reservoir that prefers ring rows falls back to the dense (else sparse) kernel when no ring layout fits the LDS or
 * offers the requested waves per clip; an explicit ring request (modes 3, 4) fails instead. */
int lsm_reservoir_plan(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip, int *kernel_out,
                       int *wpc_out, int *slots_out, int *lds_bytes_out, long *table_bytes_out);

/* Bytes ONE reservoir spike makes the planned kernel request from its weight table, mean over the presynaptic
 * neurons (what bench.py's `roofline.row_gather` charges per spike; padding of the table is not charged): dense rows
 * ld x 4; ring rows the window's existing bytes (128-byte-aligned start .. window end, 16-byte granules) + 8 bytes per
 * list entry + the (waves + 1) row pointers; sparse 8 bytes per synapse + the two row pointers. */
int lsm_reservoir_row_request_bytes(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip,
                                    double *mean_bytes_out);

/* How the planned kernel forms the input drive (introspection for tests): dense rows 0 = input-map entries streamed
 * from global memory + LDS atomics, 1 = entries in registers + LDS atomics, 2 = per-neuron channel masks, four
 * popcounts, 3 = channel masks at coloured bit positions, one popcount (C <= 128 and an assignment exists in which
 * the channels feeding one neuron differ mod 32); ring rows 10 = packed entries streamed, 11 = entries in registers: in
 * quads the wave's packed input-map entries, in pair blocks (129 to 256 channels) one (bit position -> row word) entry per
 * coloured bit of a neuron, held as a position mask and three bit planes and resolved by bitwise selects,
 * 12 / 13 = per-neuron channel masks at natural / coloured positions (C <= 128, every neuron the same leak
 * coefficient, strided quad ownership with at most two quads per wave), 14 / 15 = the same masks in the pair-block form of the
 * ring rows (C <= 128; any leak coefficients); sparse kernel 20. */
int lsm_reservoir_input_mode(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip);

/* Which form of the ring rows the planned kernel is (the same decision as lsm_reservoir_plan): 0 = the planned kernel is
 * not ring rows, 1 = quads with contiguous ownership, 2 = quads with strided ownership, 3 = pair blocks; < 0 on error. */
int lsm_reservoir_ring_form(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip);

/* Host-only (no GPU, no HIP call): the ring-window table, the pair-block lists ({LDS byte offset of the target's accumulator,
 * weight bits} per entry) and the 16-byte row records lsm_reservoir_create would build for these CSC arrays and `wpc` (4, 8, 16)
 * waves per clip, with the two tables placed at the given (fictitious) addresses.  Call with null arrays for the sizes
 * (band_floats, n_list_entries, pitch_bytes), then with band_out[band_floats], rem_out[2 * n_list_entries],
 * rec_out[4 * num_neurons * wpc].  Returns the blocks per wave, 0 when the reservoir has no pair layout with that many waves,
 * < 0 on a bad argument.  tests/test_pair_layout.py applies every row from these tables alone, on the CPU. */
int lsm_debug_pair_layout(int num_neurons, const int32_t *csc_ptr, const int32_t *csc_post, const float *csc_w, int wpc,
                          unsigned long long band_addr, unsigned long long rem_addr, long *band_floats, long *n_list_entries,
                          int *pitch_bytes, float *band_out, uint32_t *rem_out, uint32_t *rec_out);

/* Host-only (no GPU, no HIP call): what lsm_reservoir_create would upload for the pair-block kernel's input drive with `wpc`
 * (4, 8, 16) waves per clip: perm_out[n_channels], the bit position of every channel in a step's input bit row (word * 32 +
 * colour; the channel's own number where the masks keep the natural positions), and words_out[4 * NPAD], NPAD = 256 *
 * ceil(num_neurons / 256), four words per neuron: up to 128 channels the channel masks (bit `position`), from 129 to 256
 * channels {posmask, P0, P1, P2} -- bit p of posmask: a channel at a position = p mod 32 feeds the neuron; bit p of Pj: bit j
 * of that channel's word.  Either array may be NULL.  Returns 1 (masks, natural positions), 2 (masks, coloured positions) or
 * 3 (bit planes); 0 when the map has no such form (more than 256 channels, no colouring above 128, a channel naming a neuron
 * twice) or the blocks do not share out over `wpc` waves; < 0 on a bad argument. */
int lsm_debug_pair_inputs(int num_neurons, int n_channels, const int32_t *in_tgt, int in_fanout, int wpc, uint8_t *perm_out,
                          uint32_t *words_out);

#ifdef __cplusplus
}
#endif
#endif /* LSM_HIP_H */
