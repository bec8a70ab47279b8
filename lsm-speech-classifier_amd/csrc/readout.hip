// Readout scores for gfx950 (SPEC.md §6, include/lsm_hip_readout.h): scaler and linear readout over feature rows that exist
// (lsm_readout_rows_f32) and over the sliding windows of segment records (lsm_readout_windows), whose rows are never written.
//
// Layout.  One workgroup of four to eight wave64 per row, in two phases per chunk of 512 output neurons (one chunk for
// every reservoir up to 512 output neurons).
//   scale   All threads share out the chunk's neurons: in the window launch a thread folds its neuron's K records once
//           (lsm_lif::merge_feature_records, 16-byte loads that are contiguous over the threads) and forms its n_keys features
//           (lsm_lif::feature_value); in the row launch it loads them, again contiguous.  It scales them and leaves the
//           float64 z in LDS, key-major like the row: n_keys * 512 * 8 bytes at most (32 KB).  The fold, the features'
//           and the scaler's divisions -- the expensive part -- are done once per row, by all the waves together.
//   score   Wave w owns the classes w * CT .. w * CT + CT - 1 (CT a template parameter; waves behind the last class idle
//           here).  §6 gives lane l the neurons o = l, l + 64, ... and within a neuron the keys in ascending order: the lane
//           reads z from LDS (consecutive lanes, consecutive banks), the CT coefficients from global memory (contiguous over
//           the lanes, the model stays in L2) and adds into CT lane sums held in registers (the loop over them unrolled: no
//           indexed register array, no scratch).  A chunk starts at a multiple of 64, so the lane sums run on in §6's order
//           from chunk to chunk.
// The tree is six shuffles per class; lane 0 of a wave adds the intercept, stores its logits and leaves them in 512 bytes of
// LDS, from which thread 0 reads the label after a barrier.  Nothing but the logits and the label is ever stored.  Every
// index is formed from clamped counts: a window is scored only when wdw * H + K <= clamp(clip_segments[b], 0, G), so no
// record behind a clip's G is read; the test is uniform over the workgroup, which returns as a whole before any barrier.
#include "lif_common.h"
#include "reservoir_facts.h"
#include <algorithm>

namespace {

struct ReadoutArgs {
    const double *mean, *scale, *coef, *intercept;      // (D), (D), (C, D), (C)
    double *logits;                                     // (rows, C) or null
    int32_t *labels;                                    // (rows) or null
    int n_out, n_keys, C, D;
    const float *features;                              // rows launch: (rows, D)
    const uint4 *rec;                                   // window launch: (B, G, n_out)
    const int32_t *valid;                               // (B) or null: G everywhere
    int G, S, K, H, W, burst_isi_max;
    int key_ids[8];
};

constexpr int MAX_CLASSES = 64, MIN_WAVES = 4, MAX_WAVES = 8, CHUNK = 512;

template <int CT, bool WINDOWS>
__global__ __launch_bounds__(LSM_WAVE * MAX_WAVES) void readout_kernel(const ReadoutArgs a)
{
    extern __shared__ double s_z[];                                  // (n_keys, pitch) scaled features of the chunk
    __shared__ double s_logit[MAX_CLASSES];
    const int tid = threadIdx.x, n_threads = blockDim.x;
    const int lane = tid & (LSM_WAVE - 1);
    const int c0 = (tid / LSM_WAVE) * CT;                            // this wave's classes: c0 .. c0 + CT - 1, below C
    const size_t row = blockIdx.x;
    const uint4 *rec = nullptr;
    const float *x = nullptr;
    if (WINDOWS) {
        const int b = (int)(row / (size_t)a.W), wdw = (int)(row % (size_t)a.W);
        const int gv = a.valid ? min(max(a.valid[b], 0), a.G) : a.G;
        if ((long)wdw * a.H + a.K > gv) return;                      // not a whole window of this clip: nothing is stored
        rec = a.rec + ((size_t)b * a.G + (size_t)wdw * a.H) * a.n_out;
    } else {
        x = a.features + row * (size_t)a.D;
    }
    const int pitch = min(a.n_out, CHUNK);
    double p[CT];
#pragma unroll
    for (int i = 0; i < CT; ++i) p[i] = 0.0;
    for (int o_lo = 0; o_lo < a.n_out; o_lo += CHUNK) {              // uniform: every thread meets every barrier
        const int o_hi = min(o_lo + CHUNK, a.n_out);
        if (o_lo) __syncthreads();                                   // the chunk before has been read
        // ---- scale ---------------------------------------------------------------------------------------------------
        for (int o = o_lo + tid; o < o_hi; o += n_threads) {
            uint4 f = make_uint4(0, 0, 0, 0);
            if (WINDOWS)
                for (int j = 0; j < a.K; ++j)
                    f = lsm_lif::merge_feature_records(f, rec[(size_t)j * a.n_out + o], (uint32_t)(j * a.S), a.burst_isi_max);
            const int n = (int)(f.x & 0xFFFFu), bursts = (int)(f.x >> 16);
            const int first = (int)(f.y & 0xFFFFu), last = (int)(f.y >> 16);
            for (int k = 0; k < a.n_keys; ++k) {
                const size_t d = (size_t)k * a.n_out + o;
                const float xv = WINDOWS ? lsm_lif::feature_value(a.key_ids[k], n, bursts, first, last, f.z, f.w, a.K * a.S)
                                         : x[d];
                s_z[k * pitch + (o - o_lo)] = ((double)xv - a.mean[d]) / a.scale[d];
            }
        }
        __syncthreads();
        // ---- score ---------------------------------------------------------------------------------------------------
        if (c0 < a.C) {
            for (int o = o_lo + lane; o < o_hi; o += LSM_WAVE) {
                for (int k = 0; k < a.n_keys; ++k) {
                    const size_t d = (size_t)k * a.n_out + o;
                    const double z = s_z[k * pitch + (o - o_lo)];
#pragma unroll
                    for (int i = 0; i < CT; ++i) {
                        const int c = min(c0 + i, a.C - 1);          // a class behind the last: computed again, never used
                        p[i] = p[i] + z * a.coef[(size_t)c * a.D + d];
                    }
                }
            }
        }
    }
    if (c0 < a.C) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (int i = 0; i < CT; ++i) p[i] = p[i] + __shfl_down(p[i], s, LSM_WAVE);   // lanes >= s hold values nobody reads
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < CT; ++i) {
                const int c = c0 + i;
                if (c < a.C) {
                    const double logit = a.intercept[c] + p[i];
                    if (a.logits) a.logits[row * (size_t)a.C + c] = logit;
                    s_logit[c] = logit;
                }
            }
        }
    }
    if (!a.labels) return;                                           // uniform
    __syncthreads();
    if (tid == 0) {
        double best = s_logit[0];
        int best_c = 0;
        bool any_nan = best != best;
        for (int c = 1; c < a.C; ++c) {
            const double logit = s_logit[c];
            any_nan |= logit != logit;
            if (logit > best) {
                best = logit;
                best_c = c;
            }
        }
        a.labels[row] = any_nan ? -1 : best_c;
    }
}

// The class tile of a launch: tiles of 4 classes up to 32 classes, of 8 above, one wave each; at least four waves (for the
// scale phase), at most eight.  Dynamic LDS: the chunk's scaled features.
template <bool WINDOWS>
void launch(const ReadoutArgs &a, size_t rows, hipStream_t stream)
{
    const int tile = a.C <= 2 ? a.C : a.C <= 32 ? 4 : 8;
    void (*fn)(const ReadoutArgs) = tile == 1 ? readout_kernel<1, WINDOWS> : tile == 2 ? readout_kernel<2, WINDOWS>
                                    : tile == 4 ? readout_kernel<4, WINDOWS> : readout_kernel<8, WINDOWS>;
    const int waves = std::max(MIN_WAVES, (a.C + tile - 1) / tile);
    const size_t lds = sizeof(double) * (size_t)a.n_keys * (size_t)std::min(a.n_out, CHUNK);
    hipLaunchKernelGGL(fn, dim3((unsigned)rows), dim3((unsigned)(LSM_WAVE * waves)), lds, stream, a);
}

bool aligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

LSM_API int lsm_readout_supported(int n_keys, int n_out, int n_classes)
{
    return n_keys >= 1 && n_keys <= 8 && n_out >= 1 && n_out <= 8192 && n_classes >= 1 && n_classes <= 64 ? 1 : 0;
}

LSM_API int lsm_readout_rows_f32(const double *mean, const double *scale, const double *coef, const double *intercept,
                                 const float *features, int n_rows, int n_keys, int n_out, int n_classes, double *logits_out,
                                 int32_t *labels_out, void *stream)
{
    LSM_REQUIRE(n_rows >= 0, "n_rows=%d must be >= 0", n_rows);
    LSM_REQUIRE(n_keys >= 1 && n_keys <= 8, "n_keys=%d must be in [1, 8]", n_keys);
    LSM_REQUIRE(n_out >= 1 && n_out <= 8192, "n_out=%d must be in [1, 8192]", n_out);
    LSM_REQUIRE(n_classes >= 1 && n_classes <= 64, "n_classes=%d must be in [1, 64]", n_classes);
    LSM_REQUIRE(mean && scale && coef && intercept, "readout: mean, scale, coef and intercept are required");
    LSM_REQUIRE(logits_out || labels_out, "readout: logits_out and labels_out are both NULL");
    LSM_REQUIRE(aligned(mean, 8) && aligned(scale, 8) && aligned(coef, 8) && aligned(intercept, 8) && aligned(logits_out, 8),
                "mean, scale, coef, intercept and logits_out must be 8-byte aligned");
    LSM_REQUIRE(aligned(features, 4) && aligned(labels_out, 4), "features and labels_out must be 4-byte aligned");
    if (n_rows == 0) return LSM_OK;
    LSM_REQUIRE(features, "readout: null features");
    ReadoutArgs a{};
    a.mean = mean; a.scale = scale; a.coef = coef; a.intercept = intercept; a.logits = logits_out; a.labels = labels_out;
    a.n_out = n_out; a.n_keys = n_keys; a.C = n_classes; a.D = n_keys * n_out; a.features = features;
    launch<false>(a, (size_t)n_rows, (hipStream_t)stream);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_readout_windows(const lsm_reservoir *h, const double *mean, const double *scale, const double *coef,
                                const double *intercept, const void *records, int n_clips, int n_segments,
                                const int32_t *clip_segments, int segment_steps, int window_segments, int hop_segments,
                                const int32_t *key_ids, int n_keys, int n_classes, double *logits_out, int32_t *labels_out,
                                void *stream)
{
    LSM_REQUIRE(h != nullptr, "lsm_readout_windows: null handle");
    LSM_REQUIRE(n_clips >= 0 && n_segments >= 1, "bad n_clips/n_segments");
    LSM_REQUIRE(segment_steps >= 1, "segment_steps=%d must be >= 1", segment_steps);
    LSM_REQUIRE(window_segments >= 1 && window_segments <= n_segments, "window_segments=%d must be in [1, n_segments=%d]",
                window_segments, n_segments);
    LSM_REQUIRE(hop_segments >= 1, "hop_segments=%d must be >= 1", hop_segments);
    LSM_REQUIRE((long)window_segments * segment_steps <= 65535, "a window of %d segments of %d steps exceeds 65535 steps "
                "(the feature records hold spike times in 16 bits)", window_segments, segment_steps);
    LSM_REQUIRE(n_keys >= 1 && n_keys <= 8 && key_ids, "n_keys must be in [1, 8]");
    for (int k = 0; k < n_keys; ++k)
        LSM_REQUIRE(key_ids[k] >= 0 && key_ids[k] < 8, "key id %d out of range", key_ids[k]);
    LSM_REQUIRE(n_classes >= 1 && n_classes <= 64, "n_classes=%d must be in [1, 64]", n_classes);
    LSM_REQUIRE(mean && scale && coef && intercept, "readout: mean, scale, coef and intercept are required");
    LSM_REQUIRE(logits_out || labels_out, "readout: logits_out and labels_out are both NULL");
    LSM_REQUIRE(aligned(records, 16), "records must be 16-byte aligned");
    LSM_REQUIRE(aligned(mean, 8) && aligned(scale, 8) && aligned(coef, 8) && aligned(intercept, 8) && aligned(logits_out, 8),
                "mean, scale, coef, intercept and logits_out must be 8-byte aligned");
    LSM_REQUIRE(aligned(clip_segments, 4) && aligned(labels_out, 4), "clip_segments and labels_out must be 4-byte aligned");
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(records, "readout: null records");
    const ReservoirRecordFacts facts = reservoir_record_facts(h);
    int dev_now = -1;
    LSM_CHECK_HIP(hipGetDevice(&dev_now));
    LSM_REQUIRE(dev_now == facts.device, "reservoir handle lives on device %d but the current device is %d", facts.device,
                dev_now);
    ReadoutArgs a{};
    a.mean = mean; a.scale = scale; a.coef = coef; a.intercept = intercept; a.logits = logits_out; a.labels = labels_out;
    a.n_out = facts.n_out; a.n_keys = n_keys; a.C = n_classes; a.D = n_keys * facts.n_out;
    a.rec = static_cast<const uint4 *>(records); a.valid = clip_segments;
    a.G = n_segments; a.S = segment_steps; a.K = window_segments; a.H = hop_segments;
    a.W = (n_segments - window_segments) / hop_segments + 1;
    a.burst_isi_max = facts.burst_isi_max;
    for (int k = 0; k < 8; ++k) a.key_ids[k] = k < n_keys ? key_ids[k] : 0;
    const long rows = (long)n_clips * a.W;
    LSM_REQUIRE(rows <= 0x7FFFFFFFL, "too many (clip, window) pairs: %ld", rows);
    launch<true>(a, (size_t)rows, (hipStream_t)stream);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
