// Streamed mel front end for gfx950 (SPEC.md §1.7, include/lsm_hip_mel_stream.h): centred STFT frames -> mel power -> dB ->
// fixed-range normalise -> hysteresis spike encoder, continued from a saved per-stream state.  A stream cut into launches at
// any hop boundaries gives, byte for byte, the raster of its one uncut run: STFT frames do not depend on each other, so all
// that travels in the state block is the tail of samples the next frames reach back into, the latches and a saturating hop
// count; the normalisation range is fixed for the stream's life, and there is one time bin per frame (no resize).
//
// Two kernels enqueued by one call, in stream order (chosen for simplicity over mel_spikes_kernel's "last workgroup to
// arrive finishes": no arrival counters to zero, no agent-scope fences, and the kernel boundary is what orders every read of
// the history before its in-place shift, DESIGN.md "The state block"):
//   1. mel_stream_frames_kernel   grid (H, n_streams), one wave per (new frame, stream): the frame transform of mel_body.h on
//                                 [history | new audio], power values to the workspace;
//   2. mel_stream_finish_kernel   one workgroup per stream: dB, normalise, latches over this push's frames in order, raster
//                                 bytes, history shift, hop count.
// Every float operation of a frame is mel_power_kernel's in its order (mel_body.h); compiled with -ffp-contract=off.
#include "lsm_common.h"
#include "mel_body.h"
#include "spikes_body.h"
#include "stream_state.h"
#include <cmath>

namespace {

using namespace lsm_mel;
using lsm_fe::MAX_THR;
using namespace lsm_state;

constexpr int HOP_MIN = NFFT / 16, HOP_MAX = NFFT / 2;
constexpr int FIN_THREADS = 256;
constexpr int FIN_TILE = 64;                 // filters and columns of a tile of the finish kernel
constexpr int HIST_PER_THREAD = NFFT / FIN_THREADS;     // the history is shorter than NFFT samples

// Lg = ceil((n_fft / 2) / hop): the hops a stream must hold before its frame 0 is complete
__host__ __device__ inline int latency_hops(int hop) { return (N2 + hop - 1) / hop; }
// Hs = (Lg - 1) * hop + n_fft / 2 samples of history: frame i of a launch is [i * hop, i * hop + n_fft) of [history | audio]
__host__ __device__ inline int history_samples(int hop) { return (latency_hops(hop) - 1) * hop + N2; }

// One stream's state block:
//   Hs x float32        the stream's last Hs samples (zeros before its start: the centre padding)
//   n_mels x uint32     latch bits (bit k: threshold k)
//   uint32              hops seen, saturating at Lg - 1
// rounded up to a multiple of 16 bytes.  All zeros: the start of a stream.
__host__ __device__ inline size_t state_used_bytes(int n_mels, int hop)
{
    return ((size_t)history_samples(hop) + (size_t)n_mels + 1) * 4;
}
__host__ __device__ inline size_t state_block_bytes(int n_mels, int hop)
{
    return state_round16(state_used_bytes(n_mels, hop));
}

struct MelStreamArgs {
    const float *audio;                 // (n_streams, H * hop)
    Tables tab;
    const int32_t *stream_hops;         // (n_streams) or null
    const unsigned char *state_in;      // or null
    unsigned char *state_out;           // or null; may be state_in
    uint8_t *raster;                    // (n_streams, F * R, H * n_thr)
    float *power_ws;                    // (n_streams, F, H): the frames kernel's values for the finish kernel
    float *power_out, *db_out;          // (n_streams, F, H) or null
    int n_streams, n_hops, hop, n_thr, redundancy;
    float db_lo, db_hi;                 // rounded to float32 once, by the launch function
    float on[MAX_THR], off[MAX_THR];    // entries from n_thr on never fire (+inf / -inf)
};

// What a stream does in this launch (wave-uniform): h_b hops, of which the first `skip` complete frames that would lie before
// the stream's start; the others complete the frames that become columns 0 .. cols - 1.
struct StreamPlan {
    int hb, cnt, skip, cols;
};
__device__ __forceinline__ StreamPlan stream_plan(const MelStreamArgs &a, const int b)
{
    const int H = a.n_hops, Lg = latency_hops(a.hop);
    StreamPlan p;
    p.hb = stream_count(a.stream_hops, b, H);
    p.cnt = 0;
    if (a.state_in) {
        const uint32_t *su = reinterpret_cast<const uint32_t *>(a.state_in + (size_t)b * state_block_bytes(a.tab.n_mels, a.hop));
        p.cnt = (int)min(su[history_samples(a.hop) + a.tab.n_mels], (uint32_t)(Lg - 1));
    }
    p.skip = Lg - 1 - p.cnt;
    p.cols = max(p.hb - p.skip, 0);
    return p;
}

// grid = (H, n_streams), one wave each: column c of stream b, the frame its new hop skip + c completes
__global__ __launch_bounds__(64) void mel_stream_frames_kernel(const MelStreamArgs a)
{
    __shared__ double2 z[ZPAD];                 // 17 KB
    const int b = blockIdx.y, c = blockIdx.x;
    const StreamPlan p = stream_plan(a, b);
    if (c >= p.cols) return;                    // wave-uniform
    const int H = a.n_hops, hop = a.hop, F = a.tab.n_mels, Hs = history_samples(hop);
    const int base = (p.skip + c) * hop;        // the frame's first sample in [history | audio]: base + 2047 < Hs + h_b * hop
    const float *__restrict__ row = a.audio + (size_t)b * H * hop;
    // without a state block the history is zeros: the loads then go to the row's first sample and their values are dropped
    const bool have_hist = a.state_in != nullptr;
    const float *__restrict__ hist = have_hist
        ? reinterpret_cast<const float *>(a.state_in + (size_t)b * state_block_bytes(F, hop)) : row;
    const int hist_last = have_hist ? Hs - 1 : 0;
    float *__restrict__ ws = a.power_ws, *__restrict__ power_out = a.power_out;
    mel_frame_wave(a.tab, z,
        [&](const int q, double &v0, double &v1) {
            // both sources are read at clamped indices and one value is kept (mel.hip: no guarded loads)
            const int s0 = base + q, s1 = s0 + 1;
            const float h0 = hist[min(s0, hist_last)], h1 = hist[min(s1, hist_last)];
            const float x0 = row[max(s0 - Hs, 0)], x1 = row[max(s1 - Hs, 0)];
            v0 = s0 >= Hs ? (double)x0 : (have_hist ? (double)h0 : 0.0);
            v1 = s1 >= Hs ? (double)x1 : (have_hist ? (double)h1 : 0.0);
        },
        [&](const int m, const float acc) {
            const size_t o = ((size_t)b * F + m) * H + c;
            ws[o] = acc;
            if (power_out) power_out[o] = acc;
        });
}

// grid = n_streams, one workgroup each: dB, normalise, latches, raster of the stream's new columns; then its state block.
__global__ __launch_bounds__(FIN_THREADS) void mel_stream_finish_kernel(const MelStreamArgs a)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const StreamPlan p = stream_plan(a, b);
    const int H = a.n_hops, hop = a.hop, F = a.tab.n_mels, Hs = history_samples(hop), Lg = latency_hops(hop);
    const size_t block = state_block_bytes(F, hop);
    const StateBlock blk = state_block(a.state_in, a.state_out, b, block);
    const unsigned char *sin = blk.sin;
    unsigned char *sout = blk.sout;
    if (p.hb == 0) {
        carry_idle_block<FIN_THREADS>(blk, block, tid);
        return;
    }
    // the new history: the last Hs samples of [history | this push's h_b * hop samples], read into registers by every
    // thread BEFORE any of them is stored (state_out may be state_in, and a short push shifts within the block); the
    // latch loop lies between, so this is not stream_state.h's chunked shift
    const float *hist = reinterpret_cast<const float *>(sin);
    const float *__restrict__ row = a.audio + (size_t)b * H * hop;
    const int adv = p.hb * hop;                 // <= H * hop <= 2^31 - 1
    float keep[HIST_PER_THREAD];
#pragma unroll
    for (int k = 0; k < HIST_PER_THREAD; ++k) {
        const int j = tid + FIN_THREADS * k;
        keep[k] = 0.0f;
        if (j < Hs) {
            // j + adv as a sum of two ints below 2^31 each: compared without forming it
            if (j >= Hs - adv) keep[k] = row[adv - (Hs - j)];
            else if (hist) keep[k] = hist[j + adv];
        }
    }

    const float lo = a.db_lo, hi = a.db_hi;
    const float fl = hi - 80.0f;
    const float den = (hi - lo) + 1e-8f;
    const int n_thr = a.n_thr, R = a.redundancy;
    const uint32_t tmask = (1u << n_thr) - 1u;
    const size_t row_bytes = (size_t)H * n_thr;
    const uint32_t *latch_in = sin ? reinterpret_cast<const uint32_t *>(sin) + Hs : nullptr;
    uint32_t *latch_out = sout ? reinterpret_cast<uint32_t *>(sout) + Hs : nullptr;
    // Tiles of FIN_TILE filters x FIN_TILE columns.  1. every thread takes elements of the tile, a lane a column (the loads
    // along a row): dB value, normalised value, and per threshold "above on" / "below off" as two bytes of bits in LDS;
    // 2. thread m of the first wave runs filter m's latches over the tile's columns in order and stores the raster bytes.
    __shared__ uint8_t upb[FIN_TILE][FIN_TILE + 4], dnb[FIN_TILE][FIN_TILE + 4];
    const int col = tid & (FIN_TILE - 1), sub = tid / FIN_TILE;
    for (int r0 = 0; r0 < F; r0 += FIN_TILE) {
        const int m = r0 + tid;                 // the filter of a latch thread
        const bool latch_thread = tid < FIN_TILE && m < F;
        uint32_t act = (latch_thread && latch_in) ? latch_in[m] : 0u;
        for (int c0 = 0; c0 < p.cols; c0 += FIN_TILE) {
            const int c = c0 + col;
            for (int rl = sub; rl < FIN_TILE; rl += FIN_THREADS / FIN_TILE) {
                if (r0 + rl >= F || c >= p.cols) continue;
                const size_t o = ((size_t)b * F + r0 + rl) * H + c;
                const float S = a.power_ws[o];
                // np.maximum propagates a NaN, fmaxf drops it
                const float v = 10.0f * log10f(S != S ? S : fmaxf(1e-10f, S));
                // a NaN stays a NaN through the floor and compares false with every threshold: the latches keep their state
                const float val = lsm_fe::floored_value(v, fl, lo, den);
                uint32_t up = 0u, dn = 0u;
#pragma unroll
                for (int t = 0; t < MAX_THR; ++t) {
                    up |= (val > a.on[t] ? 1u : 0u) << t;
                    dn |= (val < a.off[t] ? 1u : 0u) << t;
                }
                upb[rl][col] = (uint8_t)up;
                dnb[rl][col] = (uint8_t)dn;
                if (a.db_out) a.db_out[o] = v;
            }
            __syncthreads();
            if (latch_thread) {
                uint8_t *rrow = a.raster + ((size_t)b * F + m) * R * row_bytes;       // this filter's first raster row
                const int nc = min(FIN_TILE, p.cols - c0);
                for (int j = 0; j < nc; ++j) {
                    const uint32_t up = upb[tid][j], dn = dnb[tid][j];
                    act = lsm_fe::latch_step(act, up, dn, tmask);
                    lsm_fe::store_column(rrow, row_bytes, c0 + j, n_thr, R, act);
                }
            }
            __syncthreads();                    // the tile's bits are free for the next one
        }
        if (latch_thread && latch_out) latch_out[m] = act;
    }
    __syncthreads();                            // every thread has read its share of the old history
    if (sout) {
        float *hout = reinterpret_cast<float *>(sout);
#pragma unroll
        for (int k = 0; k < HIST_PER_THREAD; ++k) {
            const int j = tid + FIN_THREADS * k;
            if (j < Hs) hout[j] = keep[k];
        }
        if (tid == 0) reinterpret_cast<uint32_t *>(sout)[Hs + F] = (uint32_t)min(p.cnt + p.hb, Lg - 1);
        carry_padding<uint32_t>(blk, state_used_bytes(F, hop) / 4, block, tid);
    }
}

bool shape_ok(int n_mels, int n_fft, int hop) { return n_mels >= 1 && n_fft == NFFT && hop >= HOP_MIN && hop <= HOP_MAX; }

}  // namespace

LSM_API long lsm_mel_stream_state_bytes(int n_mels, int n_fft, int hop)
{
    if (!shape_ok(n_mels, n_fft, hop)) return 0;
    return (long)state_block_bytes(n_mels, hop);
}

LSM_API long lsm_mel_stream_workspace(int n_streams, int n_mels, int n_hops)
{
    if (n_streams < 0 || n_mels < 1 || n_hops < 1) return 0;
    // the power values of the launch's frames, float32 (n_streams, n_mels, n_hops)
    return (long)(((size_t)n_streams * n_mels * n_hops * sizeof(float) + 255) / 256 * 256);
}

LSM_API int lsm_mel_stream_f32(const float *audio, int n_streams, int n_hops, int n_fft, int hop, const double *window_dev,
                               const double *twiddle_dev, const float *basis_dev, const int32_t *lo_dev,
                               const int32_t *hi_dev, int n_mels, const int32_t *stream_hops, double db_lo, double db_hi,
                               const float *thr_on, const float *thr_off, int n_thr, int redundancy, const void *state_in,
                               void *state_out, uint8_t *raster_out, float *power_out, float *db_out, void *workspace,
                               long workspace_bytes, void *stream)
{
    LSM_REQUIRE(n_fft == NFFT, "n_fft must be %d (librosa's default), got %d", NFFT, n_fft);
    LSM_REQUIRE(hop >= HOP_MIN && hop <= HOP_MAX, "hop=%d outside [%d, %d] (n_fft / 16 .. n_fft / 2)", hop, HOP_MIN, HOP_MAX);
    LSM_REQUIRE(n_mels >= 1, "n_mels=%d must be >= 1", n_mels);
    LSM_REQUIRE(n_streams >= 0 && n_streams <= 65535, "n_streams=%d outside [0, 65535] (grid.y)", n_streams);
    LSM_REQUIRE(n_hops >= 1, "n_hops=%d: a launch's row stride H must be >= 1", n_hops);
    LSM_REQUIRE((long)n_hops * hop <= 0x7fffffffL, "n_hops * hop exceeds 2^31 - 1 samples per row");
    LSM_REQUIRE(std::isfinite(db_lo) && std::isfinite(db_hi), "db_lo and db_hi (the calibration range) must be finite");
    LSM_REQUIRE(db_lo < db_hi, "the calibration range needs db_lo < db_hi, got [%g, %g]", db_lo, db_hi);
    const float lo32 = (float)db_lo, hi32 = (float)db_hi;
    LSM_REQUIRE(std::isfinite(lo32) && std::isfinite(hi32) && lo32 < hi32,
                "the calibration range needs db_lo < db_hi as float32 values, got [%g, %g]", db_lo, db_hi);
    LSM_REQUIRE(n_thr >= 1 && n_thr <= MAX_THR, "n_thr=%d outside [1, %d]", n_thr, MAX_THR);
    LSM_REQUIRE(redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(thr_on && thr_off, "null threshold table");
    LSM_REQUIRE(raster_out != nullptr, "raster_out is required");
    LSM_REQUIRE_ALIGNED(raster_out, 4);
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE((((uintptr_t)window_dev | (uintptr_t)twiddle_dev) & 15u) == 0,
                "the window and twiddle tables are misaligned: they must be 16-byte aligned");
    LSM_REQUIRE((((uintptr_t)basis_dev | (uintptr_t)lo_dev | (uintptr_t)hi_dev) & 3u) == 0,
                "the basis, lo and hi tables are misaligned: they must be 4-byte aligned");
    LSM_REQUIRE_ALIGNED(stream_hops, 4);
    LSM_REQUIRE_ALIGNED(state_in, 16);
    LSM_REQUIRE_ALIGNED(state_out, 16);
    LSM_REQUIRE_ALIGNED(power_out, 4);
    LSM_REQUIRE_ALIGNED(db_out, 4);
    LSM_REQUIRE_ALIGNED(workspace, 16);
    const long need = lsm_mel_stream_workspace(n_streams, n_mels, n_hops);
    LSM_REQUIRE(workspace_bytes >= need, "workspace of %ld bytes, need %ld (lsm_mel_stream_workspace)", workspace_bytes, need);
    if (n_streams == 0) return LSM_OK;
    LSM_REQUIRE(audio && window_dev && twiddle_dev && basis_dev && lo_dev && hi_dev && workspace, "mel_stream: null buffer");
    MelStreamArgs a;
    a.audio = audio;
    a.tab.window = window_dev; a.tab.twiddle = reinterpret_cast<const double2 *>(twiddle_dev); a.tab.basis = basis_dev;
    a.tab.lo = lo_dev; a.tab.hi = hi_dev; a.tab.n_mels = n_mels;
    a.stream_hops = stream_hops;
    a.state_in = static_cast<const unsigned char *>(state_in);
    a.state_out = static_cast<unsigned char *>(state_out);
    a.raster = raster_out; a.power_ws = static_cast<float *>(workspace); a.power_out = power_out; a.db_out = db_out;
    a.n_streams = n_streams; a.n_hops = n_hops; a.hop = hop; a.n_thr = n_thr; a.redundancy = redundancy;
    a.db_lo = lo32; a.db_hi = hi32;
    lsm_fe::fill_thresholds<float>(a.on, a.off, thr_on, thr_off, n_thr);
    hipLaunchKernelGGL(mel_stream_frames_kernel, dim3(n_hops, n_streams), dim3(64), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(mel_stream_finish_kernel, dim3(n_streams), dim3(FIN_THREADS), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
