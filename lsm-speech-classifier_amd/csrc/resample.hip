// Polyphase FIR resampler for gfx950 (SPEC.md §1.8, include/lsm_hip_resample.h): float32 or int16 mono PCM at the device's
// rate in, float32 at the front end's rate out.  Two forms over one tap loop (resample_body.h):
//   batch     resample_kernel          grid (tiles, n_clips): y[m] = z[m + delay], scipy's centred alignment, zeros outside a clip;
//   streamed  resample_stream_kernel   grid (tiles, n_streams): z itself on [history | new blocks], then
//             resample_state_kernel    one workgroup per stream: the last Hs samples become the new history.
// The kernel boundary orders every read of the old history before its in-place shift (DESIGN.md "The state block").
//
// Layout.  A workgroup of 512 threads makes a tile of 2048 consecutive outputs of one row, thread t the outputs
// t, t + 512, ...: neighbouring lanes read inputs down/up samples apart (2.76 at 44.1 kHz), a wave some 700 contiguous bytes per
// tap, which is left to L1 -- a staged input tile would be read 21 to 127 times per sample as well, from LDS banks the taps
// already keep busy.  The tap table is staged in LDS [phase][tap] with an odd row stride (resample_body.h): 160 rows of 58 at
// 44.1 kHz (74 KB), 640 of 21 at 11.025 kHz (105 KB), one row at 48 kHz; loading it costs 8 * K bytes from L2 per 2048
// outputs, under 3 % of what the tap loop reads.  A table over 160 KB is refused (LSM_ERR_UNSUPPORTED).
#include "resample_body.h"
#include "stream_state.h"
#include <numeric>

namespace {

using namespace lsm_resample;
using namespace lsm_state;

struct ResampleArgs {
    const void *audio;                  // batch (n_clips, n_in); streamed (n_streams, G * down); float32 or int16
    const double *taps;                 // hp, n_taps doubles
    float *out;                         // batch (n_clips, n_out); streamed (n_streams, G * up)
    const int32_t *stream_blocks;       // (n_streams) or null
    const unsigned char *state_in;      // or null
    unsigned char *state_out;           // or null; may be state_in
    int fmt, n_taps, up, down;
    int n_in, n_out, delay;             // batch
    int n_blocks;                       // streamed: G
};

__host__ __device__ inline size_t state_block_bytes(int n_taps, int up)
{
    const size_t used = (size_t)history_samples(n_taps, up) * 4;
    return used ? state_round16(used) : 16;
}

__global__ __launch_bounds__(THREADS) void resample_kernel(const ResampleArgs a)
{
    extern __shared__ double tab[];
    load_table(tab, a.taps, a.n_taps, a.up);
    const int b = blockIdx.y, fmt = a.fmt, n_in = a.n_in;
    const size_t row = (size_t)b * n_in;
    const void *__restrict__ audio = a.audio;
    float *__restrict__ out = a.out + (size_t)b * a.n_out;
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const long long m = (long long)blockIdx.x * TILE + q * THREADS + threadIdx.x;
        if (m >= a.n_out) continue;
        const long long p = (m + a.delay) * a.down;
        out[m] = causal_sample(tab, a.n_taps, a.up, p / a.up, (int)(p % a.up), [&](const long long i) {
            // read at a clamped index and keep or drop the value (mel.hip: no guarded loads)
            const float v = pcm_f32(audio, row + (size_t)min(max(i, 0LL), (long long)n_in - 1), fmt);
            return (i >= 0 && i < n_in) ? (double)v : 0.0;
        });
    }
}

__global__ __launch_bounds__(THREADS) void resample_stream_kernel(const ResampleArgs a)
{
    extern __shared__ double tab[];
    const int b = blockIdx.y, fmt = a.fmt;
    const long long n = (long long)stream_count(a.stream_blocks, b, a.n_blocks) * a.up;               // outputs of this stream: <= G * up < 2^31
    if ((long long)blockIdx.x * TILE >= n) return;                              // workgroup-uniform
    load_table(tab, a.taps, a.n_taps, a.up);
    const int Hs = history_samples(a.n_taps, a.up);
    const long long row_len = (long long)a.n_blocks * a.down;
    const size_t row = (size_t)b * row_len;
    const void *__restrict__ audio = a.audio;
    // without a state block the history is zeros and nothing is loaded for it
    const bool have_hist = a.state_in != nullptr && Hs > 0;
    const float *__restrict__ hist = have_hist
        ? reinterpret_cast<const float *>(a.state_in + (size_t)b * state_block_bytes(a.n_taps, a.up)) : nullptr;
    float *__restrict__ out = a.out + (size_t)b * a.n_blocks * a.up;
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const long long m = (long long)blockIdx.x * TILE + q * THREADS + threadIdx.x;
        if (m >= n) continue;
        const long long p = m * a.down;
        out[m] = causal_sample(tab, a.n_taps, a.up, p / a.up, (int)(p % a.up), [&](const long long i) {
            // i < k_b * down always; i >= -Hs by the length of the longest row.  Both sources at clamped indices.
            const float x = pcm_f32(audio, row + (size_t)min(max(i, 0LL), row_len - 1), fmt);
            const float h = have_hist ? hist[min(max(i + Hs, 0LL), (long long)Hs - 1)] : 0.0f;
            return (double)(i >= 0 ? x : h);
        });
    }
}

// grid = n_streams, one workgroup each: the last Hs samples of [history | this push's k_b * down samples] as float32
__global__ __launch_bounds__(THREADS) void resample_state_kernel(const ResampleArgs a)
{
    const int b = blockIdx.x, tid = threadIdx.x, fmt = a.fmt;
    const int Hs = history_samples(a.n_taps, a.up);
    const size_t block = state_block_bytes(a.n_taps, a.up);
    // launched only where there is a state_out: its block is formed without the null test of state_block
    const unsigned char *sin = a.state_in ? a.state_in + (size_t)b * block : nullptr;
    unsigned char *sout = a.state_out + (size_t)b * block;
    const StateBlock blk{sin, sout, sout != sin};
    const int kb = stream_count(a.stream_blocks, b, a.n_blocks);
    if (kb == 0) {
        carry_idle_block<THREADS>(blk, block, tid);
        return;
    }
    const float *hist = reinterpret_cast<const float *>(blk.sin);
    float *hout = reinterpret_cast<float *>(blk.sout);
    const size_t row = (size_t)b * a.n_blocks * a.down;
    shift_history<THREADS>(Hs, (long long)kb * a.down, tid,
                           [&](const long long j) { return hist ? hist[j] : 0.0f; },
                           [&](const long long i) { return pcm_f32(a.audio, row + (size_t)i, fmt); },
                           [&](const int j, const float v) { hout[j] = v; });
    carry_words<THREADS>(blk, (size_t)Hs, block, tid);            // out of place: the padding travels too
}

// what both entry points ask of the design; LSM_OK, or the code with the message set
int check_design(const void *audio, int sample_format, const double *taps_dev, int n_taps, int up, int down)
{
    LSM_REQUIRE(sample_format == 0 || sample_format == 1, "sample_format=%d: 0 (float32) or 1 (int16)", sample_format);
    LSM_REQUIRE(up >= 1 && down >= 1, "up=%d and down=%d must be >= 1", up, down);
    LSM_REQUIRE(up != down, "up == down (%d): nothing to resample; copy the samples instead", up);
    LSM_REQUIRE(std::gcd(up, down) == 1, "up=%d and down=%d share the factor %d: reduce them", up, down, std::gcd(up, down));
    LSM_REQUIRE(n_taps >= 1, "n_taps=%d must be >= 1", n_taps);
    LSM_REQUIRE(audio && taps_dev, "resample: null buffer");
    LSM_REQUIRE_ALIGNED(audio, sample_format ? 2 : 4);
    LSM_REQUIRE_ALIGNED(taps_dev, 8);
    if (table_bytes(n_taps, up) > LDS_MAX) {
        lsm_set_error("the tap table of n_taps=%d, up=%d takes %ld bytes laid out by phase, over the %ld of a CU's LDS",
                      n_taps, up, table_bytes(n_taps, up), LDS_MAX);
        return LSM_ERR_UNSUPPORTED;
    }
    return LSM_OK;
}

template <typename Kernel>
void launch_tiles(Kernel kernel, long long outputs_per_row, int rows, const ResampleArgs &a, void *stream)
{
    const size_t lds = (size_t)table_bytes(a.n_taps, a.up);
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(kernel));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((outputs_per_row + TILE - 1) / TILE), rows), dim3(THREADS), lds,
                       (hipStream_t)stream, a);
}

}  // namespace

LSM_API long lsm_resample_state_bytes(int n_taps, int up)
{
    if (n_taps < 1 || up < 1) return 0;
    return (long)state_block_bytes(n_taps, up);
}

LSM_API int lsm_resample_f32(const void *audio, int sample_format, int n_clips, int n_in, const double *taps_dev, int n_taps,
                             int up, int down, int delay, int n_out, float *out, void *stream)
{
    const int rc = check_design(audio, sample_format, taps_dev, n_taps, up, down);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE(n_clips >= 1 && n_clips <= 65535, "n_clips=%d outside [1, 65535] (grid.y)", n_clips);
    LSM_REQUIRE(n_in >= 1 && n_out >= 1, "n_in=%d and n_out=%d must be >= 1", n_in, n_out);
    LSM_REQUIRE(delay >= 0 && (long long)delay * down < n_taps,
                "delay=%d does not fit the table: delay * down must lie in [0, n_taps = %d)", delay, n_taps);
    LSM_REQUIRE(out != nullptr, "out is required");
    LSM_REQUIRE_ALIGNED(out, 4);
    ResampleArgs a{};
    a.audio = audio; a.taps = taps_dev; a.out = out;
    a.fmt = sample_format; a.n_taps = n_taps; a.up = up; a.down = down;
    a.n_in = n_in; a.n_out = n_out; a.delay = delay;
    launch_tiles(resample_kernel, n_out, n_clips, a, stream);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_resample_stream_f32(const void *audio, int sample_format, int n_streams, int n_blocks, const double *taps_dev,
                                    int n_taps, int up, int down, const int32_t *stream_blocks, const void *state_in,
                                    void *state_out, float *out, void *stream)
{
    const int rc = check_design(audio, sample_format, taps_dev, n_taps, up, down);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE(n_streams >= 1 && n_streams <= 65535, "n_streams=%d outside [1, 65535] (grid.y)", n_streams);
    LSM_REQUIRE(n_blocks >= 1, "n_blocks=%d: a call's row stride G must be >= 1", n_blocks);
    LSM_REQUIRE((long long)n_blocks * down <= 0x7fffffffLL && (long long)n_blocks * up <= 0x7fffffffLL,
                "n_blocks * down and n_blocks * up must not exceed 2^31 - 1 samples per row");
    LSM_REQUIRE(out != nullptr, "out is required");
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE_ALIGNED(stream_blocks, 4);
    LSM_REQUIRE_ALIGNED(state_in, 16);
    LSM_REQUIRE_ALIGNED(state_out, 16);
    ResampleArgs a{};
    a.audio = audio; a.taps = taps_dev; a.out = out;
    a.stream_blocks = stream_blocks;
    a.state_in = static_cast<const unsigned char *>(state_in);
    a.state_out = static_cast<unsigned char *>(state_out);
    a.fmt = sample_format; a.n_taps = n_taps; a.up = up; a.down = down; a.n_blocks = n_blocks;
    launch_tiles(resample_stream_kernel, (long long)n_blocks * up, n_streams, a, stream);
    LSM_CHECK_HIP(hipGetLastError());
    if (state_out) {
        hipLaunchKernelGGL(resample_state_kernel, dim3(n_streams), dim3(THREADS), 0, (hipStream_t)stream, a);
        LSM_CHECK_HIP(hipGetLastError());
    }
    return LSM_OK;
}
