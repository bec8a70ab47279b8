// Reverberation for gfx950 (SPEC.md §1.11, include/lsm_hip_reverb.h): every clip or stream convolved with a row of a bank of
// room impulse responses, in front of the noise mixer.  Two forms over one tap loop (reverb_body.h):
//   batch     reverb_kernel          grid (tiles, n_clips): y[i] = sum over k < len of h[k] * x[i - k], zeros outside the clip;
//   streamed  reverb_stream_kernel   grid (tiles, n_streams): the same on [history | new samples], then
//             reverb_state_kernel    one workgroup per stream: the last K - 1 samples become the new history.
// The kernel boundary orders every read of the old history before its in-place shift (DESIGN.md "The state block").
//
// A workgroup of 256 lanes makes 2048 consecutive outputs of one row, a lane 8 of them from a sliding register window; the
// input tile and the taps of a chunk are staged in LDS as float64 (33 KB, four workgroups per CU).  A dry row copies.
#include "reverb_body.h"

namespace {

using namespace lsm_reverb;
using namespace lsm_state;

struct ReverbArgs {
    const float *audio;                 // batch (n_clips, n_in); streamed (n_streams, n_cols)
    const float *rir;                   // (M, K)
    float *out;                         // batch (n_clips, n_out); streamed (n_streams, n_cols)
    const int32_t *rir_len;             // (M) or null: K everywhere
    const int32_t *rir_row;             // (rows) or null: row 0
    const int32_t *count;               // streamed: (n_streams) or null: n_cols
    const unsigned char *state_in;      // or null: every stream starts
    unsigned char *state_out;           // or null; may be state_in
    int n_in, n_out, M, K;
};

// the row of stream or clip b (negative: dry) and its length
__device__ __forceinline__ int row_of(const ReverbArgs &a, int b, int &len)
{
    const int raw = a.rir_row ? a.rir_row[b] : 0;
    const int r = min(max(raw, 0), a.M - 1);
    len = clamped_at(a.rir_len, r, 1, a.K, a.K);
    return raw < 0 ? -1 : r;
}

// The lane's R outputs o .. o + R - 1 of a row, those below `limit` only
__device__ __forceinline__ void store_outputs(float *__restrict__ out, long long o, long long limit, const double (&acc)[R])
{
    if (o + R <= limit && ((uintptr_t)(out + o) & 15u) == 0) {
        float4 *dst = reinterpret_cast<float4 *>(out + o);
#pragma unroll
        for (int q = 0; q < R / 4; ++q)
            dst[q] = make_float4((float)acc[4 * q], (float)acc[4 * q + 1], (float)acc[4 * q + 2], (float)acc[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (o + j < limit) out[o + j] = (float)acc[j];
    }
}

__global__ __launch_bounds__(THREADS) void reverb_kernel(const ReverbArgs a)
{
    __shared__ Tile lds;
    const int b = blockIdx.y, t = threadIdx.x, n = a.n_in;
    const long long o0 = (long long)blockIdx.x * TILE, n_out = a.n_out;
    const float *__restrict__ x = a.audio + (size_t)b * n;
    float *__restrict__ out = a.out + (size_t)b * n_out;
    int len;
    const int r = row_of(a, b, len);
    if (r < 0) {                                                                // dry: the clip's bits, +0.0 behind it
        const uint32_t *src = reinterpret_cast<const uint32_t *>(x);
        uint32_t *dst = reinterpret_cast<uint32_t *>(out);
        for (long long i = o0 + t; i < min(o0 + TILE, n_out); i += THREADS) dst[i] = i < n ? src[i] : 0u;
        return;
    }
    const long long o = o0 + (long long)t * R;
    const bool busy = o0 + (long long)(t & ~(LSM_WAVE - 1)) * R < n_out;        // wave-uniform
    double acc[R];
    convolve_tile(lds, a.rir + (size_t)r * a.K, len, o0, busy, acc, [&](const long long i) {
        // read at a clamped index and keep or drop the value (no guarded load)
        const float v = x[min(max(i, 0LL), (long long)n - 1)];
        return (i >= 0 && i < n) ? v : 0.0f;
    });
    store_outputs(out, o, n_out, acc);
}

__global__ __launch_bounds__(THREADS) void reverb_stream_kernel(const ReverbArgs a)
{
    __shared__ Tile lds;
    const int b = blockIdx.y, t = threadIdx.x, H = a.n_in, Hs = a.K - 1;
    const long long o0 = (long long)blockIdx.x * TILE;
    const long long c = stream_count(a.count, b, H);
    if (o0 >= c) return;                                                        // workgroup-uniform
    const float *__restrict__ x = a.audio + (size_t)b * H;
    float *__restrict__ out = a.out + (size_t)b * H;
    int len;
    const int r = row_of(a, b, len);
    if (r < 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(x);
        uint32_t *dst = reinterpret_cast<uint32_t *>(out);
        for (long long i = o0 + t; i < min(o0 + TILE, c); i += THREADS) dst[i] = src[i];
        return;
    }
    // without a state block the history is zeros and nothing is loaded for it
    const bool have_hist = a.state_in != nullptr && Hs > 0;
    const float *__restrict__ hist =
        have_hist ? reinterpret_cast<const float *>(a.state_in + (size_t)b * state_block_bytes(a.K)) : nullptr;
    const long long o = o0 + (long long)t * R;
    const bool busy = o0 + (long long)(t & ~(LSM_WAVE - 1)) * R < c;
    double acc[R];
    convolve_tile(lds, a.rir + (size_t)r * a.K, len, o0, busy, acc, [&](const long long i) {
        // an output below c reads i < c and i >= -(K - 1); both sources at clamped indices, below the history +0.0
        const float v = x[min(max(i, 0LL), (long long)H - 1)];
        const float p = have_hist ? hist[min(max(i + Hs, 0LL), (long long)max(Hs, 1) - 1)] : 0.0f;
        return i >= 0 ? v : (i >= -(long long)Hs ? p : 0.0f);
    });
    store_outputs(out, o, c, acc);
}

// grid = n_streams, one workgroup each: the last K - 1 samples of [history | this push's c samples]
__global__ __launch_bounds__(THREADS) void reverb_state_kernel(const ReverbArgs a)
{
    const int b = blockIdx.x, tid = threadIdx.x, H = a.n_in, Hs = a.K - 1;
    const size_t block = state_block_bytes(a.K);
    // launched only where there is a state_out: its block is formed without the null test of state_block
    const unsigned char *sin = a.state_in ? a.state_in + (size_t)b * block : nullptr;
    unsigned char *sout = a.state_out + (size_t)b * block;
    const StateBlock blk{sin, sout, sout != sin};
    const int c = stream_count(a.count, b, H);
    if (c == 0) {
        carry_idle_block<THREADS>(blk, block, tid);
        return;
    }
    // samples move as words, so -0.0 and NaN payloads stay
    const uint32_t *win = reinterpret_cast<const uint32_t *>(blk.sin);
    uint32_t *wout = reinterpret_cast<uint32_t *>(blk.sout);
    const uint32_t *x = reinterpret_cast<const uint32_t *>(a.audio + (size_t)b * H);
    shift_history<THREADS>(Hs, c, tid,
                           [&](const long long j) { return win ? win[j] : 0u; },
                           [&](const long long i) { return x[i]; },
                           [&](const int j, const uint32_t v) { wout[j] = v; });
    carry_words<THREADS>(blk, (size_t)Hs, block, tid);            // out of place: the padding travels too
}

// what both entry points ask of the bank and of a row's shape; LSM_OK, or the code with the message set
int check_bank(const char *what, int n, int n_rows, int n_rir_rows, int n_taps)
{
    LSM_REQUIRE(n_taps >= 1 && n_taps <= MAX_TAPS, "n_taps=%d outside [1, %d]", n_taps, MAX_TAPS);
    LSM_REQUIRE(n_rir_rows >= 1, "n_rir_rows=%d must be >= 1", n_rir_rows);
    LSM_REQUIRE(n >= 1 && n <= MAX_SAMPLES, "%s=%d outside [1, %d]", what, n, MAX_SAMPLES);
    LSM_REQUIRE(n_rows >= 0 && n_rows <= 65535, "%d rows outside [0, 65535] (grid.y)", n_rows);
    return LSM_OK;
}

}  // namespace

LSM_API long lsm_reverb_state_bytes(int n_taps)
{
    if (n_taps < 1 || n_taps > MAX_TAPS) return 0;
    return (long)state_block_bytes(n_taps);
}

LSM_API int lsm_reverb_f32(const float *audio, int n_clips, int n_in, const float *rir, int n_rir_rows, int n_taps,
                           const int32_t *rir_len, const int32_t *rir_row, int n_out, float *out, void *stream)
{
    const int rc = check_bank("n_in", n_in, n_clips, n_rir_rows, n_taps);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE(n_out >= 1, "n_out=%d must be >= 1", n_out);
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE_ALIGNED(rir, 4);
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE_ALIGNED(rir_len, 4);
    LSM_REQUIRE_ALIGNED(rir_row, 4);
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(audio && rir && out, "reverb: null buffer (audio, rir and out are required)");
    LSM_REQUIRE(out != audio, "out must not be audio: an output reads the samples in front of it");
    ReverbArgs a{};
    a.audio = audio; a.rir = rir; a.out = out; a.rir_len = rir_len; a.rir_row = rir_row;
    a.n_in = n_in; a.n_out = n_out; a.M = n_rir_rows; a.K = n_taps;
    hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)(((long long)n_out + TILE - 1) / TILE), n_clips), dim3(THREADS), 0,
                       (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_reverb_stream_f32(const float *audio, int n_streams, int n_cols, const float *rir, int n_rir_rows, int n_taps,
                                  const int32_t *rir_len, const int32_t *rir_row, const int32_t *count, const void *state_in,
                                  void *state_out, float *out, void *stream)
{
    const int rc = check_bank("n_cols", n_cols, n_streams, n_rir_rows, n_taps);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE_ALIGNED(rir, 4);
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE_ALIGNED(rir_len, 4);
    LSM_REQUIRE_ALIGNED(rir_row, 4);
    LSM_REQUIRE_ALIGNED(count, 4);
    LSM_REQUIRE_ALIGNED(state_in, 16);
    LSM_REQUIRE_ALIGNED(state_out, 16);
    if (n_streams == 0) return LSM_OK;
    LSM_REQUIRE(audio && rir && out, "reverb stream: null buffer (audio, rir and out are required)");
    LSM_REQUIRE(out != audio, "out must not be audio: an output reads the samples in front of it");
    ReverbArgs a{};
    a.audio = audio; a.rir = rir; a.out = out; a.rir_len = rir_len; a.rir_row = rir_row; a.count = count;
    a.state_in = static_cast<const unsigned char *>(state_in);
    a.state_out = static_cast<unsigned char *>(state_out);
    a.n_in = n_cols; a.n_out = n_cols; a.M = n_rir_rows; a.K = n_taps;
    hipLaunchKernelGGL(reverb_stream_kernel, dim3((unsigned)((n_cols + TILE - 1) / TILE), n_streams), dim3(THREADS), 0,
                       (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    if (state_out) {
        hipLaunchKernelGGL(reverb_state_kernel, dim3(n_streams), dim3(THREADS), 0, (hipStream_t)stream, a);
        LSM_CHECK_HIP(hipGetLastError());
    }
    return LSM_OK;
}
