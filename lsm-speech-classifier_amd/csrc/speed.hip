// Speed perturbation for gfx950 (SPEC.md §1.12, include/lsm_hip_speed.h): every clip of a batch played at its own speed in
// one launch.  A clip played s times faster is the clip resampled from 16000 * s Hz to 16000 Hz, so the arithmetic is the
// resampler's (resample_body.h: the table's layout in LDS and the tap loop, one copy); what this kernel adds is a bank of
// up to 16 designs and a per-clip choice among them.
//
// Layout.  The tile geometry of resample_kernel: grid (tiles of 2048 outputs, n_clips), 512 threads.  A workgroup serves
// one clip and so one design: it reads the clip's row, which is made a scalar value, picks that design's five numbers out
// of the table that travels BY VALUE in the kernel arguments (kernarg memory, read with scalar loads at a scalar offset:
// no private copy, no scratch), and stages that design's taps from the concatenated tap array into LDS.  Dynamic LDS is
// the largest table of the bank.  Two kinds of tile never touch LDS and leave ahead of the barrier, both on
// workgroup-uniform conditions: a clip without a design (row < 0: copy, then zeros) and a tile that lies wholly at or
// behind ceil((n_in + Hs) * up / down), where every tap of every output meets a zero (finite taps: +0.0).
//
// The ragged form (SPEC.md §1.18, include/lsm_hip_ragged_speed.h) is the kernel's second instantiation: the clip's own
// sample count, clamped and made a scalar like its row, stands where n_in stood, so a tap that reaches outside the clip
// meets +0.0 as it does outside the row; the clip ends at n' = ragged_length(...), a scalar too, behind which the row is
// zeros (the clip alone has no ring-out tail), so a tile at or behind n' leaves ahead of the table like a tile of zeros
// above; and thread 0 of tile 0 stores n' and its bins.  The plain instantiation compiles none of this.
#include "resample_body.h"
#include <numeric>
#include <type_traits>

namespace {

using namespace lsm_resample;

constexpr int MAX_DESIGNS = 16;

struct SpeedDesign {
    int up, down, n_taps, delay, tap_offset;
};

struct SpeedArgs {
    const void *audio;                  // (n_clips, n_in) float32 or int16
    const double *taps;                 // the designs' taps one behind the other
    float *out;                         // (n_clips, n_out)
    const int32_t *design_row;          // (n_clips) or null
    int fmt, n_in, n_out, n_designs;
    SpeedDesign design[MAX_DESIGNS];
};

// what the ragged launch takes beside: the clips' sample counts and where their new counts go (each may be null)
struct RaggedSpeedArgs : SpeedArgs {
    const int32_t *clip_samples;        // (n_clips)
    int32_t *clip_samples_out, *clip_bins_out;
    int time_bins;
};

constexpr int HOP = 160;                // samples per time bin of the ragged launches

template <bool RAGGED>
__global__ __launch_bounds__(THREADS) void speed_kernel(const std::conditional_t<RAGGED, RaggedSpeedArgs, SpeedArgs> a)
{
    extern __shared__ double tab[];
    const int b = blockIdx.y, fmt = a.fmt, stride = a.n_in, n_out = a.n_out;
    // one value per workgroup: a scalar, so that everything chosen by it is scalar too
    const int r = __builtin_amdgcn_readfirstlane(a.design_row ? a.design_row[b] : 0);
    // the clip's samples: the row's, or the clip's own count, clamped so that no int32 reaches outside the row
    int n_in = stride;
    if constexpr (RAGGED) n_in = __builtin_amdgcn_readfirstlane(min(max(a.clip_samples[b], 0), stride));
    const size_t row = (size_t)b * stride;
    const void *__restrict__ audio = a.audio;
    float *__restrict__ out = a.out + (size_t)b * n_out;
    const long long m0 = (long long)blockIdx.x * TILE;
    // ragged: the clip's new counts, n_new <= n_out samples and their bins, by one thread of the clip's first tile
    [[maybe_unused]] auto store_counts = [&](const int n_new) {
        if constexpr (RAGGED) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                if (a.clip_samples_out) a.clip_samples_out[b] = n_new;
                if (a.clip_bins_out) a.clip_bins_out[b] = min((n_new + HOP - 1) / HOP, a.time_bins);
            }
        }
    };
    if (r < 0) {
        // an unperturbed clip: its bits (a float32 sample moves as a word, so -0.0 and NaN payloads stay), then +0.0
        store_counts(min(n_in, n_out));
        const uint32_t *__restrict__ words = static_cast<const uint32_t *>(audio);
        uint32_t *__restrict__ out_words = reinterpret_cast<uint32_t *>(out);
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const long long m = m0 + q * THREADS + threadIdx.x;
            if (m >= n_out) continue;
            if (m >= n_in) out[m] = 0.0f;
            else if (fmt) out[m] = pcm_f32(audio, row + (size_t)m, 1);
            else out_words[m] = words[row + (size_t)m];
        }
        return;
    }
    const SpeedDesign d = a.design[max(min(r, a.n_designs - 1), 0)];  // r >= 0 here; the index is in range on its own
    const int up = d.up, down = d.down, n_taps = d.n_taps, delay = d.delay;
    // From here on z reads zeros only: i0 - Hs >= n_in for every m' = m + delay >= zero_from.  Ragged: the clip ends at
    // n' and every output from there on IS +0.0 (n' >= 1 wherever a sample is formed, so n_in >= 1 there).
    long long zero_from;
    if constexpr (RAGGED) {
        zero_from = ragged_length(n_in, up, down, n_out);
        store_counts((int)zero_from);
    } else {
        zero_from = (((long long)n_in + history_samples(n_taps, up)) * up + down - 1) / down;
    }
    if (m0 >= zero_from) {
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const long long m = m0 + q * THREADS + threadIdx.x;
            if (m < n_out) out[m] = 0.0f;
        }
        return;
    }
    load_table(tab, a.taps + d.tap_offset, n_taps, up);
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const long long m = m0 + q * THREADS + threadIdx.x;
        if (m >= n_out) continue;
        if constexpr (RAGGED) {
            if (m >= zero_from) {
                out[m] = 0.0f;
                continue;
            }
        }
        const long long p = (m + delay) * down;
        out[m] = causal_sample(tab, n_taps, up, p / up, (int)(p % up), [&](const long long i) {
            // read at a clamped index and keep or drop the value (resample_kernel)
            const float v = pcm_f32(audio, row + (size_t)min(max(i, 0LL), (long long)n_in - 1), fmt);
            return (i >= 0 && i < n_in) ? (double)v : 0.0;
        });
    }
}

// What a design must satisfy whatever it is used with: the conditions of the resampler's check_design that speak of the
// design alone, and a tap offset that is no index below 0.
const char *design_fault(const int32_t *d)
{
    const int up = d[0], down = d[1], n_taps = d[2], delay = d[3], tap_offset = d[4];
    if (up < 1 || down < 1) return "up and down must be >= 1";
    if (up == down) return "up == down: nothing to resample; give such a clip a row below 0 instead";
    if (std::gcd(up, down) != 1) return "up and down share a factor: reduce them";
    if (n_taps < 1) return "n_taps must be >= 1";
    if (delay < 0 || (long long)delay * down >= n_taps) return "delay does not fit the table: delay * down must lie in [0, n_taps)";
    if (tap_offset < 0) return "tap_offset must be >= 0";
    return nullptr;
}

}  // namespace

LSM_API long lsm_speed_lds_bytes(const int32_t *designs, int n_designs)
{
    if (!designs || n_designs < 1 || n_designs > MAX_DESIGNS) return 0;
    long most = 0;
    for (int r = 0; r < n_designs; ++r) {
        const int32_t *d = designs + 5 * r;
        if (design_fault(d) || table_bytes(d[2], d[0]) > LDS_MAX) return 0;
        most = std::max(most, table_bytes(d[2], d[0]));
    }
    return most;
}

namespace {

// lsm_speed_f32's refusals in its order, then the launch's arguments and its dynamic LDS: one copy for both entry points
int checked_launch(const void *audio, int sample_format, int n_clips, int n_in, const double *taps_dev, int n_taps_total,
                   const int32_t *designs, int n_designs, const int32_t *design_row, int n_out, float *out, SpeedArgs &a,
                   size_t &lds)
{
    LSM_REQUIRE(sample_format == 0 || sample_format == 1, "sample_format=%d: 0 (float32) or 1 (int16)", sample_format);
    LSM_REQUIRE(n_designs >= 1 && n_designs <= MAX_DESIGNS, "n_designs=%d outside [1, %d]", n_designs, MAX_DESIGNS);
    LSM_REQUIRE(designs != nullptr, "designs is required (host memory, n_designs rows of up, down, n_taps, delay, tap_offset)");
    LSM_REQUIRE(n_taps_total >= 1, "n_taps_total=%d must be >= 1", n_taps_total);
    for (int r = 0; r < n_designs; ++r) {
        const int32_t *d = designs + 5 * r;
        const char *fault = design_fault(d);
        LSM_REQUIRE(!fault, "design %d (up=%d, down=%d, n_taps=%d, delay=%d, tap_offset=%d): %s", r, d[0], d[1], d[2], d[3],
                    d[4], fault);
        LSM_REQUIRE((long long)d[4] + d[2] <= n_taps_total,
                    "design %d: tap_offset=%d + n_taps=%d runs past the n_taps_total=%d values of taps_dev", r, d[4], d[2],
                    n_taps_total);
    }
    LSM_REQUIRE(audio && taps_dev, "speed: null buffer");
    LSM_REQUIRE_ALIGNED(audio, sample_format ? 2 : 4);
    LSM_REQUIRE_ALIGNED(taps_dev, 8);
    LSM_REQUIRE_ALIGNED(design_row, 4);
    LSM_REQUIRE(n_clips >= 1 && n_clips <= 65535, "n_clips=%d outside [1, 65535] (grid.y)", n_clips);
    LSM_REQUIRE(n_in >= 1 && n_out >= 1, "n_in=%d and n_out=%d must be >= 1", n_in, n_out);
    LSM_REQUIRE(out != nullptr, "out is required");
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE(out != audio, "out must not be audio: an output reads the samples around it");
    lds = 0;
    for (int r = 0; r < n_designs; ++r) {
        const int32_t *d = designs + 5 * r;
        if (table_bytes(d[2], d[0]) > LDS_MAX) {
            lsm_set_error("the tap table of design %d (n_taps=%d, up=%d) takes %ld bytes laid out by phase, over the %ld of a "
                          "CU's LDS", r, d[2], d[0], table_bytes(d[2], d[0]), LDS_MAX);
            return LSM_ERR_UNSUPPORTED;
        }
        lds = std::max(lds, (size_t)table_bytes(d[2], d[0]));
        a.design[r] = SpeedDesign{d[0], d[1], d[2], d[3], d[4]};
    }
    a.audio = audio; a.taps = taps_dev; a.out = out; a.design_row = design_row;
    a.fmt = sample_format; a.n_in = n_in; a.n_out = n_out; a.n_designs = n_designs;
    return LSM_OK;
}

template <bool RAGGED, typename Args>
int launch(const Args &a, int n_clips, size_t lds, void *stream)
{
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(&speed_kernel<RAGGED>));
    hipLaunchKernelGGL(speed_kernel<RAGGED>, dim3((unsigned)(((long long)a.n_out + TILE - 1) / TILE), n_clips), dim3(THREADS),
                       lds, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

}  // namespace

LSM_API int lsm_speed_f32(const void *audio, int sample_format, int n_clips, int n_in, const double *taps_dev, int n_taps_total,
                          const int32_t *designs, int n_designs, const int32_t *design_row, int n_out, float *out,
                          void *stream)
{
    SpeedArgs a{};
    size_t lds = 0;
    if (const int rc = checked_launch(audio, sample_format, n_clips, n_in, taps_dev, n_taps_total, designs, n_designs,
                                      design_row, n_out, out, a, lds))
        return rc;
    return launch<false>(a, n_clips, lds, stream);
}

LSM_API int lsm_speed_ragged_length(int n_b, int up, int down, int n_out)
{
    LSM_REQUIRE(up >= 1 && down >= 1 && n_out >= 0, "up=%d and down=%d must be >= 1, n_out=%d >= 0", up, down, n_out);
    return ragged_length(std::max(n_b, 0), up, down, n_out);
}

LSM_API int lsm_speed_ragged_f32(const void *audio, int sample_format, int n_clips, int n_in, const int32_t *clip_samples,
                                 const double *taps_dev, int n_taps_total, const int32_t *designs, int n_designs,
                                 const int32_t *design_row, int n_out, float *out, int32_t *clip_samples_out,
                                 int32_t *clip_bins_out, int time_bins, void *stream)
{
    RaggedSpeedArgs a{};
    size_t lds = 0;
    if (const int rc = checked_launch(audio, sample_format, n_clips, n_in, taps_dev, n_taps_total, designs, n_designs,
                                      design_row, n_out, out, a, lds))
        return rc;
    LSM_REQUIRE(clip_samples != nullptr, "speed: null clip_samples (the ragged launch needs every clip's sample count)");
    LSM_REQUIRE_ALIGNED(clip_samples, 4);
    LSM_REQUIRE_ALIGNED(clip_samples_out, 4);
    LSM_REQUIRE_ALIGNED(clip_bins_out, 4);
    if (clip_bins_out) {
        LSM_REQUIRE(time_bins >= 3, "time_bins=%d: a row of the ragged launches has at least 3 time bins", time_bins);
        LSM_REQUIRE(n_out >= (long long)HOP * time_bins, "n_out=%d is less than the %d * time_bins=%d samples of a row of the "
                    "ragged launches", n_out, HOP, time_bins);
    }
    a.clip_samples = clip_samples; a.clip_samples_out = clip_samples_out; a.clip_bins_out = clip_bins_out;
    a.time_bins = time_bins;
    return launch<true>(a, n_clips, lds, stream);
}
