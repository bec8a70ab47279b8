// Silence trimming for gfx950 (SPEC.md §1.15, include/lsm_hip_trim.h): per clip, the energies of its 160-sample bins, the
// span of the bins that hold speech, and the clip's samples of that span moved to the start of its output row.
//
// Layout.  One workgroup of 256 threads (four wave64) per clip, three phases with LDS between them.
//   energies   The pinned sum of a bin -- 160 squares into one float64 accumulator, in ascending order -- is one lane's work.
//              A lane per bin reading global memory would stride 640 bytes from lane to lane, so the clip's samples go
//              through LDS in tiles of 64 bins: all threads stage 64 * 160 contiguous words with coalesced loads (a sample
//              at or behind len_b is not loaded and staged as +0.0), then lane j of the first wave walks row j.  The rows
//              have a pitch of 161 words: 161 mod 64 is odd, so the 64 lanes of a step hit 64 different banks (a pitch of
//              160 would put every lane on two).  The energies stay in LDS, 8 * time_bins bytes.
//   endpoints  max e_j, and the first and the last active bin: order-independent and exact, by LDS atomics on three words (a
//              float64 that is >= +0.0 orders like its bits taken as an unsigned integer).  The endpoint rule itself
//              (trim_body.h) is workgroup-uniform.
//   copy       the slice and the zero fill of the rest of the row, coalesced, by 16-byte accesses where source and
//              destination allow and by words otherwise.  Samples move as words, so -0.0 and NaN payloads stay.
// Every index is formed from clamped counts: 0 <= len_b <= n_samples, NB_b <= time_bins, first + bins <= NB_b.
#include "lsm_common.h"
#include "bin_energy.h"
#include "trim_body.h"
#include <cmath>

namespace {

using namespace lsm_trim;
using lsm_energy::PITCH;                    // the tile and the pinned sum: bin_energy.h, shared with endpoint.hip
using lsm_energy::TILE_BINS;
using lsm_energy::TILE_WORDS;

constexpr int THREADS = 256;

struct TrimArgs {
    const float *audio;                     // (n_clips, n_samples)
    const int32_t *clip_samples;            // (n_clips) or null
    float *out;                             // (n_clips, n_out)
    int32_t *first_out, *bins_out;          // (n_clips) or null
    double *energy_out;                     // (n_clips, time_bins) or null
    double ratio;
    int n_samples, time_bins, pad_bins, min_bins, n_out;
};

__global__ __launch_bounds__(THREADS) void trim_kernel(const TrimArgs a)
{
    extern __shared__ double energy[];                              // time_bins float64, then the tile
    float *tile = reinterpret_cast<float *>(energy + a.time_bins);
    __shared__ unsigned long long s_max;
    __shared__ int s_first, s_last, s_bad;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int len = clamp_len(a.clip_samples ? a.clip_samples[b] : a.n_samples, a.n_samples);
    const int nb = bins_of(len, a.time_bins);
    const float *__restrict__ in = a.audio + b * (size_t)a.n_samples;
    if (tid == 0) {
        s_max = 0ull;
        s_first = nb;
        s_last = -1;
        s_bad = 0;
    }

    // ---- energies ------------------------------------------------------------------------------------------------------
    for (int j0 = 0; j0 < nb; j0 += TILE_BINS) {
        const int nbt = min(TILE_BINS, nb - j0);
        lsm_energy::stage_bins<THREADS>(in, len, j0, nbt, tile, tid);   // < 160 * nb; read only below len <= n_samples
        __syncthreads();
        if (tid < nbt) energy[j0 + tid] = lsm_energy::row_energy(tile + tid * PITCH);
        __syncthreads();
    }
    if (nb == 0) __syncthreads();                                   // the scalars above, where no tile ran

    // ---- endpoints -----------------------------------------------------------------------------------------------------
    {
        double most = 0.0;
        bool bad = false;
        for (int j = tid; j < nb; j += THREADS) {
            const double e = energy[j];
            if (std::isfinite(e)) most = fmax(most, e);
            else bad = true;
        }
        if (most > 0.0) atomicMax(&s_max, (unsigned long long)__double_as_longlong(most));
        if (bad) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    {
        const double level = __longlong_as_double((long long)s_max) * a.ratio;
        int lo = nb, hi = -1;
        for (int j = tid; j < nb; j += THREADS) {
            if (energy[j] > level) {
                lo = min(lo, j);
                hi = max(hi, j);
            }
        }
        if (hi >= 0) {
            atomicMin(&s_first, lo);
            atomicMax(&s_last, hi);
        }
    }
    __syncthreads();
    const Span span = endpoints(nb, s_bad != 0 || s_last < 0, s_first, s_last, a.pad_bins, a.min_bins);
    if (tid == 0) {
        if (a.first_out) a.first_out[b] = span.first;
        if (a.bins_out) a.bins_out[b] = span.bins;
    }
    if (a.energy_out) {
        double *__restrict__ e_out = a.energy_out + b * (size_t)a.time_bins;
        for (int j = tid; j < a.time_bins; j += THREADS) e_out[j] = j < nb ? energy[j] : 0.0;
    }

    // ---- copy ----------------------------------------------------------------------------------------------------------
    const int n_out = a.n_out;
    const int valid = copied_samples(len, span);                    // <= 160 * time_bins <= n_out
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(in) + HOP * span.first;
    uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(a.out + b * (size_t)n_out);
    const bool quads = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    const int n_quads = quads ? valid / 4 : 0;
    for (int q = tid; q < n_quads; q += THREADS)
        reinterpret_cast<uint4 *>(dst)[q] = reinterpret_cast<const uint4 *>(src)[q];
    for (int m = 4 * n_quads + tid; m < valid; m += THREADS) dst[m] = src[m];
    // zeros from `valid` on: words up to the row's next 16-byte boundary, 16 bytes at a time from there, words at the end
    const int to_boundary = (int)((4u - ((reinterpret_cast<uintptr_t>(dst + valid) >> 2) & 3u)) & 3u);
    const int head = valid + min(to_boundary, n_out - valid);
    const int z_quads = (n_out - head) / 4;
    for (int m = valid + tid; m < head; m += THREADS) dst[m] = 0u;
    for (int q = tid; q < z_quads; q += THREADS) reinterpret_cast<uint4 *>(dst + head)[q] = make_uint4(0u, 0u, 0u, 0u);
    for (int m = head + 4 * z_quads + tid; m < n_out; m += THREADS) dst[m] = 0u;
}

}  // namespace

LSM_API int lsm_trim_lds_bytes(int time_bins)
{
    if (time_bins < MIN_BINS || time_bins > MAX_BINS) return LSM_ERR_ARG;
    return 8 * time_bins + 4 * TILE_WORDS;
}

LSM_API int lsm_trim_silence_f32(const float *audio, int n_clips, int n_samples, int time_bins, const int32_t *clip_samples,
                                 double ratio, int pad_bins, int min_bins, float *audio_out, int n_samples_out,
                                 int32_t *clip_first_out, int32_t *clip_bins_out, double *energy_out, void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_samples >= 1, "n_clips=%d must be >= 0 and n_samples=%d >= 1", n_clips, n_samples);
    LSM_REQUIRE(time_bins >= MIN_BINS, "time_bins=%d must be >= %d", time_bins, MIN_BINS);
    if (time_bins > MAX_BINS) {
        lsm_set_error("time_bins=%d: a clip's energies and endpoint reductions live in one workgroup's LDS, built for up to %d "
                      "bins", time_bins, MAX_BINS);
        return LSM_ERR_UNSUPPORTED;
    }
    LSM_REQUIRE(std::isfinite(ratio) && ratio >= 0.0 && ratio < 1.0, "ratio=%g must be finite and lie in [0, 1)", ratio);
    LSM_REQUIRE(pad_bins >= 0, "pad_bins=%d must be >= 0", pad_bins);
    LSM_REQUIRE(min_bins >= MIN_BINS && min_bins <= time_bins, "min_bins=%d outside [%d, time_bins=%d]", min_bins, MIN_BINS,
                time_bins);
    LSM_REQUIRE(audio && audio_out, "trim: audio and audio_out are required");
    LSM_REQUIRE(audio_out != audio, "audio_out must not be audio: a clip moves towards the start of its row");
    LSM_REQUIRE((long long)n_samples_out >= (long long)HOP * time_bins,
                "n_samples_out=%d must hold %d bins of %d samples", n_samples_out, time_bins, HOP);
    LSM_REQUIRE(((uintptr_t)audio & 3u) == 0 && ((uintptr_t)audio_out & 3u) == 0,
                "audio and audio_out must be 4-byte aligned");
    LSM_REQUIRE(((uintptr_t)clip_samples & 3u) == 0 && ((uintptr_t)clip_first_out & 3u) == 0
                && ((uintptr_t)clip_bins_out & 3u) == 0, "clip_samples, clip_first_out and clip_bins_out must be 4-byte aligned");
    LSM_REQUIRE(((uintptr_t)energy_out & 7u) == 0, "energy_out must be 8-byte aligned");
    if (n_clips == 0) return LSM_OK;
    TrimArgs a{};
    a.audio = audio; a.clip_samples = clip_samples; a.out = audio_out; a.first_out = clip_first_out;
    a.bins_out = clip_bins_out; a.energy_out = energy_out; a.ratio = ratio; a.n_samples = n_samples; a.time_bins = time_bins;
    a.pad_bins = pad_bins; a.min_bins = min_bins; a.n_out = n_samples_out;
    const size_t lds = (size_t)lsm_trim_lds_bytes(time_bins);
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(trim_kernel));
    hipLaunchKernelGGL(trim_kernel, dim3((unsigned)n_clips), dim3(THREADS), lds, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
