// Silence trimming (SPEC.md §1.15, include/lsm_hip_trim.h): the integer arithmetic of a clip -- the clamp of its sample count,
// its number of bins, the endpoint rule and the number of samples that move -- as host and device code, one copy: the kernel
// (trim.hip) and a host program (tests/trim_body_check.cc) compile this file.  Nothing here reads memory.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSM_TRIM_HD __host__ __device__
#else
#define LSM_TRIM_HD
#endif

namespace lsm_trim {

constexpr int HOP = 160;            // samples per bin (frontend.RAGGED_HOP)
constexpr int MIN_BINS = 3;         // a clip of fewer bins is kept whole
constexpr int MAX_BINS = 4096;      // time_bins of a launch: 3 .. 4096

struct Span {
    int first, bins;
};

// len_b: any int32 -> 0 .. n_samples (n_samples >= 1)
LSM_TRIM_HD inline int clamp_len(int v, int n_samples)
{
    return v < 0 ? 0 : (v > n_samples ? n_samples : v);
}

// NB_b = min(ceil(len / 160), time_bins), len >= 0; no sum that could pass INT_MAX
LSM_TRIM_HD inline int bins_of(int len, int time_bins)
{
    const int nb = len / HOP + (len % HOP != 0);
    return nb < time_bins ? nb : time_bins;
}

// The endpoint rule.  nb = NB_b; keep_whole: fewer than 3 bins, no active bin, or an energy that is not finite; otherwise
// 0 <= first_active <= last_active < nb.  pad_bins >= 0, 3 <= min_bins.  Returns 0 <= first, first + bins <= nb.
LSM_TRIM_HD inline Span endpoints(int nb, bool keep_whole, int first_active, int last_active, int pad_bins, int min_bins)
{
    if (keep_whole || nb < MIN_BINS) return Span{0, nb};
    const int pad = pad_bins < nb ? pad_bins : nb;              // a pad of nb already reaches both ends: no sum overflows
    int lo = first_active - pad, hi = last_active + pad;
    if (lo < 0) lo = 0;
    if (hi > nb - 1) hi = nb - 1;
    const int m = min_bins < nb ? min_bins : nb;
    if (hi - lo + 1 < m) {
        const int need = m - (hi - lo + 1);
        const int room = nb - 1 - hi;
        const int g = need < room ? need : room;
        hi += g;
        lo -= need - g;                                         // m <= nb: lo stays >= 0
    }
    return Span{lo, hi - lo + 1};
}

// How many samples of the slice [160 * first, 160 * (first + bins)) lie below len: they are copied, the rest of the row is +0.0
LSM_TRIM_HD inline int copied_samples(int len, Span s)
{
    const int from = HOP * s.first, want = HOP * s.bins;       // <= 160 * 4096
    const int have = len > from ? len - from : 0;
    return have < want ? have : want;
}

}  // namespace lsm_trim
