// The bin energy of SPEC.md §1.15 as device code, one copy: the silence trimmer (trim.hip) and the stream endpoint detector
// (endpoint.hip, §1.17) sum the same 160 squares in the same order.  A lane per bin reading global memory would stride 640
// bytes from lane to lane, so the samples go through LDS in tiles of up to 64 bins: all threads stage the tile's contiguous
// words with coalesced loads, then one lane walks one row.  The rows have a pitch of 161 words: 161 mod 64 is odd, so the 64
// lanes of a step hit 64 different banks (a pitch of 160 would put every lane on two).
#pragma once
#include "trim_body.h"

namespace lsm_energy {

constexpr int TILE_BINS = 64;                       // one wave sums a tile
constexpr int PITCH = lsm_trim::HOP + 1;            // words per staged bin: odd mod 64
constexpr int TILE_WORDS = TILE_BINS * PITCH;

// All THREADS threads: bins j0 .. j0 + nbt - 1 of `in` into `tile`; a sample at or behind `len` is not loaded and staged as
// +0.0.  The caller synchronises before the rows are read.
template <int THREADS>
__device__ inline void stage_bins(const float *__restrict__ in, int len, int j0, int nbt, float *tile, int tid)
{
    const int base = lsm_trim::HOP * j0;
    for (int k = tid; k < lsm_trim::HOP * nbt; k += THREADS) {
        const int at = base + k;                    // < 160 * (j0 + nbt); read only below len
        tile[(k / lsm_trim::HOP) * PITCH + k % lsm_trim::HOP] = at < len ? in[at] : 0.0f;
    }
}

// One lane: the pinned sum of a staged row -- one float64 accumulator from +0.0, i ascending, (double)x squared.
__device__ inline double row_energy(const float *row)
{
    double acc = 0.0;
#pragma unroll 16
    for (int i = 0; i < lsm_trim::HOP; ++i) {
        const double x = (double)row[i];
        acc += x * x;
    }
    return acc;
}

}  // namespace lsm_energy
