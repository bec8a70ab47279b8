// Reverberation (SPEC.md §1.11): what the batch and the streamed kernels of reverb.hip share -- the staged input tile's
// layout in LDS and the tap loop of one tile of outputs.
//
// One output is   acc = +0.0;  for k = 0, 1, ... < len ascending:  acc = fma((double)h[k], (double)x[i - k], acc);  y[i] = (float)acc.
// The product of two float32 values is exact in float64, so the fma gives the bits of acc + h * x (SPEC §1.11); the
// translation unit keeps -ffp-contract=off and the fma below is explicit.
//
// Layout.  A workgroup of THREADS lanes makes a tile of TILE = THREADS * R consecutive outputs, lane t the R outputs
// o0 + t * R + j.  For tap k output j reads x[o0 + t * R + j - k]: one step down per tap, so a lane keeps a sliding window
// of its input in registers and needs ONE new sample per tap for its R multiply-adds.  The tap row is walked in chunks of
// at most CHUNK taps; for a chunk [k0, k0 + kc) the samples S[p] = x[s0 + p], s0 = o0 - k0 - kce + 1 (kce = kc rounded up to
// R), are staged as float64 in LDS at [p mod R][p / R]: the lanes of a wave then read consecutive doubles of one row for
// every window slot, where a flat layout would put lanes R samples apart on the same banks.  The chunk's taps are staged
// as float64 as well; every lane reads the same tap, which the LDS broadcasts.  LDS use is fixed, whatever K.
#pragma once
#include "stream_state.h"

namespace lsm_reverb {

constexpr int THREADS = 256;
constexpr int R = 8;                         // consecutive outputs of a lane: independent accumulators in flight
constexpr int TILE = THREADS * R;            // outputs of a workgroup
constexpr int CHUNK = 1024;                  // taps staged at a time (a multiple of R)
constexpr int MAX_TAPS = 16384;
constexpr int MAX_SAMPLES = 1 << 24;
constexpr int ROWS = THREADS + CHUNK / R + 1;          // rows of R samples that a chunk can touch
// Row stride in doubles.  Reads walk along a row and never conflict; the staging stores put R consecutive samples into R
// different rows, and a stride of 2 mod 16 doubles spreads a 16-lane store group over all 32 banks.
constexpr int STRIDE = ((ROWS + 13) / 16) * 16 + 2;
static_assert(STRIDE >= ROWS && STRIDE % 16 == 2 && CHUNK % R == 0, "LDS layout");

struct Tile {
    double samples[R * STRIDE];
    double taps[CHUNK + R];                     // a group of taps is read one group ahead
};

// The state of a stream: its last n_taps - 1 input samples as float32, in a block rounded up to 16 bytes, never below 16
__host__ __device__ inline size_t state_block_bytes(int n_taps)
{
    const size_t used = (size_t)(n_taps - 1) * 4;
    return used ? lsm_state::state_round16(used) : 16;
}

// R taps of one lane: tp[e] against the window g[0 .. 2R - 2] = S[R * row + 0 ..], whose lower R values are `lo` (row `row`)
// and whose upper R - 1 are `hi` (row `row + 1`); output j of tap e reads g[R - 1 - e + j].  `nt` taps of the group are real
// (workgroup-uniform); `full` drops the test from the groups in front of a row's last.
template <bool full>
__device__ __forceinline__ void tap_group(double (&acc)[R], const double (&lo)[R], const double (&hi)[R], const double (&tp)[R],
                                          int nt)
{
#pragma unroll
    for (int e = 0; e < R; ++e) {
        if (full || e < nt) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int m = R - 1 - e + j;
                acc[j] = fma(tp[e], m < R ? lo[m] : hi[m - R], acc[j]);
            }
        }
    }
}

__device__ __forceinline__ void load_row(double (&d)[R], const Tile &lds, int row)
{
#pragma unroll
    for (int m = 0; m < R; ++m) d[m] = lds.samples[m * STRIDE + row];
}

__device__ __forceinline__ void load_taps(double (&d)[R], const Tile &lds, int u)
{
#pragma unroll
    for (int e = 0; e < R; ++e) d[e] = lds.taps[u * R + e];
}

// y[o0 + t * R + j] for the lane's R outputs, over taps h[0 .. len) (global memory, float32).  `sample(i)` is x[i] as float32
// for any long long i the tile can ask for, +0.0 outside the signal: such a sample goes through the multiply and the add
// like any other.  `busy` (wave-uniform) false: the wave owns no output that is kept; it stages and waits but skips the
// arithmetic.  Every thread of the workgroup calls this (barriers inside).
template <typename Sample>
__device__ __forceinline__ void convolve_tile(Tile &lds, const float *__restrict__ h, int len, long long o0, bool busy,
                                              double (&acc)[R], Sample sample)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < len; k0 += CHUNK) {
        const int kc = min(CHUNK, len - k0);
        const int kce = (kc + R - 1) / R * R;
        const long long s0 = o0 - k0 - kce + 1;
        const int staged = TILE + kce;                   // S[0 .. TILE + kce - 2] is read; one more keeps the count even
        __syncthreads();                                 // the chunk before has been read
        // four loads in flight per lane: `sample` reads at clamped indices, so a load past the staged range is harmless
        for (int p0 = t; p0 < staged; p0 += 4 * THREADS) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = sample(s0 + p0 + q * THREADS);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = p0 + q * THREADS;
                if (p < staged) lds.samples[(p % R) * STRIDE + p / R] = (double)v[q];
            }
        }
        for (int k = t; k < kc; k += THREADS) lds.taps[k] = (double)h[k0 + k];
        __syncthreads();
        if (!busy) continue;
        // Group u of R taps reads rows t + kce / R - 1 - u and the one above it.  The next group's row and taps are read
        // before this group's arithmetic, into the buffer the group before has done with: three groups per turn, so that
        // a row goes from "next" to lower half to upper half by its name, not by a copy.
        const int full = kc / R, rem = kc - full * R;
        int row = t + kce / R - 1, u = 0;
        // one group: false once the chunk's last tap is done
        auto group = [&](const double (&lo)[R], const double (&hi)[R], const double (&tp)[R], double (&next)[R],
                         double (&next_tp)[R]) {
            if (u >= full) {
                if (rem) tap_group<false>(acc, lo, hi, tp, rem);
                return false;
            }
            load_row(next, lds, max(row - 1, 0));
            load_taps(next_tp, lds, u + 1);
            tap_group<true>(acc, lo, hi, tp, R);
            --row;
            ++u;
            return true;
        };
        double A[R], B[R], D[R], TA[R], TB[R], TD[R];
        load_row(B, lds, row + 1);
        load_row(A, lds, row);
        load_taps(TA, lds, 0);
        while (group(A, B, TA, D, TB) && group(D, A, TB, B, TD) && group(B, D, TD, A, TA)) {}
    }
}

}  // namespace lsm_reverb
