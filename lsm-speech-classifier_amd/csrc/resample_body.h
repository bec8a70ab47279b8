// Polyphase FIR resampler (SPEC.md §1.8): what the batch and the streamed kernels of resample.hip share -- the tap table's
// layout in LDS and the tap loop of one output sample.
//
// The causal sample z[m] of a signal x is, with p = m * down and k0 = p mod up,
//     acc = +0.0;  for k = k0, k0 + up, ... < K:  acc = acc + hp[k] * x[(p - k) / up];  z[m] = (float)acc
// in float64 without FMA (the translation unit is compiled with -ffp-contract=off).  (p - k) / up = p / up - j for the
// j-th tap of phase k0, so a lane walks DOWN its input from i0 = p / up and ALONG row k0 of the table laid out [phase][tap].
#pragma once
#include "lsm_common.h"

namespace lsm_resample {

constexpr int THREADS = 512;                 // 8 waves: with a table over 80 KB one workgroup owns a CU
constexpr int PER_THREAD = 4;
constexpr int TILE = THREADS * PER_THREAD;   // output samples of a workgroup
constexpr long LDS_MAX = 160 * 1024;         // a CU's LDS

// taps of phase k0: the k = k0 + j * up below K
__host__ __device__ inline int phase_taps(int n_taps, int up, int k0) { return (n_taps - k0 + up - 1) / up; }
// Row stride of the LDS table in doubles: the longest row, made odd.  Neighbouring lanes sit (down mod up) phases apart;
// with an odd stride the 32 lanes of a ds_read_b64 group spread over the 32 bank pairs whenever that step is odd too
// (441 at 44.1, 22.05 and 11.025 kHz); with up <= 2 a wave reads one or two addresses, which broadcast.
__host__ __device__ inline int row_stride(int n_taps, int up) { return phase_taps(n_taps, up, 0) | 1; }
__host__ __device__ inline long table_bytes(int n_taps, int up) { return (long)up * row_stride(n_taps, up) * 8; }
// Hs = (K - 1) / up input samples of history: the reach of the longest row behind i0
__host__ __device__ inline int history_samples(int n_taps, int up) { return (n_taps - 1) / up; }
// Samples of a clip of n (>= 0) on a design (up, down) in a row of n_out (SPEC.md §1.18): min(ceil(n * up / down), n_out).
// One copy for the ragged speed kernel and for the host export that tells Python the same integer.
__host__ __device__ inline int ragged_length(int n, int up, int down, int n_out)
{
    const long long whole = ((long long)n * up + down - 1) / down;
    return whole < n_out ? (int)whole : n_out;
}

// hp (n_taps doubles, global memory, natural order) -> tab[k % up][k / up], by the whole workgroup; ends with a barrier
__device__ __forceinline__ void load_table(double *tab, const double *__restrict__ taps, int n_taps, int up)
{
    const int stride = row_stride(n_taps, up);
    for (int k = threadIdx.x; k < n_taps; k += THREADS) tab[(k % up) * stride + k / up] = taps[k];
    __syncthreads();
}

// z[m] for p = m * down given as i0 = p / up and k0 = p mod up.  `sample(i)` is x[i] widened to float64, +0.0 outside the
// signal: such a sample goes through the multiply and the add like any other, so a NaN tap product is formed on both sides
// of a cut alike and the signed zeros agree.
template <typename Sample>
__device__ __forceinline__ float causal_sample(const double *tab, int n_taps, int up, long long i0, int k0, Sample sample)
{
    const double *row = tab + (size_t)k0 * row_stride(n_taps, up);
    const int n = phase_taps(n_taps, up, k0);
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc = acc + row[j] * sample(i0 - j);
    return (float)acc;
}

// One PCM sample as float32: format 0 is float32, format 1 int16 scaled by 2^-15 (exact)
__device__ __forceinline__ float pcm_f32(const void *__restrict__ base, size_t i, int fmt)
{
    return fmt ? (float)static_cast<const int16_t *>(base)[i] * (1.0f / 32768.0f) : static_cast<const float *>(base)[i];
}

}  // namespace lsm_resample
