// Noise mixer (SPEC.md §1.10): what the kernels of mix.hip share -- the one copy of "sample i of the shifted, scaled clip", of
// "sample i of the mixed signal", of the walk round a noise row and of the row power P.
//
// Everything is float64 without FMA (the translation unit is compiled with -ffp-contract=off): a product is rounded, then
// the sum is rounded.  A float32 sample times a float32 scale is exact in float64.
#pragma once
#include "lsm_common.h"

namespace lsm_mix {

constexpr int THREADS = 256;                 // the 256 partial sums of P, one per thread
constexpr int MAX_SAMPLES = 1 << 24;         // samples of a row: i, o + i and p + i stay below 2^32

// (o + i) mod L for 0 <= o < L <= 2^31 - 1 and 0 <= i <= 2^24: the sum fits 32 unsigned bits
__device__ __forceinline__ uint32_t noise_index(uint32_t o, uint32_t i, uint32_t L) { return (o + i) % L; }
// the index one sample on
__device__ __forceinline__ uint32_t noise_next(uint32_t idx, uint32_t L) { return idx + 1 == L ? 0u : idx + 1; }
// v mod L, non-negative, for any int32 v
__device__ __forceinline__ uint32_t mod_nonneg(int v, int L)
{
    const int m = v % L;
    return (uint32_t)(m < 0 ? m + L : m);
}

// x[i] = a * row[i - s] where 0 <= i - s < n, else +0.0: read at a clamped index and keep or drop the value (no guarded load)
__device__ __forceinline__ double shifted_sample(const float *row, int n, int s, double a, int i)
{
    const int j = i - s;
    const float u = row[min(max(j, 0), n - 1)];
    return (j >= 0 && j < n) ? a * (double)u : 0.0;
}

// Sample i of the mixed signal.  `noisy` false: the noise value never reaches the result (and is not read by the callers).
__device__ __forceinline__ float mixed_sample(double x, bool noisy, double g, double v)
{
    return noisy ? (float)(x + g * v) : (float)x;
}

// The tree of P over the 256 partial sums in LDS: p[l] = p[l] + p[l+s] for s = 128, ..., 1; the result for every thread.
// `p` holds `rows` arrays of THREADS doubles, reduced side by side.  Ends with a barrier.
template <int rows>
__device__ __forceinline__ void power_tree(double (*p)[THREADS], const double (&mine)[rows])
{
    const int l = threadIdx.x;
#pragma unroll
    for (int r = 0; r < rows; ++r) p[r][l] = mine[r];
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s >= 1; s >>= 1) {
        if (l < s) {
#pragma unroll
            for (int r = 0; r < rows; ++r) p[r][l] = p[r][l] + p[r][l + s];
        }
        __syncthreads();
    }
}

// Rows of 16-byte stores where the row's address allows: out[i] = y(i) for i in [0, n), the whole workgroup.  `y4(i, q)`
// gives the four samples i .. i + 3; `y(i)` one.  A head of up to three samples brings the stores to a 16-byte boundary.
template <typename One, typename Four>
__device__ __forceinline__ void store_row(float *out, int n, One y, Four y4)
{
    const int head = min(n, (int)(((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) >> 2));
    const int quads = (n - head) >> 2;
    const int tid = threadIdx.x;
    if (tid < head) out[tid] = y(tid);
    for (int q = tid; q < quads; q += THREADS) {
        const int i = head + 4 * q;
        float4 v;
        y4(i, v);
        *reinterpret_cast<float4 *>(out + i) = v;
    }
    const int i = head + 4 * quads + tid;
    if (i < n) out[i] = y(i);
}

// out[i] = +0.0 for i in [0, n): store_row's head, 16-byte stores and tail on a row that starts anywhere (n may be 0)
__device__ __forceinline__ void fill_row(float *out, int n)
{
    store_row(out, n, [](const int) { return 0.0f; }, [](const int, float4 &y) { y = make_float4(0.0f, 0.0f, 0.0f, 0.0f); });
}

}  // namespace lsm_mix
