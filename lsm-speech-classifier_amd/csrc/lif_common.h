// lif_common.h -- what the four reservoir kernels (lif_kernel.h, lif_dense.h, lif_ring.h, lif_pair.h) share: the
// prologue that bit-packs a clip's raster, the statistics and SPEC.md §4 feature epilogues, and two wave-level helpers.
// Everything is inlined into the kernels; barriers stay where the kernels put them, except the one inside write_stats.
#pragma once
#include "lsm_common.h"

namespace lsm_lif {

constexpr int IN_REG_SLOTS = 6;       // input-map entries per lane kept in registers (lif_kernel.h, lif_dense.h)

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int lane_rank(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Prologue: the feature accumulators (n_out) and the clip's input bit image (T * CW words) start at zero.  The caller's
// barrier separates this from pack_raster_bits.
template <int NT>
__device__ __forceinline__ void zero_features_and_bits(uint4 *feat, int n_out, uint32_t *bits, int n_words, int tid)
{
    for (int i = tid; i < n_out; i += NT) feat[i] = make_uint4(0, 0, 0, 0);
    for (int i = tid; i < n_words; i += NT) bits[i] = 0u;
}

// Prologue: bit-pack clip b of the (B, C, T) uint8 raster time-major into `bits` (T rows of CW words, zeroed before):
// bit p of row t = channel c spikes at step t, p = inperm[c] (PERM: the coloured positions chosen by the host) or c.
// Four steps per load when a channel's T bytes are whole dwords.
template <int NT, bool PERM>
__device__ __forceinline__ void pack_raster_bits(const uint8_t *raster, const uint8_t *inperm, int b, int C, int T, int CW,
                                                 uint32_t *bits, int tid)
{
    const uint8_t *clip = raster + (size_t)b * C * T;
    if ((T & 3) == 0) {
        const uint32_t *clip4 = reinterpret_cast<const uint32_t *>(clip);
        const int nd = C * T / 4;
        for (int q = tid; q < nd; q += NT) {
            const uint32_t v = clip4[q];
            if (v == 0) continue;
            const int c = (q * 4) / T;
            const int t0 = (q * 4) - c * T;
            const int pc = PERM ? (int)inperm[c] : c;        // the channel's place in the bit row
            const uint32_t bit = 1u << (pc & 31);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((v >> (8 * k)) & 0xFFu) atomicOr(&bits[(t0 + k) * CW + (pc >> 5)], bit);
        }
    } else {
        const int nb = C * T;
        for (int q = tid; q < nb; q += NT)
            if (clip[q]) {
                const int c = q / T;
                const int pc = PERM ? (int)inperm[c] : c;
                atomicOr(&bits[(q - c * T) * CW + (pc >> 5)], 1u << (pc & 31));
            }
    }
}

// Epilogue: health statistics of clip b, {neurons that fired at least once, spikes of the whole reservoir}, summed over the
// workgroup in two LDS words that are zero on entry.  hf: one bit per neuron of the lane that fired; tot_spk: spikes of the
// lane's wave.  Contains a barrier: every thread calls it, under the uniform test of `stats`.
__device__ __forceinline__ void write_stats(int32_t *stats, int b, uint32_t *fired, uint32_t *spikes, uint32_t hf,
                                            uint32_t tot_spk, int lane, int tid)
{
    atomicAdd(fired, (uint32_t)__popc(hf));
    if (lane == 0) atomicAdd(spikes, tot_spk);
    __syncthreads();
    if (tid == 0) {
        stats[2 * b] = (int32_t)*fired;
        stats[2 * b + 1] = (int32_t)*spikes;
    }
}

// SPEC.md §4: one feature of an output neuron from its exact integers (n spikes, first / last spike time, S1 = sum of the
// spike times, Q = sum of the squared inter-spike intervals, bursts), evaluated in float64 and rounded to float32.
__device__ __forceinline__ float feature_value(int key, int n, int bursts, int first, int last, uint32_t s1, uint32_t q2, int T)
{
    double val = 0.0;
    switch (key) {
    case 0: val = (double)n; break;
    case 1: { const double p = (double)n / (double)T; val = p * (1.0 - p); } break;
    case 2: val = n >= 1 ? (double)s1 / (double)n : 0.0; break;
    case 3: val = n >= 1 ? (double)first : 0.0; break;
    case 4: val = n >= 1 ? (double)last : 0.0; break;
    case 5: val = n >= 2 ? (double)(last - first) / (double)(n - 1) : 0.0; break;
    case 6:
        if (n >= 2) {
            const double m = (double)(last - first) / (double)(n - 1);
            val = (double)q2 / (double)(n - 1) - m * m;
        }
        break;
    default: val = (double)bursts; break;
    }
    return (float)val;
}

// Epilogue: the (n_keys * n_out) features of clip b from the integer accumulators feat[o] = {n | bursts << 16,
// first | last << 16, S1, Q}, key-major.
template <int NT>
__device__ __forceinline__ void write_features(float *features, const uint4 *feat, const int *key_ids, int n_keys, int n_out,
                                               int b, int T, int tid)
{
    const int nf = n_keys * n_out;
    for (int idx = tid; idx < nf; idx += NT) {
        const int kq = idx / n_out;
        const int o = idx - kq * n_out;
        const uint4 f = feat[o];
        const int n = (int)(f.x & 0xFFFFu), bursts = (int)(f.x >> 16);
        const int first = (int)(f.y & 0xFFFFu), last = (int)(f.y >> 16);
        features[(size_t)b * nf + idx] = feature_value(key_ids[kq], n, bursts, first, last, f.z, f.w, T);
    }
}

}  // namespace lsm_lif
