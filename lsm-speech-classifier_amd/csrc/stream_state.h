// stream_state.h -- what every streamed kernel does with its per-stream state block (DESIGN.md "The state block"): where
// a stream's block lies, how much of the launch a stream takes part in, what travels when state_out is not state_in, and
// the shift of a history of samples.  Small force-inlined pieces; a kernel keeps its own layout of the bytes in use.
#pragma once
#include "lsm_common.h"

namespace lsm_state {

// a block is its bytes in use rounded up to a multiple of 16
__host__ __device__ inline size_t state_round16(size_t used) { return (used + 15) & ~(size_t)15; }

// values[b] held inside [lo, hi]; `absent` where the caller gave no array
__device__ __forceinline__ int clamped_at(const int32_t *values, int b, int lo, int hi, int absent)
{
    return min(max(values ? values[b] : absent, lo), hi);
}

// how many of the launch's H hops, columns or blocks stream b delivers: all of them without a count array
__device__ __forceinline__ int stream_count(const int32_t *counts, int b, int H) { return clamped_at(counts, b, 0, H, H); }

// One stream's block.  sin null: a fresh stream, all zeros.  sout null: no state is written.  copy: out of place, so what
// the kernel does not rewrite -- an idle stream's whole block, the padding of the others -- has to travel.
struct StateBlock {
    const unsigned char *sin;
    unsigned char *sout;
    bool copy;
};

__device__ __forceinline__ StateBlock state_block(const unsigned char *state_in, unsigned char *state_out, size_t b,
                                                  size_t block_bytes)
{
    StateBlock blk;
    blk.sin = state_in ? state_in + b * block_bytes : nullptr;
    blk.sout = state_out ? state_out + b * block_bytes : nullptr;
    blk.copy = blk.sout != nullptr && blk.sout != blk.sin;
    return blk;
}

// out of place, the block's words from `first` on travel as they are: zeros where there is no state_in
template <int THREADS>
__device__ __forceinline__ void carry_words(const StateBlock &blk, size_t first, size_t block_bytes, int tid)
{
    const uint32_t *win = reinterpret_cast<const uint32_t *>(blk.sin);
    uint32_t *wout = reinterpret_cast<uint32_t *>(blk.sout);
    if (blk.copy)
        for (size_t i = first + tid; i < block_bytes / 4; i += THREADS) wout[i] = win ? win[i] : 0u;
}

// an idle stream (count 0): its block travels as it is (out of place), or stays (in place)
template <int THREADS>
__device__ __forceinline__ void carry_idle_block(const StateBlock &blk, size_t block_bytes, int tid)
{
    carry_words<THREADS>(blk, 0, block_bytes, tid);
}

// Out of place the padding travels too.  Where the bytes in use are not whole words it goes in units of U from unit
// `first` on, one step of the calling threads: it is shorter than 16 bytes.  (A block of whole words: carry_words.)
template <typename U>
__device__ __forceinline__ void carry_padding(const StateBlock &blk, size_t first, size_t block_bytes, int tid)
{
    const U *pin = reinterpret_cast<const U *>(blk.sin);
    U *pout = reinterpret_cast<U *>(blk.sout);
    if (blk.copy && first + tid < block_bytes / sizeof(U)) pout[first + tid] = pin ? pin[first + tid] : (U)0;
}

// The last Hs entries of [old history of Hs | adv new entries]: new[j] = old[j + adv], an index from Hs on read from the
// push (`new_at(i)`, i >= 0), one below it from the old history (`old_at(j)`), and handed to `put(j, v)`.
// Why state_out may be state_in: chunks of THREADS entries go in ascending order and each is read whole, by every thread,
// before the barrier and stored behind it.  A chunk reads at or above its own indices (adv >= 0), hence strictly above
// every chunk stored before it, so a push shorter than the history shifts within the block without losing an entry.
// Every thread of the workgroup calls it (the barrier), with adv >= 0.
template <int THREADS, typename Adv, typename Old, typename New, typename Put>
__device__ __forceinline__ void shift_history(int Hs, Adv adv, int tid, Old old_at, New new_at, Put put)
{
    const long long hs = Hs;
    for (int base = 0; base < Hs; base += THREADS) {
        const int j = base + tid;
        decltype(old_at(0LL)) v{};
        if (j < Hs) {
            const long long src = (long long)j + adv;
            if (src >= hs) v = new_at(src - hs);
            else v = old_at(src);
        }
        __syncthreads();
        if (j < Hs) put(j, v);
    }
}

}  // namespace lsm_state
