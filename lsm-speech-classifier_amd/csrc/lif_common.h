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
// LIM (ST forms, SPEC.md §4c): only the steps t < Tb of every channel row are packed -- a dword that straddles Tb loses its
// bytes at t >= Tb, a byte at t >= Tb is skipped -- and only the rows below Tb need to be zero.  T stays the row stride.
template <int NT, bool PERM, bool LIM = false>
__device__ __forceinline__ void pack_raster_bits(const uint8_t *raster, const uint8_t *inperm, int b, int C, int T, int CW,
                                                 uint32_t *bits, int tid, int Tb = 0)
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
            if (LIM && t0 >= Tb) continue;
            const int pc = PERM ? (int)inperm[c] : c;        // the channel's place in the bit row
            const uint32_t bit = 1u << (pc & 31);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((v >> (8 * k)) & 0xFFu) && (!LIM || t0 + k < Tb)) atomicOr(&bits[(t0 + k) * CW + (pc >> 5)], bit);
        }
    } else {
        const int nb = C * T;
        for (int q = tid; q < nb; q += NT)
            if (clip[q]) {
                const int c = q / T;
                if (LIM && q - c * T >= Tb) continue;
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

// ---- continuation (SPEC.md §4a, include/lsm_hip.h: lsm_reservoir_run_from) ----------------------------------------------
// One block per clip, the same for every kernel and layout, all zeros = reset():
//   uint32 header[4] {spikes of the whole reservoir so far, 0, 0, 0} | float v[NP] | uint16 ref[NP] |
//   uint32 last_spikes[NP/32] | uint32 ever_fired[NP/32] | uint4 feat[n_out],     NP = N rounded up to 64.
// The ST forms of the kernels (template parameter, off in every stateless form) convert it into their own registers and
// step lists in the prologue and back in the epilogue; the step loops run on local times 0 .. T-1 either way.
struct StateArgs {
    const unsigned char *in;   // (B, stride) state after step t0-1, or null: reset
    unsigned char *out;        // (B, stride) receives the state after step t0+T-1, or null; may be `in`
    long stride;               // bytes per clip: state_bytes(N, n_out)
    int t0;                    // steps done before this launch
    int seg;                   // SPEC.md §4b: steps per segment (divides T), 0 = the launch is not segmented
    uint4 *rec;                // seg > 0: (B, T / seg, n_out) segment records
    const int *steps;          // SPEC.md §4c: (B) steps every clip runs in this launch (clamped into [0, T]), or null: T
    // SPEC.md §4d, stream launch (seg > 0): t0 is STREAM_T0 -- no cumulative record is kept, the feat block of `in` is not
    // read and that of `out` is written as zeros --, and `steps` counts whole segments: clip b runs
    // clamp(steps[b], 0, count_limit) * count_steps steps.  Every other launch: count_limit = T, count_steps = 1.
    int count_limit, count_steps;
};
constexpr int STREAM_T0 = -1;          // StateArgs::t0 of a stream launch: it has no position (every real first step is >= 0)

// count_limit and count_steps of the launch, read from the kernel-argument segment through a pointer the optimiser cannot see
// through (st_offset: offsetof(<the kernel's argument struct>, st), as state_pass_through below): scalar loads of the
// prologue that are not merged with the other loads of a.st and do not stay live across the step loop.
__device__ __forceinline__ int2 state_count_scale(size_t st_offset)
{
    typedef __attribute__((address_space(4))) const unsigned char *karg_t;
    karg_t ka = (karg_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    ka += st_offset;
    return make_int2(*reinterpret_cast<__attribute__((address_space(4))) const int *>(ka + offsetof(StateArgs, count_limit)),
                     *reinterpret_cast<__attribute__((address_space(4))) const int *>(ka + offsetof(StateArgs, count_steps)));
}

// SPEC.md §4c: the steps clip b runs in a launch of T (Tb).  b is workgroup-uniform, so this is one scalar load; T stays the
// row stride of the raster, the spike matrix and the trace and the size of the LDS image.
// Stream launch (SPEC.md §4d): the count is in whole segments, clamped into [0, T / seg]; Tb is a multiple of seg, so the
// clip's last step closes its last record and no clip ends inside a segment.
// The same value in two forms, because the ST kernels' register allocation follows the form (profiles/stream_segments.txt:
// with either form alone some kernels gain scratch or lose a wave per SIMD, with each kernel on its form none does):
//   clip_step_count           the §4c count, then min(., count_limit) * count_steps, the two scale fields read apart from a.st
//                             (lif_ring.h, lif_pair.h, lif_dense.h but for INMODE 1);
//   clip_step_count_unscaled  the §4c count alone, and behind the zero-step exit stream_step_scale: a count n > 0 of whole
//                             segments becomes min(n * seg, T) steps (lif_kernel.h, lif_dense.h with INMODE 1).  n <= T <=
//                             65535 and seg <= 65535, so the product stays below 2^32: the compare is unsigned.
__device__ __forceinline__ int clip_step_count_unscaled(const StateArgs &st, int b, int T)
{
    return st.steps ? min(max(st.steps[b], 0), T) : T;
}

__device__ __forceinline__ int clip_step_count(const StateArgs &st, int b, int T, size_t st_offset)
{
    const int n = clip_step_count_unscaled(st, b, T);
    const int2 scale = state_count_scale(st_offset);         // {T, 1}, stream launch {T / seg, seg}
    return min(n, scale.x) * scale.y;
}

__device__ __forceinline__ int stream_step_scale(const StateArgs &st, int n, int T)
{
    return st.t0 == STREAM_T0 ? (int)min((uint32_t)n * (uint32_t)st.seg, (uint32_t)T) : n;
}

// A clip of zero steps (SPEC.md §4c): its state block passes through -- out receives in byte for byte (zeros without in;
// nothing when they are the same block), 16 bytes per move (the stride and both bases are multiples of 16) -- and nothing
// else of the clip is touched.  Called before the first barrier and before any LDS write, under a workgroup-uniform test;
// the workgroup returns behind it.
// st_offset: offsetof(<the kernel's argument struct>, st).  The block reads StateArgs from the kernel-argument segment (the
// argument struct is the kernel's only parameter: offset 0) through a pointer the optimiser cannot see through, NOT as
// `a.st`: loads of a.st.in / out / stride at the top of the kernel are merged with those of the state prologue and epilogue
// and stay live across the step loop -- lif_dense_kernel<2, 1, 0, false, true> then took 101 registers for 81 (4 waves per
// SIMD for 5), <16, 16, 0, false, true> 100 bytes of scratch for 84 (profiles/ragged_batches.txt).
template <int NT>
__device__ __forceinline__ void state_pass_through(int b, int tid, size_t st_offset)
{
    typedef __attribute__((address_space(4))) const unsigned char *karg_t;
    karg_t ka = (karg_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    ka += st_offset;
    typedef const unsigned char *in_t;
    typedef unsigned char *out_t;
    const in_t in = *reinterpret_cast<__attribute__((address_space(4))) const in_t *>(ka + offsetof(StateArgs, in));
    const out_t out = *reinterpret_cast<__attribute__((address_space(4))) const out_t *>(ka + offsetof(StateArgs, out));
    const long stride = *reinterpret_cast<__attribute__((address_space(4))) const long *>(ka + offsetof(StateArgs, stride));
    if (!out || out == in) return;
    const size_t off = (size_t)b * stride;
    uint4 *dst = reinterpret_cast<uint4 *>(out + off);
    const uint4 *src = in ? reinterpret_cast<const uint4 *>(in + off) : nullptr;
    const int n16 = (int)(stride >> 4);
    for (int i = tid; i < n16; i += NT) dst[i] = src ? src[i] : make_uint4(0u, 0u, 0u, 0u);
}

__host__ __device__ inline int state_np(int N) { return (N + 63) & ~63; }
__host__ __device__ inline long state_off_v() { return 16; }
__host__ __device__ inline long state_off_ref(int NP) { return 16 + 4L * NP; }
__host__ __device__ inline long state_off_last(int NP) { return 16 + 6L * NP; }
__host__ __device__ inline long state_off_ever(int NP) { return 16 + 6L * NP + NP / 8; }
__host__ __device__ inline long state_off_feat(int NP) { return 16 + 6L * NP + NP / 4; }
__host__ __device__ inline long state_bytes(int N, int n_out) { return state_off_feat(state_np(N)) + 16L * n_out; }

// Words of LDS scratch the ST epilogue needs (last-step bits, ever-fired bits, one spike total); every kernel has an idle
// accumulator array of at least its padded neuron count in words behind the last step.
__host__ __device__ inline int state_scratch_words(int NP) { return NP / 16 + 1; }

// Prologue: neuron i (< N) of the clip whose block starts at `sin`.
__device__ __forceinline__ void state_load_neuron(const unsigned char *sin, int NP, int i, float *v, uint32_t *ref, bool *last,
                                                  bool *ever)
{
    *v = reinterpret_cast<const float *>(sin + state_off_v())[i];
    *ref = reinterpret_cast<const uint16_t *>(sin + state_off_ref(NP))[i];
    *last = (reinterpret_cast<const uint32_t *>(sin + state_off_last(NP))[i >> 5] >> (i & 31)) & 1u;
    *ever = (reinterpret_cast<const uint32_t *>(sin + state_off_ever(NP))[i >> 5] >> (i & 31)) & 1u;
}

__device__ __forceinline__ uint32_t state_load_total(const unsigned char *sin) { return *reinterpret_cast<const uint32_t *>(sin); }

// Epilogue, between state_begin and state_finish: neuron i (< NP; a padding neuron N <= i stores zeros) and the neurons
// of the last step's spike lists.
__device__ __forceinline__ void state_store_neuron(unsigned char *sout, uint32_t *scratch, int NP, int N, int i, float v,
                                                   uint32_t ref, bool ever)
{
    if (i >= NP) return;
    const bool real = i < N;
    if (sout) {
        reinterpret_cast<float *>(sout + state_off_v())[i] = real ? v : 0.0f;
        reinterpret_cast<uint16_t *>(sout + state_off_ref(NP))[i] = (uint16_t)(real ? ref : 0u);
    }
    if (real && ever) atomicOr(&scratch[NP / 32 + (i >> 5)], 1u << (i & 31));
}
__device__ __forceinline__ void state_mark_last(uint32_t *scratch, int j) { atomicOr(&scratch[j >> 5], 1u << (j & 31)); }

// Epilogue, first: the scratch words start at zero.  Contains a barrier.
template <int NT>
__device__ __forceinline__ void state_begin(uint32_t *scratch, int NP, int tid)
{
    for (int i = tid; i < state_scratch_words(NP); i += NT) scratch[i] = 0u;
    __syncthreads();
}

// SPEC.md §4a: the record of [0, t0) and the record of this launch's steps on local times make the record of [0, t0 + n).
__device__ __forceinline__ uint4 merge_feature_records(uint4 f1, uint4 f2, uint32_t t0, int burst_isi_max)
{
    const uint32_t n1 = f1.x & 0xFFFFu, b1 = f1.x >> 16, n2 = f2.x & 0xFFFFu, b2 = f2.x >> 16;
    if (n2 == 0u) return f1;
    const uint32_t first2 = (f2.y & 0xFFFFu) + t0, last2 = (f2.y >> 16) + t0;
    uint4 m;
    m.z = f1.z + f2.z + n2 * t0;
    if (n1 == 0u) {
        m.x = n2 | (b2 << 16);
        m.y = first2 | (last2 << 16);
        m.w = f2.w;
        return m;
    }
    const uint32_t first1 = f1.y & 0xFFFFu, last1 = f1.y >> 16;
    const uint32_t isi = first2 - last1;                 // the interval that straddles the cut
    m.x = (n1 + n2) | ((b1 + b2 + ((int)isi <= burst_isi_max ? 1u : 0u)) << 16);
    m.y = first1 | (last2 << 16);
    m.w = f1.w + f2.w + isi * isi;
    return m;
}

// ---- segments (SPEC.md §4b, include/lsm_hip.h: lsm_reservoir_run_segments; ST forms with StateArgs::seg > 0) ------------
// The step loops keep their records on launch-local times.  After the update of the last step of a segment the lane that
// owns an output neuron -- the only writer of its record -- closes it: rebased to the segment's own times, stored, zeroed.
// No barrier is involved: the next write of the record is the same lane's.
struct SegmentCursor {
    uint4 *rec;                // records of the open segment of this clip
    uint32_t t_begin;          // its first step (launch-local)
    uint32_t t_end;            // the step after its last; 0 = not segmented (no step t has t + 1 == 0)
};

__device__ __forceinline__ SegmentCursor segment_cursor(const StateArgs &st, int b, int T, int n_out)
{
    SegmentCursor c;
    c.rec = st.seg > 0 ? st.rec + (size_t)b * (size_t)(T / st.seg) * (size_t)n_out : nullptr;
    c.t_begin = 0u;
    c.t_end = st.seg > 0 ? (uint32_t)st.seg : 0u;
    return c;
}

// Workgroup-uniform: step t was the last of the open segment.
__device__ __forceinline__ bool segment_ends(const SegmentCursor &c, int t) { return (uint32_t)(t + 1) == c.t_end; }

// The record of output slot o over the open segment, on segment-local times: first and last lose t_begin, S1 loses
// n * t_begin; the intervals (Q, bursts) do not depend on the origin.  An empty record stays all zeros.
__device__ __forceinline__ void segment_close(const SegmentCursor &c, int o, uint4 f)
{
    const uint32_t n = f.x & 0xFFFFu;
    if (n != 0u) {
        f.y -= c.t_begin | (c.t_begin << 16);
        f.z -= n * c.t_begin;
    }
    c.rec[o] = f;
}

// The LDS-held record of output slot o (-1: the neuron is no output neuron): closed and zeroed by its owner.  The callers
// read the slots of their neurons again from the layout's table, in a loop that is not unrolled: a segment end is rare,
// and the step loop's registers stay what they are.
__device__ __forceinline__ void segment_close_lds(const SegmentCursor &c, uint4 *feat, int o)
{
    if (o >= 0) {
        segment_close(c, o, feat[o]);
        feat[o] = make_uint4(0, 0, 0, 0);
    }
}

__device__ __forceinline__ void segment_next(SegmentCursor *c, int seg, int n_out)
{
    c->rec += n_out;
    c->t_begin = c->t_end;
    c->t_end += (uint32_t)seg;
}

// Epilogue, before state_finish and behind a barrier that follows the last close: the launch-wide record of every output
// neuron is the left fold of §4a's merge over the clip's own segment records, read back from the records buffer (the
// workgroup's own stores, ordered by that barrier) -- no second LDS record array.
// (The kernels pass their Tb for T: a segmented launch that keeps a cumulative record is never ragged, so Tb == T, and T
// need not outlive the step loop.  The ragged segmented launch is the stream launch of SPEC.md §4d, which keeps no cumulative
// record and skips this fold: nothing reads its records back.)
template <int NT>
__device__ __forceinline__ void segment_fold(const StateArgs &st, int b, int T, uint4 *feat, int n_out, int burst_isi_max, int tid)
{
    const int G = T / st.seg;
    const uint4 *rec = st.rec + (size_t)b * (size_t)G * (size_t)n_out;
    for (int o = tid; o < n_out; o += NT) {
        uint4 f = make_uint4(0, 0, 0, 0);
        for (int g = 0; g < G; ++g)
            f = merge_feature_records(f, rec[(size_t)g * n_out + o], (uint32_t)(g * st.seg), burst_isi_max);
        feat[o] = f;
    }
}

// Epilogue, last: every wave has stored its neurons and added its spikes to the total (lane 0, state_add_total).  Writes the
// bit fields and the header, merges the feature records (LDS `feat` holds this launch's on entry and the whole run's on
// return, as does the state).  Contains barriers; `in` and `out` may be the same block: every word is read before it is
// written, by the same thread.
// Stream launch (t0 == STREAM_T0, SPEC.md §4d): no cumulative record exists -- nothing is merged, the feat block of `sin` is
// not read, and that of `sout` (and LDS `feat`, which nobody reads: the launch has no feature keys) receives zeros.
__device__ __forceinline__ void state_add_total(uint32_t *scratch, int NP, uint32_t tot_spk) { atomicAdd(&scratch[NP / 16], tot_spk); }

template <int NT>
__device__ __forceinline__ void state_finish(const unsigned char *sin, unsigned char *sout, uint32_t *scratch, uint4 *feat,
                                             int NP, int n_out, uint32_t t0, int burst_isi_max, int tid)
{
    __syncthreads();
    if (sout) {
        uint32_t *bitsout = reinterpret_cast<uint32_t *>(sout + state_off_last(NP));      // last, then ever: NP/16 words
        for (int i = tid; i < NP / 16; i += NT) bitsout[i] = scratch[i];
        if (tid == 0) *reinterpret_cast<uint4 *>(sout) = make_uint4(scratch[NP / 16], 0u, 0u, 0u);
    }
    for (int o = tid; o < n_out; o += NT) {
        uint4 f = feat[o];
        if ((int)t0 == STREAM_T0) f = make_uint4(0u, 0u, 0u, 0u);
        else if (sin) f = merge_feature_records(reinterpret_cast<const uint4 *>(sin + state_off_feat(NP))[o], f, t0, burst_isi_max);
        feat[o] = f;
        if (sout) reinterpret_cast<uint4 *>(sout + state_off_feat(NP))[o] = f;
    }
    __syncthreads();
}

}  // namespace lsm_lif
