// lif_dense.h -- LIF reservoir time loop on dense presynaptic rows (N <= 8192), gfx950.
//
// Same contract as lif_kernel.h (SPEC.md §3-§4; replaces reset/set_input_spike_times/simulate/
// extract_features_from_spikes of /root/reference/extract_lsm_features.py:79-83), different data
// structure: W is stored as dense rows by PRESYNAPTIC neuron, Wt[j][i] (0 where there is no synapse),
// N x LD floats: 4 MB at N = 1000 (L2 resident), 64 MB at N = 4000 (Infinity Cache), 262 MB at N = 8000.  For every neuron j that spiked
// at t-1, ascending, each lane loads the weight onto ITS OWN target neuron (one coalesced 256-byte load
// per wave and 64-neuron slot) and adds it to a REGISTER accumulator.  The oracle's per-target sum runs
// over the existing synapses in ascending j; the extra terms here are exact zeros and x + 0 = x in
// float32, so the result is bit-identical.  What this removes compared with the sparse kernel: the LDS
// current accumulators and their ordered read-modify-write chain (a burst of n spikes cost n dependent LDS
// round trips on the few waves owning the targets), the segment tables, the exec masking -- every wave does
// the same S loads + S adds, so bursts no longer unbalance the waves.  What it costs: N*4 bytes per spiking
// neuron and clip from L2/MALL instead of ~8 bytes per synapse (4 KB vs 1.6 KB at N = 1000).
//
// Spike exchange: each producer wave writes its spiking neurons (ballot + mbcnt ranks, ascending) into its
// own LDS list; the first R = 64/WPC also go to the wave's fixed region of a 64-entry step list, so lane l of
// a consumer knows its entry (l) and whether it is filled (l%R < count of producer l/R) without any merge;
// when a producer has more than R spikes (its count says so) the consumers merge the per-wave lists for that
// step instead (scalar prefix over the counts + compare chain).
#pragma once
#include "lif_common.h"

struct lsm_reservoir;       // the reservoir handle (reservoir.hip)

// Row fetch, same-box A/B at 128 filters / 1000 neurons / 256 clips (profiles/r02_dense_row_chain_ab.txt): global loads.
// MUBUF `buffer_load ... offen` with the row offset as scalar operand (no per-row vector address add) took 0.60 ms
// instead of 0.53: with eight waves of a CU issuing dword gathers, buffer loads run at 3/4 of the rate of global loads
// (exp/ubench_vmem.hip, profiles/r02_ubench_global_vs_buffer_loads.txt).  The consumed list bit is cleared with one
// s_bitset0_b64 instead of the three-instruction `todo &= todo - 1`; with the row offsets premultiplied once per 64
// entries a row costs 9 instructions per wave instead of 12 (0.532 -> 0.519 ms).
namespace lsm_lif {

struct DenseArgs {
    int N, C, T, B;
    int n_out, CW, EinW, refractory, burst_isi_max, ld;
    float theta, w_in;
    const uint8_t *raster;     // (B, C, T) uint8
    const float *wt;           // (N, ld) dense rows by presynaptic neuron
    const float *leak;         // (NPAD)
    const int *oslot;          // (NPAD) output slot or -1
    const uint32_t *in_ent;    // (WPC, EinW) (channel << 16) | target, 0xFFFFFFFF = padding
    const uint32_t *inmask;    // (NPAD, 4) input-channel bit mask per neuron (INMODE 2, 3: C <= 128), or null
    const uint8_t *inperm;     // (C) bit position of channel c in the input bit row (INMODE 3), or null (position c)
    int n_keys;
    int key_ids[8];
    float *features;           // (B, n_keys * n_out)
    uint8_t *spike_matrix;     // (B, T, N) or null
    float *v_trace;            // (B, T, N) or null
    int32_t *stats;            // (B, 2) {neurons that fired at least once, spikes of the whole reservoir} or null
    const int32_t *order;      // (B) clip of workgroup g, or null (g): lsm_reservoir_run_ordered starts long clips first
    StateArgs st;              // ST forms only (lsm_reservoir_run_from)
};

// INMODE: how the input drive m_i(t) = #{active channels feeding neuron i} is formed.
//   0  the wave's (channel, target) entries are streamed from global memory, integer LDS atomics count
//   1  the entries sit in registers (<= IN_REG_SLOTS*64 per wave), integer LDS atomics count
//   2  every neuron holds the bit mask of its input channels in registers (C <= 128, SL <= 4) and counts
//      popcount(mask & row) against the step's wave-uniform input bit row: no atomics, no count array,
//      and nothing to wait for between the recurrent rows and the update
//   3  as 2, with the channels' bit positions permuted (DenseArgs::inperm, chosen by the host) so that the channels
//      feeding one neuron differ in their position mod 32: the four masked words of a neuron are disjoint and ONE
//      popcount of their union counts them -- 5 vector instructions per neuron and step instead of 9
// (Ring-like reservoirs whose dense table no longer fits the caches run on lif_ring.h instead: window + list rows.)
// REFM: the refractory countdown of the reference's period (REFRACTORY_PERIOD = 2, extract_lsm_features.py:13) lives in
// SCALAR registers -- two 64-bit lane masks per slot, h2 = "fired at the last step" and h1 = "fired the step before" --
// instead of one vector register per neuron.  The fire condition comes out of v_cmp as a lane mask, `held` = h1 | h2
// and the countdown (h1 <- h2, h2 <- fire) are scalar mask moves, the potential's reset is ONE v_cndmask on the mask,
// and the fire path takes the masks as execution masks: per neuron and step 2 vector instructions for threshold /
// reset / refractory instead of ~9 (three compares, the boolean materialised and compared again for the ballot, two
// selects, decrement, select).  The arithmetic on v is untouched.  Inside the pipeline the chip is bound by
// vector-instruction issue, and scalar instructions issue beside it.  Other periods keep the vector
// countdown (REFM = false).
// ST: the launch continues from a saved state and / or saves its own (lif_common.h); prologue and epilogue only.  REFM: the
// state's countdown 2 / 1 is the lane mask h2 / h1.
// The body is lif_dense_kernel.inc: one text for this kernel and for the fused step kernel (step_fused.hip), which runs it
// behind the front end of the same clip.  The six macros name what differs between the two: where the LDS image lies, where
// the input bit rows come from, and how many steps the clip runs and its features count; here they expand to the tokens the
// body held before it was shared.
template <int SL, int WPC, int INMODE, bool REFM, bool ST = false>
__global__ __launch_bounds__(WPC * 64) void lif_dense_kernel(const DenseArgs a)
{
#define LSM_DENSE_LDS_DECL extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#define LSM_DENSE_LDS smem
#define LSM_DENSE_INPUT_BITS_INC "lif_dense_pack_raster.inc"
#define LSM_DENSE_CLIP_STEPS \
    !ST ? T : SCALE_LATE ? clip_step_count_unscaled(a.st, b, T) : clip_step_count(a.st, b, T, LSM_DENSE_ST_OFFSET)
#define LSM_DENSE_FEATURE_STEPS ST ? Tb + a.st.t0 : T
#define LSM_DENSE_ST_OFFSET offsetof(DenseArgs, st)
#include "lif_dense_kernel.inc"
#undef LSM_DENSE_LDS_DECL
#undef LSM_DENSE_LDS
#undef LSM_DENSE_INPUT_BITS_INC
#undef LSM_DENSE_CLIP_STEPS
#undef LSM_DENSE_FEATURE_STEPS
#undef LSM_DENSE_ST_OFFSET
}

typedef void (*dense_fn_t)(const DenseArgs);

// What a state step (include/lsm_hip_step_state.h) adds to the dense launch of a pipeline step: lsm_reservoir_run_from's
// first_step and state blocks and, `segmented`, lsm_reservoir_run_segments' segment_steps and records.
struct StepState {
    int first_step = 0;
    const void *state_in = nullptr;
    void *state_out = nullptr;
    bool segmented = false;
    int segment_steps = 0;
    void *records = nullptr;
};

// reservoir.hip, for step_fused.hip: the arguments, slots per lane and LDS bytes of the dense launch of one pipeline step.
// `state`: the step continues from / saves a state or closes segment records -- the refusals are then those of
// lsm_reservoir_run_from / _run_segments (n_keys may be 0), and DenseArgs::st is filled as those entry points fill it.
int step_dense_args(const ::lsm_reservoir *h, int n_clips, int n_steps, const int32_t *key_ids, int n_keys, float *features,
                    int32_t *stats, bool probe, DenseArgs *out, int *sl_out, size_t *lds_out, const StepState *state = nullptr);

// REFM needs 2 x 2 scalar registers per slot: offered up to 4 slots per lane (the layouts of N <= 4096 with >= 4
// waves, i.e. every reservoir the dense rows serve by default); fatter layouts keep the countdown in vector registers.
constexpr int DENSE_REFM_MAX_SL = 4;
constexpr int DENSE_REFM_REFRACTORY = 2;        // the one period the mask form is written for (the reference's)

template <int SL, int INMODE, bool REFM, bool ST>
dense_fn_t pick_dense_wpc(int wpc)
{
    switch (wpc) {
    case 1: return lif_dense_kernel<SL, 1, INMODE, REFM, ST>;
    case 2: return lif_dense_kernel<SL, 2, INMODE, REFM, ST>;
    case 4: return lif_dense_kernel<SL, 4, INMODE, REFM, ST>;
    case 8: return lif_dense_kernel<SL, 8, INMODE, REFM, ST>;
    case 16: return lif_dense_kernel<SL, 16, INMODE, REFM, ST>;
    default: return nullptr;
    }
}

template <int INMODE, bool ST>
dense_fn_t pick_dense_sl_st(int sl, int wpc, bool refm)
{
    if (refm && sl <= DENSE_REFM_MAX_SL) {
        switch (sl) {
        case 1: return pick_dense_wpc<1, INMODE, true, ST>(wpc);
        case 2: return pick_dense_wpc<2, INMODE, true, ST>(wpc);
        case 4: return pick_dense_wpc<4, INMODE, true, ST>(wpc);
        default: return nullptr;
        }
    }
    switch (sl) {
    case 1: return pick_dense_wpc<1, INMODE, false, ST>(wpc);
    case 2: return pick_dense_wpc<2, INMODE, false, ST>(wpc);
    case 4: return pick_dense_wpc<4, INMODE, false, ST>(wpc);
    case 8: if (INMODE >= 2) return nullptr; else return pick_dense_wpc<INMODE >= 2 ? 4 : 8, INMODE, false, ST>(wpc);
    case 16: if (INMODE >= 2) return nullptr; else return pick_dense_wpc<INMODE >= 2 ? 4 : 16, INMODE, false, ST>(wpc);
    default: return nullptr;
    }
}

// state: the ST form (continuation)
template <int INMODE>
dense_fn_t pick_dense_sl(int sl, int wpc, bool refm, bool state)
{
    return state ? pick_dense_sl_st<INMODE, true>(sl, wpc, refm) : pick_dense_sl_st<INMODE, false>(sl, wpc, refm);
}

// refm: the caller checked a.refractory == DENSE_REFM_REFRACTORY (else the countdown stays in vector registers)
dense_fn_t pick_dense_0(int sl, int wpc, bool refm, bool state);      // lif_dense_0.hip (INMODE 0: entries from global memory)
dense_fn_t pick_dense_1(int sl, int wpc, bool refm, bool state);      // lif_dense_1.hip (INMODE 1: entries in registers)
dense_fn_t pick_dense_2(int sl, int wpc, bool refm, bool state);      // lif_dense_2.hip (INMODE 2: channel masks, C <= 128, SL <= 4)
dense_fn_t pick_dense_3(int sl, int wpc, bool refm, bool state);      // lif_dense_3.hip (INMODE 3: channel masks at coloured positions)

}  // namespace lsm_lif
