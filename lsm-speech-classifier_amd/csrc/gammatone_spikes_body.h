// gammatone_spikes_body.h -- the fused gammatone front end (filterbank -> dB -> normalise -> resize -> hysteresis encoder ->
// raster in ONE launch): its argument type, its helpers, the kernel that frontend.hip launches and the one table that picks a
// form of it for every unit that instantiates its text (launch_fused_form, at the end).  The kernel's text is
// gammatone_spikes_kernel.inc; the masked kernel (mask.hip, SPEC.md 1.13) is the same text with MASK = true, in a
// translation unit of its own, compiled beside frontend.hip.
// Everything here sits in an unnamed namespace, as it did inside frontend.hip: the kernels' symbols carry that
// namespace and FusedArgs in their names, and those names stay what they were.
#pragma once
#include "lsm_common.h"
#include "gammatone_body.h"
#include "spikes_body.h"
#include <type_traits>

namespace {

constexpr int NWIN_MAX = 4;
constexpr int GT_MAX_WPB = 8;           // waves per workgroup, at most
using lsm_fe::MAX_THR;

// ---------------------------------------------------------------------------------------------
// Fused front end: filterbank -> dB -> floor/min-max normalise -> linear resize -> hysteresis encoder ->
// uint8 raster in ONE launch (create_dataset.py:49-104 per clip).  The filter loop is the one of
// gammatone_kernel; what differs:
//   * a wave carries NCH channel groups of its clip (NCH = 2: 128 channels, two independent float64
//     dependency chains per lane that share the scalar sample loads and the float32 -> float64
//     conversion), so at 128 filters ONE WAVE IS ONE CLIP and the clip's max/min need no other wave;
//   * the clip's dB columns go to a private scratch, column-major per wave (64 consecutive doubles per
//     store); the lane that wrote a value is the only one that reads it back, after the last window, when
//     the clip's maximum is known.  A row's 98 float64 values do not fit the registers next to the filter
//     state of two chains and 100 KB per clip do not fit the LDS four times per CU;
//   * max/min: running per lane, xor-shuffles per wave, one LDS exchange when a clip spans several waves
//     (the waves of a clip always share a workgroup);
//   * normalise / SciPy-exact resize / 4-threshold latch: one lane per channel, arithmetic and comparison
//     order of spec_to_spikes_kernel<double>; the raster rows of a wave are staged bit-packed in LDS and
//     leave as coalesced 4-byte stores.
// Waves beyond the batch (last workgroup) skip the filter loop but keep the barriers.
//
// PAIR (lane-pair layout, NCH = 1): a wave carries 32 channels of its clip, channel j in lanes j (head) and j + 32
// (tail), so at 128 filters a clip is 4 waves and a 256-clip launch puts a wave on every SIMD.  In the iteration of
// sample n the head runs sections 1-2 on sample n + 1 and the tail sections 3-4 on sample n, fed with the head's
// section-2 output of sample n, which v_permlane32_swap moves from lane j to lane j + 32 at the top of the iteration.
// Both halves run the same two-section code with their own section coefficients and state.  The division, the
// square and the window sums run on both halves (one instruction stream) but only the tail's feed the dB columns,
// the max/min and the epilogue.  Every float64 operation of a channel and its order are those of the other layouts:
// the skew only changes when section 3 sees a value, and the hand-off moves bits.
// ---------------------------------------------------------------------------------------------
struct FusedArgs {
    const float *audio;
    const double *coefs;
    double *ws;                 // (n_clips, ncols, groups*NCH*64) float64 scratch (32 channels per group in the lane pair)
    uint8_t *raster;            // (n_clips, n_filters*redundancy, time_bins*n_thr)
    int n_clips, n_samples, n_filters, nwin, hop, ncols;
    int time_bins, n_thr, redundancy, groups;
    int unused_;                // (keeps the argument layout, and with it the filter loop's code, of the measured build)
    int prio;                   // wave priority of the filter loop: 0 (see the kernel)
    double on[MAX_THR], off[MAX_THR];
};

// Head lanes (0-31) keep `lo`, tail lanes (32-63) receive v of lane - 32: v_permlane32_swap exchanges lanes 32-63 of
// its first operand with lanes 0-31 of its second; one swap per 32-bit half.
__device__ __forceinline__ double pair_up(double lo, double v)
{
    const unsigned long long a = (unsigned long long)__double_as_longlong(lo);
    const unsigned long long c = (unsigned long long)__double_as_longlong(v);
    const auto rl = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)c, false, false);
    const auto rh = __builtin_amdgcn_permlane32_swap((unsigned)(a >> 32), (unsigned)(c >> 32), false, false);
    return __longlong_as_double((long long)(((unsigned long long)rh[0] << 32) | rl[0]));
}

__device__ __forceinline__ double uniform_f64(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The unmasked kernel: the text of gammatone_spikes_kernel.inc with MASK = false
#define LSM_FUSED_KERNEL gammatone_spikes_kernel
#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(GT_MAX_WPB * 64)
#define LSM_FUSED_TAIL_INC "gammatone_spikes_raster_out.inc"
#define LSM_FUSED_PARAMS const FusedArgs a
#define LSM_FUSED_MASK constexpr bool MASK = false; const lsm_fe::MaskArgs m{nullptr, nullptr};
#define LSM_FUSED_RAGGED constexpr bool RAGGED = false; const lsm_fe::RaggedArgs rg{nullptr, nullptr};
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_TAIL_INC
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_MASK
#undef LSM_FUSED_RAGGED

}  // namespace

namespace lsm_fe {

// What the host needs to launch one of the kernel's forms: chosen by fused_plan and the entry point's checks (frontend.hip)
struct FusedLaunch {
    int nw, nch;                // live windows (1..4), chains per lane
    bool fast, shb0, pair;
    unsigned grid, block;
    size_t lds;
};

// The masked launches, defined in mask.hip (their kernels are a translation unit of their own); frontend.hip calls them once
// its one check (plan_front, launch_spec_to_spikes) has passed.  `fused_args`: a FusedArgs -- the type lives in each unit's
// unnamed namespace, so it crosses between units as bytes: here, at the ragged launch below and in StepFront, nowhere else.
void launch_gammatone_spikes_masked(const FusedLaunch &l, const void *fused_args, const MaskArgs &m, void *stream);
template <typename T>
void launch_spec_to_spikes_masked(const SpikeArgs<T> &a, const MaskArgs &m, int threads, size_t lds, void *stream);

// The front-end half of a fused step launch (step_fused.hip, include/lsm_hip_step.h): what lsm_gammatone_spikes_f64 would
// launch for these arguments, after the same refusals -- the FusedArgs as bytes, for the reason above.  frontend.hip.
struct StepFront {
    FusedLaunch l;
    alignas(8) unsigned char args[sizeof(FusedArgs)];
};
int step_front_args(const float *audio, int n_clips, int n_samples, const double *coefs, int n_filters, int nwin, int hop,
                    int ncols, int time_bins, const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                    void *workspace, long workspace_bytes, int coef_flags, StepFront *out);
// the own refusals of the masked and of the ragged step (lsm_step_fused_masked_f64, lsm_step_fused_ragged_f64): those of the
// masked and of the ragged front end, in their order and words.  frontend.hip.
int step_check_masks(const uint32_t *freq_mask, const uint32_t *time_mask);
int step_check_ragged(const int32_t *clip_bins, int time_bins, long n_samples, long hop);

// The ragged launches (SPEC.md 1.14), defined in ragged_frontend.hip, likewise a translation unit of its own
void launch_gammatone_spikes_ragged(const FusedLaunch &l, const void *fused_args, const RaggedArgs &rg, void *stream);
template <typename T>
void launch_spec_to_spikes_ragged(const SpikeArgs<T> &a, const RaggedCounts &rc, int threads, size_t lds, void *stream);

// The masked ragged launches (SPEC.md 1.16), defined in ragged_masked_frontend.hip, likewise
void launch_gammatone_spikes_ragged_masked(const FusedLaunch &l, const void *fused_args, const RaggedArgs &rg, const MaskArgs &m,
                                           void *stream);
template <typename T>
void launch_spec_to_spikes_ragged_masked(const SpikeArgs<T> &a, const RaggedCounts &rc, const MaskArgs &m, int threads, size_t lds,
                                         void *stream);

}  // namespace lsm_fe

namespace {

// The form table of the fused kernel, once for every translation unit that instantiates its text.  `Family` names the unit's
// kernel: a struct whose `template <int NW, bool FAST, int NCH, bool SHB0, bool PAIR> static auto kernel()` returns it;
// `args` are the kernel's arguments (the FusedArgs, then the family's own: none, MaskArgs or RaggedArgs).
template <typename Family, typename... Args>
void launch_fused_form(const lsm_fe::FusedLaunch &l, void *stream, const Args &...args)
{
    using T = std::true_type;
    using F = std::false_type;
    using One = std::integral_constant<int, 1>;
    using Two = std::integral_constant<int, 2>;
    auto launch = [&](auto nw_c, auto fast_c, auto nch_c, auto shb0_c, auto pair_c) {
        auto fn = Family::template kernel<decltype(nw_c)::value, decltype(fast_c)::value, decltype(nch_c)::value,
                                          decltype(shb0_c)::value, decltype(pair_c)::value>();
        if (l.lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
        hipLaunchKernelGGL(fn, dim3(l.grid), dim3(l.block), l.lds, (hipStream_t)stream, args...);
    };
    // the eight forms of a kernel: the shared b0 exists on the fast path only, and not with one chain per lane
    auto launch_nw = [&](auto nw_c) {
        if (l.fast) {
            if (l.pair) { if (l.shb0) launch(nw_c, T{}, One{}, T{}, T{}); else launch(nw_c, T{}, One{}, F{}, T{}); }
            else if (l.nch == 2) { if (l.shb0) launch(nw_c, T{}, Two{}, T{}, F{}); else launch(nw_c, T{}, Two{}, F{}, F{}); }
            else launch(nw_c, T{}, One{}, F{}, F{});
        } else {
            if (l.pair) launch(nw_c, F{}, One{}, F{}, T{});
            else if (l.nch == 2) launch(nw_c, F{}, Two{}, F{}, F{});
            else launch(nw_c, F{}, One{}, F{}, F{});
        }
    };
    switch (l.nw) {
    case 1: launch_nw(std::integral_constant<int, 1>{}); break;
    case 2: launch_nw(std::integral_constant<int, 2>{}); break;
    case 3: launch_nw(std::integral_constant<int, 3>{}); break;
    default: launch_nw(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace
