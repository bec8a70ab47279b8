// Masks on ragged launches (SPEC.md 1.16, include/lsm_hip_ragged_augment.h): the MASK = true, RAGGED = true forms of the code
// that mask.hip runs with RAGGED = false and ragged_frontend.hip with MASK = false (spikes_body.h's device function,
// gammatone_spikes_kernel.inc's kernel text), in a translation unit of their own so that they compile beside those two.  The
// entry points fill a launch request in frontend.hip, which alone refuses, plans and builds the arguments, then calls the two
// launch functions below; the fused kernel's form is picked by the one table (launch_fused_form, gammatone_spikes_body.h).
//
// A clip's time bit j names bin j of its own T_b bins; its mask rows lie at the launch's stride, ceil(time_bins / 32) words.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void spec_to_spikes_ragged_masked_kernel(const lsm_fe::SpikeArgs<T> a, const lsm_fe::RaggedCounts rc,
                                                                           const lsm_fe::MaskArgs m)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lsm_fe::spec_to_spikes_body<T, true, true>(a, (int)blockIdx.x, smem, m, rc);
}

// gammatone_spikes_ragged_masked_kernel(const FusedArgs a, const lsm_fe::RaggedArgs rg, const lsm_fe::MaskArgs m): the fused
// kernel's text with both switches on
#define LSM_FUSED_KERNEL gammatone_spikes_ragged_masked_kernel
#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(GT_MAX_WPB * 64)
#define LSM_FUSED_TAIL_INC "gammatone_spikes_raster_out.inc"
#define LSM_FUSED_PARAMS const FusedArgs a, const lsm_fe::RaggedArgs rg, const lsm_fe::MaskArgs m
#define LSM_FUSED_MASK constexpr bool MASK = true;
#define LSM_FUSED_RAGGED constexpr bool RAGGED = true;
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_TAIL_INC
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_MASK
#undef LSM_FUSED_RAGGED

// this unit's kernel for the form table (gammatone_spikes_body.h, launch_fused_form)
struct RaggedMaskedFamily {
    template <int NW, bool FAST, int NCH, bool SHB0, bool PAIR>
    static auto kernel() { return gammatone_spikes_ragged_masked_kernel<NW, FAST, NCH, SHB0, PAIR>; }
};

}  // namespace

namespace lsm_fe {

template <typename T>
void launch_spec_to_spikes_ragged_masked(const SpikeArgs<T> &a, const RaggedCounts &rc, const MaskArgs &m, int threads, size_t lds,
                                         void *stream)
{
    auto fn = spec_to_spikes_ragged_masked_kernel<T>;
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
    hipLaunchKernelGGL(fn, dim3(a.n_clips), dim3(threads), lds, (hipStream_t)stream, a, rc, m);
}
template void launch_spec_to_spikes_ragged_masked<double>(const SpikeArgs<double> &, const RaggedCounts &, const MaskArgs &, int,
                                                          size_t, void *);
template void launch_spec_to_spikes_ragged_masked<float>(const SpikeArgs<float> &, const RaggedCounts &, const MaskArgs &, int,
                                                         size_t, void *);

void launch_gammatone_spikes_ragged_masked(const FusedLaunch &l, const void *fused_args, const RaggedArgs &rg, const MaskArgs &m,
                                           void *stream)
{
    launch_fused_form<RaggedMaskedFamily>(l, stream, *static_cast<const FusedArgs *>(fused_args), rg, m);
}

}  // namespace lsm_fe
