// The masked spike encoders (SPEC.md 1.13, include/lsm_hip_mask.h): SpecAugment-style frequency and time masks applied to the
// normalised spectrogram INSIDE the encoders, before the latches see a value.  The kernels here are the MASK = true
// forms of the code that the unmasked kernels of frontend.hip run with MASK = false (spikes_body.h's device function,
// gammatone_spikes_kernel.inc's kernel text); they are a translation unit of their own because the fused kernel has three
// dozen forms and the units compile in parallel.  The entry points, their refusals and the launch geometry are frontend.hip's:
// it calls the two launch functions below once everything is checked.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void spec_to_spikes_masked_kernel(const lsm_fe::SpikeArgs<T> a, const lsm_fe::MaskArgs m)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lsm_fe::spec_to_spikes_body<T, true>(a, (int)blockIdx.x, smem, m);
}

// gammatone_spikes_masked_kernel(const FusedArgs a, const lsm_fe::MaskArgs m): the fused kernel's text with MASK = true
#define LSM_FUSED_KERNEL gammatone_spikes_masked_kernel
#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(GT_MAX_WPB * 64)
#define LSM_FUSED_TAIL_INC "gammatone_spikes_raster_out.inc"
#define LSM_FUSED_PARAMS const FusedArgs a, const lsm_fe::MaskArgs m
#define LSM_FUSED_MASK constexpr bool MASK = true;
#define LSM_FUSED_RAGGED constexpr bool RAGGED = false; const lsm_fe::RaggedArgs rg{nullptr, nullptr};
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_TAIL_INC
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_MASK
#undef LSM_FUSED_RAGGED

template <int N> using Int = std::integral_constant<int, N>;

}  // namespace

namespace lsm_fe {

template <typename T>
void launch_spec_to_spikes_masked(const SpikeArgs<T> &a, const MaskArgs &m, int threads, size_t lds, void *stream)
{
    auto fn = spec_to_spikes_masked_kernel<T>;
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
    hipLaunchKernelGGL(fn, dim3(a.n_clips), dim3(threads), lds, (hipStream_t)stream, a, m);
}
template void launch_spec_to_spikes_masked<double>(const SpikeArgs<double> &, const MaskArgs &, int, size_t, void *);
template void launch_spec_to_spikes_masked<float>(const SpikeArgs<float> &, const MaskArgs &, int, size_t, void *);

void launch_gammatone_spikes_masked(const FusedLaunch &l, const void *fused_args, const MaskArgs &m, void *stream)
{
    const FusedArgs &a = *static_cast<const FusedArgs *>(fused_args);
    auto launch = [&](auto nw_c, auto fast_c, auto nch_c, auto shb0_c, auto pair_c) {
        auto fn = gammatone_spikes_masked_kernel<decltype(nw_c)::value, decltype(fast_c)::value, decltype(nch_c)::value,
                                                 decltype(shb0_c)::value, decltype(pair_c)::value>;
        if (l.lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
        hipLaunchKernelGGL(fn, dim3(l.grid), dim3(l.block), l.lds, (hipStream_t)stream, a, m);
    };
    // the eight forms of a kernel, as in lsm_gammatone_spikes_f64
    auto launch_nw = [&](auto nw_c) {
        using T = std::true_type;
        using F = std::false_type;
        if (l.fast) {
            if (l.pair) { if (l.shb0) launch(nw_c, T{}, Int<1>{}, T{}, T{}); else launch(nw_c, T{}, Int<1>{}, F{}, T{}); }
            else if (l.nch == 2) { if (l.shb0) launch(nw_c, T{}, Int<2>{}, T{}, F{}); else launch(nw_c, T{}, Int<2>{}, F{}, F{}); }
            else launch(nw_c, T{}, Int<1>{}, F{}, F{});
        } else {
            if (l.pair) launch(nw_c, F{}, Int<1>{}, F{}, T{});
            else if (l.nch == 2) launch(nw_c, F{}, Int<2>{}, F{}, F{});
            else launch(nw_c, F{}, Int<1>{}, F{}, F{});
        }
    };
    switch (l.nw) {
    case 1: launch_nw(Int<1>{}); break;
    case 2: launch_nw(Int<2>{}); break;
    case 3: launch_nw(Int<3>{}); break;
    default: launch_nw(Int<4>{}); break;
    }
}

}  // namespace lsm_fe
