// step_fused_family.inc -- one family of the one-launch step's kernels beside the plain one of step_fused.hip: the three kernel
// texts (1, 2 and 4 neuron slots per lane) in the two forms the step serves (3 live windows, the fast coefficient path, the
// lane pair; with and without the shared b0), and the function that launches one of them.  The includer
// (step_fused_masked.hip, step_fused_ragged.hip, step_fused_ragged_masked.hip, step_fused_state.hip) says
//   LSM_STEP_FAMILY_KERNEL(sl)   the kernels' names;
//   LSM_STEP_FAMILY_ARG          the type of the family's own kernel argument, behind FusedArgs and DenseArgs;
//   LSM_STEP_FAMILY_ARG_NAME     its name in the kernel text (`m`, `rg`, `sx`, or `rm`, which carries both `rg` and `m`);
//   LSM_FUSED_MASK, LSM_FUSED_RAGGED   as gammatone_spikes_kernel.inc reads them;
//   LSM_FUSED_STATE                    as step_fused_tail.inc reads it (constexpr bool ST, and `sx` where it is no parameter);
//   LSM_STEP_FAMILY_LAUNCH       the name of the launch function (step_fused_forms.h).
// Qualifiers and tail are step_fused.hip's: 256 threads, four workgroups per CU, step_fused_tail.inc.
namespace {

#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(256, 4)
#define LSM_FUSED_PARAMS const FusedArgs a, const lsm_lif::DenseArgs d, const LSM_STEP_FAMILY_ARG LSM_STEP_FAMILY_ARG_NAME
#define LSM_FUSED_TAIL_INC "step_fused_tail.inc"

#define LSM_FUSED_KERNEL LSM_STEP_FAMILY_KERNEL(1)
#define LSM_STEP_SL 1
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#define LSM_FUSED_KERNEL LSM_STEP_FAMILY_KERNEL(2)
#define LSM_STEP_SL 2
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#define LSM_FUSED_KERNEL LSM_STEP_FAMILY_KERNEL(4)
#define LSM_STEP_SL 4
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_TAIL_INC

typedef void (*step_family_fn_t)(const FusedArgs, const lsm_lif::DenseArgs, const LSM_STEP_FAMILY_ARG);

step_family_fn_t pick_step_family(int sl, bool shb0)
{
    switch (sl) {
    case 1: return shb0 ? LSM_STEP_FAMILY_KERNEL(1)<3, true, 1, true, true> : LSM_STEP_FAMILY_KERNEL(1)<3, true, 1, false, true>;
    case 2: return shb0 ? LSM_STEP_FAMILY_KERNEL(2)<3, true, 1, true, true> : LSM_STEP_FAMILY_KERNEL(2)<3, true, 1, false, true>;
    case 4: return shb0 ? LSM_STEP_FAMILY_KERNEL(4)<3, true, 1, true, true> : LSM_STEP_FAMILY_KERNEL(4)<3, true, 1, false, true>;
    default: return nullptr;
    }
}

}  // namespace

bool lsm_step::LSM_STEP_FAMILY_LAUNCH(const StepLaunch &l, const void *fused_args, const lsm_lif::DenseArgs &d,
                                      const LSM_STEP_FAMILY_ARG &x, void *stream)
{
    step_family_fn_t fn = pick_step_family(l.sl, l.shb0);
    if (fn == nullptr) return false;
    FusedArgs a;
    memcpy(&a, fused_args, sizeof a);
    if (l.lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
    hipLaunchKernelGGL(fn, dim3(l.grid), dim3(l.block), l.lds, (hipStream_t)stream, a, d, x);
    return true;
}
