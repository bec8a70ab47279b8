// The ragged one-launch step (include/lsm_hip_step.h: lsm_step_fused_ragged_f64): step_fused.hip's kernels with
// RAGGED = true -- clip b filters and encodes its own rg.bins[b] time bins exactly as gammatone_spikes_ragged_kernel does
// (ragged_frontend.hip, SPEC.md 1.14), and the reservoir half runs that many bins' steps with the features of that many steps
// (step_fused_tail.inc).  rg.steps_out is null: the count never leaves the workgroup.  A translation unit of its own: six forms
// that compile beside step_fused.hip's six, which keep their machine code.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"
#include "step_fused_forms.h"
#include <cstring>

#define LSM_STEP_FAMILY_KERNEL(sl) step_fused_ragged_kernel_sl##sl
#define LSM_STEP_FAMILY_ARG lsm_fe::RaggedArgs
#define LSM_STEP_FAMILY_ARG_NAME rg
#define LSM_STEP_FAMILY_LAUNCH launch_step_ragged
#define LSM_FUSED_MASK constexpr bool MASK = false; const lsm_fe::MaskArgs m{nullptr, nullptr};
#define LSM_FUSED_RAGGED constexpr bool RAGGED = true;
#define LSM_FUSED_STATE constexpr bool ST = false; const lsm_step::StateRows sx{nullptr};
#include "step_fused_family.inc"
