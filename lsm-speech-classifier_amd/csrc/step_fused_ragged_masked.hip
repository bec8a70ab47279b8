// The masked ragged one-launch step (include/lsm_hip_ragged_augment.h: lsm_step_fused_ragged_masked_f64, SPEC.md 1.16):
// step_fused.hip's kernels with MASK = true and RAGGED = true -- the front half is the lane-pair form of
// gammatone_spikes_ragged_masked_kernel (ragged_masked_frontend.hip), the tail the ragged step's (step_fused_ragged.hip).  The
// family's one argument carries both the counts and the masks.  A translation unit of its own: six forms that compile beside
// the other families', which keep their machine code.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"
#include "step_fused_forms.h"
#include <cstring>

#define LSM_STEP_FAMILY_KERNEL(sl) step_fused_ragged_masked_kernel_sl##sl
#define LSM_STEP_FAMILY_ARG lsm_step::RaggedMaskArgs
#define LSM_STEP_FAMILY_ARG_NAME rm
#define LSM_STEP_FAMILY_LAUNCH launch_step_ragged_masked
#define LSM_FUSED_MASK constexpr bool MASK = true; const lsm_fe::MaskArgs m = rm.m;
#define LSM_FUSED_RAGGED constexpr bool RAGGED = true; const lsm_fe::RaggedArgs rg = rm.rg;
#define LSM_FUSED_STATE constexpr bool ST = false; const lsm_step::StateRows sx{nullptr};
#include "step_fused_family.inc"
