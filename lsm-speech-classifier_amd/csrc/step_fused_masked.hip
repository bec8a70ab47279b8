// The masked one-launch step (include/lsm_hip_step.h: lsm_step_fused_masked_f64): step_fused.hip's kernels with
// MASK = true -- the front half is the masked lane-pair kernel of lsm_gammatone_spikes_masked_f64 (mask.hip), a masked value is
// +0.0 before the latches (SPEC.md 1.13); the tail is the plain step's.  A translation unit of its own: six forms that compile
// beside step_fused.hip's six, which keep their machine code.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"
#include "step_fused_forms.h"
#include <cstring>

#define LSM_STEP_FAMILY_KERNEL(sl) step_fused_masked_kernel_sl##sl
#define LSM_STEP_FAMILY_ARG lsm_fe::MaskArgs
#define LSM_STEP_FAMILY_ARG_NAME m
#define LSM_STEP_FAMILY_LAUNCH launch_step_masked
#define LSM_FUSED_MASK constexpr bool MASK = true;
#define LSM_FUSED_RAGGED constexpr bool RAGGED = false; const lsm_fe::RaggedArgs rg{nullptr, nullptr};
#define LSM_FUSED_STATE constexpr bool ST = false; const lsm_step::StateRows sx{nullptr};
#include "step_fused_family.inc"
