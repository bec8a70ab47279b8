// The state forms of the one-launch step (include/lsm_hip_step_state.h: lsm_step_fused_from_f64, lsm_step_fused_segments_f64,
// DESIGN.md 3a): step_fused.hip's kernels with the reservoir half in its ST form -- the workgroup loads its clip's SPEC.md 4a
// state block behind the front end, runs the launch's T steps, closes the 4b segment records on the way, stores the state and
// writes the features of [0, first_step + T) (step_fused_tail.inc).  State and segments are DenseArgs::st, filled as
// lsm_reservoir_run_from / _run_segments fill it; the family's own argument is the pointer of the tumbling segment rows.  The
// front half is the plain one: no mask, no ragged count.  A translation unit of its own: six forms that compile beside the
// eighteen of the other three units, which keep their machine code.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"
#include "step_fused_forms.h"
#include <cstring>

#define LSM_STEP_FAMILY_KERNEL(sl) step_fused_state_kernel_sl##sl
#define LSM_STEP_FAMILY_ARG lsm_step::StateRows
#define LSM_STEP_FAMILY_ARG_NAME sx
#define LSM_STEP_FAMILY_LAUNCH launch_step_state
#define LSM_FUSED_MASK constexpr bool MASK = false; const lsm_fe::MaskArgs m{nullptr, nullptr};
#define LSM_FUSED_RAGGED constexpr bool RAGGED = false; const lsm_fe::RaggedArgs rg{nullptr, nullptr};
#define LSM_FUSED_STATE constexpr bool ST = true;
#include "step_fused_family.inc"
