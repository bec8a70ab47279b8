// step_fused_forms.h -- the masked, the ragged and the state forms of the one-launch step (include/lsm_hip_step.h,
// include/lsm_hip_step_state.h), each family in a translation unit of its own (step_fused_masked.hip,
// step_fused_ragged.hip, step_fused_state.hip) so that the units compile in parallel and step_fused.hip keeps its objects.
// step_fused.hip alone refuses, plans and builds the arguments; it then calls one of the launch functions below.  `fused_args`: the front half's FusedArgs as bytes (the type lives in each unit's
// unnamed namespace: gammatone_spikes_body.h, StepFront).
#pragma once
#include "lsm_common.h"
#include "spikes_body.h"
#include "lif_dense.h"

namespace lsm_step {

// which kernel text (neuron slots per lane: 1, 2 or 4), which of its two forms (the shared first-section gain), and the
// launch geometry: one workgroup of 256 threads per clip, `lds` bytes of dynamic LDS
struct StepLaunch {
    int sl;
    bool shb0;
    unsigned grid, block;
    size_t lds;
};

// The state family's own kernel argument (step_fused_state.hip).  State and segments themselves travel in DenseArgs::st, as
// in every ST form of the reservoir kernels; what the fused kernel adds is the clip's tumbling feature rows.
struct StateRows {
    float *segment_rows;       // (n_clips, T / seg, n_keys * n_out) or null; a segmented launch only
};

// The masked ragged family's own kernel argument (step_fused_ragged_masked.hip): the ragged step's counts and the masked
// step's words, one argument because a family has one
struct RaggedMaskArgs {
    lsm_fe::RaggedArgs rg;
    lsm_fe::MaskArgs m;
};

// false: no such form (sl is none of 1, 2, 4); nothing was launched
bool launch_step_masked(const StepLaunch &l, const void *fused_args, const lsm_lif::DenseArgs &d, const lsm_fe::MaskArgs &m,
                        void *stream);
bool launch_step_ragged(const StepLaunch &l, const void *fused_args, const lsm_lif::DenseArgs &d, const lsm_fe::RaggedArgs &rg,
                        void *stream);
bool launch_step_ragged_masked(const StepLaunch &l, const void *fused_args, const lsm_lif::DenseArgs &d, const RaggedMaskArgs &rm,
                               void *stream);
bool launch_step_state(const StepLaunch &l, const void *fused_args, const lsm_lif::DenseArgs &d, const StateRows &sx,
                       void *stream);

}  // namespace lsm_step
