// step_fused_tail.inc -- what the fused step kernels (step_fused.hip, step_fused_masked.hip, step_fused_ragged.hip) do once
// their clip's raster rows are staged in LDS, included by gammatone_spikes_kernel.inc where the other kernels write the raster
// out (LSM_FUSED_TAIL_INC): the reservoir's dense-row time loop (lif_dense_kernel.inc, the <LSM_STEP_SL, 4, 3, true> form) on
// the same clip in the same workgroup.  `d` is the launch's lsm_lif::DenseArgs; its LDS image lies behind the front end's
// stage, and its input bit rows come from that stage (step_fused_bits.inc).  The barrier in front of this file has made every
// wave's staged rows visible.
// RAGGED: the workgroup is one clip, so its bin count is the workgroup's: the time loop runs the clip's own tb_clip * n_thr
// steps (`row_bits`) and the features are those of T = that count (LSM_DENSE_CLIP_STEPS; no state block, no count in memory).
// A clip of 0 bins ends here, all 4 waves of it behind the same barrier: its feature row and stats row stay as they were.
{
    using namespace lsm_lif;
    static_assert(PAIR && NCH == 1, "the fused step runs the lane-pair front end: 4 waves of 32 channels per clip");
    if constexpr (RAGGED) {
        if (tb_clip == 0) return;                       // workgroup-uniform
    }
    const uint32_t *const step_stage = stage_all;
    const int step_rw = RW, step_red = a.redundancy;
    unsigned char *const step_lds = smem + 2 * GT_MAX_WPB * sizeof(double) + (size_t)(blockDim.x >> 6) * CPW * RW * 4;
    {
        const DenseArgs &a = d;
        constexpr int SL = LSM_STEP_SL, WPC = 4, INMODE = 3;
        constexpr bool REFM = true, ST = false;
#define LSM_DENSE_LDS_DECL
#define LSM_DENSE_LDS step_lds
#define LSM_DENSE_INPUT_BITS_INC "step_fused_bits.inc"
#define LSM_DENSE_CLIP_STEPS RAGGED ? row_bits : T
#define LSM_DENSE_FEATURE_STEPS RAGGED ? Tb : T
#include "lif_dense_kernel.inc"
#undef LSM_DENSE_LDS_DECL
#undef LSM_DENSE_LDS
#undef LSM_DENSE_INPUT_BITS_INC
#undef LSM_DENSE_CLIP_STEPS
#undef LSM_DENSE_FEATURE_STEPS
    }
}
