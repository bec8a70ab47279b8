// step_fused_tail.inc -- what the fused step kernels (step_fused.hip, step_fused_masked.hip, step_fused_ragged.hip,
// step_fused_state.hip) do once
// their clip's raster rows are staged in LDS, included by gammatone_spikes_kernel.inc where the other kernels write the raster
// out (LSM_FUSED_TAIL_INC): the reservoir's dense-row time loop (lif_dense_kernel.inc, the <LSM_STEP_SL, 4, 3, true> form) on
// the same clip in the same workgroup.  `d` is the launch's lsm_lif::DenseArgs; its LDS image lies behind the front end's
// stage, and its input bit rows come from that stage (step_fused_bits.inc).  The barrier in front of this file has made every
// wave's staged rows visible.
// RAGGED: the workgroup is one clip, so its bin count is the workgroup's: the time loop runs the clip's own tb_clip * n_thr
// steps (`row_bits`) and the features are those of T = that count (LSM_DENSE_CLIP_STEPS; no state block, no count in memory).
// A clip of 0 bins ends here, all 4 waves of it behind the same barrier: its feature row and stats row stay as they were.
// ST (LSM_FUSED_STATE, step_fused_state.hip): the reservoir half is the text's ST form on d.st -- the SPEC.md 4a state block
// loaded and stored, the 4b segment records closed -- over T steps with the features of first_step + T.  The text's zero-step
// exit reads StateArgs from the kernel-argument segment, where DenseArgs is this kernel's SECOND parameter: it is given the
// true offset (step_st_offset), although no launch reaches it (a state step is never ragged and the host refuses T < 1).
// With sx.segment_rows the workgroup ends by writing its clip's T / seg tumbling feature rows from its own records.
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
        constexpr bool REFM = true;
        LSM_FUSED_STATE                                 // constexpr bool ST, and `sx` where it is no parameter
        static_assert(!(ST && RAGGED), "there is no ragged state step");
        constexpr size_t step_st_offset = ((sizeof(FusedArgs) + alignof(DenseArgs) - 1) & ~(alignof(DenseArgs) - 1)) +
                                          offsetof(DenseArgs, st);
#define LSM_DENSE_LDS_DECL
#define LSM_DENSE_LDS step_lds
#define LSM_DENSE_INPUT_BITS_INC "step_fused_bits.inc"
#define LSM_DENSE_CLIP_STEPS RAGGED ? row_bits : T
#define LSM_DENSE_FEATURE_STEPS RAGGED ? Tb : ST ? Tb + a.st.t0 : T
#define LSM_DENSE_ST_OFFSET step_st_offset
#include "lif_dense_kernel.inc"
#undef LSM_DENSE_LDS_DECL
#undef LSM_DENSE_LDS
#undef LSM_DENSE_INPUT_BITS_INC
#undef LSM_DENSE_CLIP_STEPS
#undef LSM_DENSE_FEATURE_STEPS
#undef LSM_DENSE_ST_OFFSET
        if constexpr (ST) {
            // The clip's tumbling rows (lsm_segment_features with window_segments = hop_segments = 1): row g, key k, neuron o is
            // the feature of record[g][o] over seg steps.  The records are this workgroup's own stores, behind the barriers of
            // the fold and of state_finish.  (n_clips, T / seg, n_keys * n_out), key-major.
            if (sx.segment_rows != nullptr) {           // workgroup-uniform; the host gives it to a segmented launch only
                const int seg = a.st.seg, n_out = a.n_out, rows_nf = a.n_keys * n_out;
                const int n_seg = a.T / seg;
                const uint4 *rec = a.st.rec + (size_t)b * (size_t)n_seg * (size_t)n_out;
                float *rows = sx.segment_rows + (size_t)b * (size_t)n_seg * (size_t)rows_nf;
#pragma unroll 1
                for (int idx = tid; idx < n_seg * rows_nf; idx += NT) {
                    const int g = idx / rows_nf;
                    const int i = idx - g * rows_nf;
                    const int kq = i / n_out;
                    const uint4 f = rec[(size_t)g * n_out + (i - kq * n_out)];
                    rows[idx] = feature_value(a.key_ids[kq], (int)(f.x & 0xFFFFu), (int)(f.x >> 16), (int)(f.y & 0xFFFFu),
                                              (int)(f.y >> 16), f.z, f.w, seg);
                }
            }
        }
    }
}
