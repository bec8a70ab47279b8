// One launch per step (include/lsm_hip_step.h): the lane-pair gammatone front end of a clip and the dense-row
// LIF time loop on that clip in ONE workgroup of 4 waves.  The kernel is two existing texts back to back --
// gammatone_spikes_kernel.inc in its PAIR form up to the staged raster rows, then (step_fused_tail.inc) a hand-off of the
// staged bits into the reservoir's input bit rows and lif_dense_kernel.inc in its <SL, 4, 3, true> form -- so every float
// operation and its order are those of lsm_gammatone_spikes_f64 followed by lsm_reservoir_run.  What the step no longer does:
// write the uint8 raster (13 MB per 256 clips x 128 channels x 400 steps), read it back, re-pack it with LDS atomics, and tie two
// launches of two streams with an event.  With 4 hardware queues or fewer the pipeline (pipeline.HotPath) takes this launch.
// The entry point's refusals and the arguments of the two halves are frontend.hip's and reservoir.hip's (step_front_args,
// which fills the front end's launch request in its Step form and gets the plan back instead of a launch, and
// step_dense_args); the translation unit is its own so that the existing kernels keep their machine code.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"
#include "lif_dense.h"
#include "step_fused_forms.h"
#include <cstring>

namespace {

// step_fused_kernel_sl<SL>(const FusedArgs a, const lsm_lif::DenseArgs d): one text per neuron slots per lane (N <= 256 SL,
// 4 waves).  A workgroup is one clip: 256 threads, and no more than 128 vector registers so that four launches share a SIMD.
#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(256, 4)
#define LSM_FUSED_PARAMS const FusedArgs a, const lsm_lif::DenseArgs d
#define LSM_FUSED_MASK constexpr bool MASK = false; const lsm_fe::MaskArgs m{nullptr, nullptr};
#define LSM_FUSED_RAGGED constexpr bool RAGGED = false; const lsm_fe::RaggedArgs rg{nullptr, nullptr};
#define LSM_FUSED_STATE constexpr bool ST = false; const lsm_step::StateRows sx{nullptr};
#define LSM_FUSED_TAIL_INC "step_fused_tail.inc"

#define LSM_FUSED_KERNEL step_fused_kernel_sl1
#define LSM_STEP_SL 1
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#define LSM_FUSED_KERNEL step_fused_kernel_sl2
#define LSM_STEP_SL 2
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#define LSM_FUSED_KERNEL step_fused_kernel_sl4
#define LSM_STEP_SL 4
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_STEP_SL

#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_MASK
#undef LSM_FUSED_RAGGED
#undef LSM_FUSED_STATE
#undef LSM_FUSED_TAIL_INC

typedef void (*step_fn_t)(const FusedArgs, const lsm_lif::DenseArgs);

// The forms built: 3 live windows (2 * hop < nwin <= 3 * hop: the front end's 25 ms window on its 10 ms hop), the fast
// coefficient path, with and without the shared b0.  Not the shared form table (launch_fused_form): these are three kernel
// texts, one per SL, in two forms each, and the table would instantiate all eight forms of every one.
step_fn_t pick_step(int sl, bool shb0)
{
    switch (sl) {
    case 1: return shb0 ? step_fused_kernel_sl1<3, true, 1, true, true> : step_fused_kernel_sl1<3, true, 1, false, true>;
    case 2: return shb0 ? step_fused_kernel_sl2<3, true, 1, true, true> : step_fused_kernel_sl2<3, true, 1, false, true>;
    case 4: return shb0 ? step_fused_kernel_sl4<3, true, 1, true, true> : step_fused_kernel_sl4<3, true, 1, false, true>;
    default: return nullptr;
    }
}

// What the shape alone decides about the front-end half (the launch checks the rest): lane pair of exactly 4 waves per clip,
// one raster row per filter, the forms above.
bool front_shape_served(int n_filters, int nwin, int hop, int redundancy, int coef_flags)
{
    return n_filters > 96 && n_filters <= 128 && redundancy == 1 && hop >= 1 && nwin >= 1 && (nwin + hop - 1) / hop == 3 &&
           (coef_flags & 3) == 3;
}

// The step's LDS image: the front end's exchange doubles and staged rows (4 waves of 32 rows of RW words), the reservoir's
// image behind them, and the 128 bytes of the inverse channel permutation behind the input bit rows.
size_t step_lds_bytes(long T, size_t lif_lds)
{
    const size_t RW = ((size_t)T + 31) / 32;
    return 2 * GT_MAX_WPB * sizeof(double) + 4 * 32 * RW * 4 + lif_lds + 128;
}
constexpr size_t STEP_LDS_MAX = 160 * 1024;

// The three families of the step (include/lsm_hip_step.h): the plain kernels above, the masked ones (step_fused_masked.hip)
// and the ragged ones (step_fused_ragged.hip).  A batch that is both takes a fourth family (step_fused_ragged_masked.hip).
// STEP_STATE (include/lsm_hip_step_state.h, step_fused_state.hip) is no `form` of lsm_step_fused_form_supported: its entry
// points and its query are their own, its served set is the plain step's.
// STEP_RAGGED_MASKED (include/lsm_hip_ragged_augment.h, step_fused_ragged_masked.hip) is none either: its query is its own,
// its served set is the ragged step's.
enum StepForm { STEP_PLAIN = 0, STEP_MASKED = 1, STEP_RAGGED = 2, STEP_STATE = 3, STEP_RAGGED_MASKED = 4 };
constexpr int RAGGED_HOP = 160;         // the one hop the ragged front end is offered for (include/lsm_hip_ragged.h)

// What a form asks of the shape beyond the plain step: the ragged step the hop on which a clip of T bins is the front end of
// (160 T samples, T bins).  The LDS image is step_lds_bytes for every form.
bool form_shape_served(int form, int hop)
{
    return form != STEP_RAGGED || hop == RAGGED_HOP;
}

int step_supported(const char *what, const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                   int n_thr, int redundancy, int coef_flags, int form)
{
    LSM_REQUIRE(h != nullptr, "%s: null reservoir handle", what);
    LSM_REQUIRE(n_clips >= 1 && n_filters >= 1 && time_bins >= 1 && n_thr >= 1 && redundancy >= 1, "bad shape");
    LSM_REQUIRE(form >= STEP_PLAIN && form <= STEP_RAGGED, "%s: form %d is none of 0 (plain), 1 (masked), 2 (ragged)", what, form);
    if (!front_shape_served(n_filters, nwin, hop, redundancy, coef_flags) || !form_shape_served(form, hop)) return 0;
    if ((long)time_bins * n_thr > 65535) return 0;
    lsm_lif::DenseArgs d;
    int sl = 0;
    size_t lds = 0;
    if (lsm_lif::step_dense_args(h, n_clips, time_bins * n_thr, nullptr, 0, nullptr, nullptr, true, &d, &sl, &lds) != LSM_OK)
        return 0;
    if (d.C != n_filters * redundancy) return 0;
    return step_lds_bytes((long)time_bins * n_thr, lds) <= STEP_LDS_MAX ? 1 : 0;
}

// One step launch: the six entry points fill `form` and their own members (a member that is not the form's is never read).
// Refusals: the front end's, the reservoir's (a state step: lsm_reservoir_run_from's / _run_segments'), the form's own (the
// masks' alignment; the ragged counts and strides; the segment rows), then the shapes the launch does not serve.
struct StepOwn {
    int form = STEP_PLAIN;
    const char *what = "lsm_step_fused_f64";
    const uint32_t *freq_mask = nullptr, *time_mask = nullptr;     // Masked (SPEC.md 1.13), Ragged masked (1.16)
    const int32_t *clip_bins = nullptr;                             // Ragged (1.14), Ragged masked: DEVICE counts, clamped in the kernel
    lsm_lif::StepState state;                                       // State (4f): continuation and segment records
    float *segment_rows = nullptr;                                  //   the clip's tumbling feature rows, or null
};

int step_launch(const StepOwn &own, const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs,
                int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on, const double *thr_off,
                int n_thr, int redundancy, void *workspace, long workspace_bytes, int coef_flags, const int32_t *key_ids,
                int n_keys, float *features_out, int32_t *stats_out, void *stream)
{
    const char *const what = own.what;
    // what the caller of an unserved shape does instead: a state step's alternative may be three launches (the segment fold)
    const char *const instead = own.form == STEP_STATE ? "make the separate launches" : "make the two launches";
    LSM_REQUIRE(h != nullptr, "%s: null reservoir handle", what);
    LSM_REQUIRE(n_clips >= 0, "bad shape");
    if (n_clips == 0) return LSM_OK;
    // A step of more steps than the reservoir's records hold, or whose LDS image cannot fit a CU whatever the reservoir (every
    // reservoir image holds the step's 4 input words, 16 bytes a step), is a shape lsm_step_fused_supported answers with 0:
    // refused as such here, ahead of the two halves, which call the same sizes bad arguments (the front end its stage alone,
    // the reservoir n_steps and an image of its own past 160 KB).  What passes leaves both halves room; the whole image is
    // looked at below.
    if (time_bins >= 1 && n_thr >= 1) {
        const long steps = (long)time_bins * n_thr;
        if (steps > 65535 || step_lds_bytes(steps, 16 * (size_t)steps) > STEP_LDS_MAX) {
            lsm_set_error("%s: shape not served (%d bins x %d thresholds = %ld steps: at most 65535, and an LDS "
                          "image of at most %zu bytes): %s", what, time_bins, n_thr, steps, STEP_LDS_MAX, instead);
            return LSM_ERR_UNSUPPORTED;
        }
    }
    lsm_fe::StepFront fr;
    if (const int rc = lsm_fe::step_front_args(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on,
                                               thr_off, n_thr, redundancy, workspace, workspace_bytes, coef_flags, &fr))
        return rc;
    FusedArgs a;
    memcpy(&a, fr.args, sizeof a);
    const int T = time_bins * n_thr;
    lsm_lif::DenseArgs d;
    int sl = 0;
    size_t lif_lds = 0;
    if (const int rc = lsm_lif::step_dense_args(h, n_clips, T, key_ids, n_keys, features_out, stats_out, false, &d, &sl, &lif_lds,
                                                own.form == STEP_STATE ? &own.state : nullptr))
        return rc;
    // the form's own refusals, behind the two halves'
    if (own.form == STEP_MASKED) {
        if (const int rc = lsm_fe::step_check_masks(own.freq_mask, own.time_mask)) return rc;
    } else if (own.form == STEP_RAGGED || own.form == STEP_RAGGED_MASKED) {
        if (const int rc = lsm_fe::step_check_ragged(own.clip_bins, time_bins, n_samples, hop)) return rc;
        if (const int rc = lsm_fe::step_check_masks(own.freq_mask, own.time_mask)) return rc;      // (a ragged step: both null)
    } else if (own.form == STEP_STATE) {
        LSM_REQUIRE((reinterpret_cast<uintptr_t>(own.segment_rows) & 3) == 0, "segment_rows_out must be 4-byte aligned");
        LSM_REQUIRE(own.segment_rows == nullptr || n_keys >= 1, "segment_rows_out with n_keys=0: a row needs feature keys");
    }
    // a masked step without a mask is the plain launch (SPEC.md 1.13: the unmasked bytes), and so is a state step from reset
    // that saves no state and closes no records (SPEC.md 4f)
    const bool stateless = own.form == STEP_STATE && !own.state.state_in && !own.state.state_out && !own.state.segmented;
    // a masked ragged step without a mask is the ragged launch
    const bool maskless = !own.freq_mask && !own.time_mask;
    const int form = ((own.form == STEP_MASKED && maskless) || stateless) ? (int)STEP_PLAIN
                     : (own.form == STEP_RAGGED_MASKED && maskless)      ? (int)STEP_RAGGED
                                                                         : own.form;
    step_fn_t fn = pick_step(sl, fr.l.shb0);
    if (!front_shape_served(n_filters, nwin, hop, redundancy, coef_flags) || !fr.l.pair || fr.l.nch != 1 || !fr.l.fast ||
        fr.l.nw != 3 || a.groups != 4 || fr.l.block != 256 || fr.l.grid != (unsigned)n_clips || d.C != n_filters * redundancy ||
        d.CW != 4 || d.T != T || fn == nullptr) {
        lsm_set_error("%s: shape not served (%d filters, redundancy %d, nwin %d, hop %d, coef_flags %d, %d input "
                      "channels): %s", what, n_filters, redundancy, nwin, hop, coef_flags, d.C, instead);
        return LSM_ERR_UNSUPPORTED;
    }
    // ragged: a clip of t bins has t - (time_bins - ncols) columns; on hop 160 with the 2 columns a 25 ms window costs, that
    // is the front end of (160 t samples, t bins) for every t (include/lsm_hip_ragged.h)
    const bool ragged = own.form == STEP_RAGGED || own.form == STEP_RAGGED_MASKED;
    if (ragged && (!form_shape_served(STEP_RAGGED, hop) || ncols != time_bins - 2)) {
        lsm_set_error("%s: shape not served (hop %d, %d columns for %d bins: a ragged step needs hop %d and time_bins - 2 "
                      "columns): make the two launches", what, hop, ncols, time_bins, RAGGED_HOP);
        return LSM_ERR_UNSUPPORTED;
    }
    // the front end's image (fr.l.lds, a multiple of 16) is step_lds_bytes' first two terms
    const size_t lds = step_lds_bytes(T, lif_lds);
    LSM_REQUIRE((fr.l.lds & 15) == 0 && fr.l.lds + lif_lds + 128 == lds, "the step's LDS image is not %zu bytes", lds);
    if (lds > STEP_LDS_MAX) {
        lsm_set_error("%s: shape not served (%d steps: an LDS image of %zu bytes, at most %zu): %s", what, T, lds,
                      STEP_LDS_MAX, instead);
        return LSM_ERR_UNSUPPORTED;
    }
    if (form == STEP_PLAIN) {
        if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
        hipLaunchKernelGGL(fn, dim3(fr.l.grid), dim3(fr.l.block), lds, (hipStream_t)stream, a, d);
    } else {
        // (pick_step has said that this sl has a kernel: the families build the same three)
        const lsm_step::StepLaunch l{sl, fr.l.shb0, fr.l.grid, fr.l.block, lds};
        const bool ok = form == STEP_MASKED
                            ? lsm_step::launch_step_masked(l, &a, d, lsm_fe::MaskArgs{own.freq_mask, own.time_mask}, stream)
                        : form == STEP_RAGGED
                            ? lsm_step::launch_step_ragged(l, &a, d, lsm_fe::RaggedArgs{own.clip_bins, nullptr}, stream)
                        : form == STEP_RAGGED_MASKED
                            ? lsm_step::launch_step_ragged_masked(
                                  l, &a, d,
                                  lsm_step::RaggedMaskArgs{lsm_fe::RaggedArgs{own.clip_bins, nullptr},
                                                           lsm_fe::MaskArgs{own.freq_mask, own.time_mask}},
                                  stream)
                            : lsm_step::launch_step_state(l, &a, d, lsm_step::StateRows{own.segment_rows}, stream);
        LSM_REQUIRE(ok, "%s: no kernel for %d slots per lane", what, sl);
    }
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

}  // namespace

LSM_API int lsm_step_fused_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                                     int n_thr, int redundancy, int coef_flags)
{
    return step_supported("lsm_step_fused_supported", h, n_clips, n_filters, nwin, hop, time_bins, n_thr, redundancy, coef_flags,
                          STEP_PLAIN);
}

LSM_API int lsm_step_fused_form_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                                          int n_thr, int redundancy, int coef_flags, int form)
{
    return step_supported("lsm_step_fused_form_supported", h, n_clips, n_filters, nwin, hop, time_bins, n_thr, redundancy,
                          coef_flags, form);
}

LSM_API int lsm_step_fused_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs,
                               int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on,
                               const double *thr_off, int n_thr, int redundancy, void *workspace, long workspace_bytes,
                               int coef_flags, const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out,
                               void *stream)
{
    return step_launch(StepOwn{}, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                       n_thr, redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}

LSM_API int lsm_step_fused_masked_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                      const double *coefs, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                      const double *thr_on, const double *thr_off, int n_thr, int redundancy, void *workspace,
                                      long workspace_bytes, int coef_flags, const int32_t *key_ids, int n_keys,
                                      float *features_out, int32_t *stats_out, const uint32_t *freq_mask,
                                      const uint32_t *time_mask, void *stream)
{
    StepOwn own;
    own.form = STEP_MASKED; own.what = "lsm_step_fused_masked_f64"; own.freq_mask = freq_mask; own.time_mask = time_mask;
    return step_launch(own, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off, n_thr,
                       redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}

LSM_API int lsm_step_fused_ragged_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                      const double *coefs, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                      const int32_t *clip_bins, const double *thr_on, const double *thr_off, int n_thr,
                                      int redundancy, void *workspace, long workspace_bytes, int coef_flags,
                                      const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out, void *stream)
{
    StepOwn own;
    own.form = STEP_RAGGED; own.what = "lsm_step_fused_ragged_f64"; own.clip_bins = clip_bins;
    return step_launch(own, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off, n_thr,
                       redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}

// include/lsm_hip_ragged_augment.h (SPEC.md 1.16): the ragged step with the masked step's words
LSM_API int lsm_step_fused_ragged_masked_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop,
                                                   int time_bins, int n_thr, int redundancy, int coef_flags)
{
    // the ragged step's served set and LDS bound: the masks add no byte to the image
    return step_supported("lsm_step_fused_ragged_masked_supported", h, n_clips, n_filters, nwin, hop, time_bins, n_thr,
                          redundancy, coef_flags, STEP_RAGGED);
}

LSM_API int lsm_step_fused_ragged_masked_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                             const double *coefs, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                             const int32_t *clip_bins, const double *thr_on, const double *thr_off, int n_thr,
                                             int redundancy, void *workspace, long workspace_bytes, int coef_flags,
                                             const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out,
                                             const uint32_t *freq_mask, const uint32_t *time_mask, void *stream)
{
    StepOwn own;
    own.form = STEP_RAGGED_MASKED; own.what = "lsm_step_fused_ragged_masked_f64"; own.clip_bins = clip_bins;
    own.freq_mask = freq_mask; own.time_mask = time_mask;
    return step_launch(own, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off, n_thr,
                       redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}

LSM_API int lsm_step_fused_state_supported(const lsm_reservoir *h, int n_clips, int n_filters, int nwin, int hop, int time_bins,
                                           int n_thr, int redundancy, int coef_flags)
{
    // the plain step's served set and LDS bound: the ST form adds no byte to the image (its scratch is the idle count array)
    return step_supported("lsm_step_fused_state_supported", h, n_clips, n_filters, nwin, hop, time_bins, n_thr, redundancy,
                          coef_flags, STEP_PLAIN);
}

LSM_API int lsm_step_fused_from_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples, const double *coefs,
                                    int n_filters, int nwin, int hop, int ncols, int time_bins, const double *thr_on,
                                    const double *thr_off, int n_thr, int redundancy, void *workspace, long workspace_bytes,
                                    int coef_flags, int first_step, const void *state_in, void *state_out,
                                    const int32_t *key_ids, int n_keys, float *features_out, int32_t *stats_out, void *stream)
{
    StepOwn own;
    own.form = STEP_STATE; own.what = "lsm_step_fused_from_f64";
    own.state.first_step = first_step; own.state.state_in = state_in; own.state.state_out = state_out;
    return step_launch(own, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off, n_thr,
                       redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}

LSM_API int lsm_step_fused_segments_f64(const lsm_reservoir *h, const float *audio, int n_clips, int n_samples,
                                        const double *coefs, int n_filters, int nwin, int hop, int ncols, int time_bins,
                                        const double *thr_on, const double *thr_off, int n_thr, int redundancy, void *workspace,
                                        long workspace_bytes, int coef_flags, int first_step, const void *state_in,
                                        void *state_out, const int32_t *key_ids, int n_keys, float *features_out,
                                        int32_t *stats_out, int segment_steps, void *records_out, float *segment_rows_out,
                                        void *stream)
{
    StepOwn own;
    own.form = STEP_STATE; own.what = "lsm_step_fused_segments_f64";
    own.state.first_step = first_step; own.state.state_in = state_in; own.state.state_out = state_out;
    own.state.segmented = true; own.state.segment_steps = segment_steps; own.state.records = records_out;
    own.segment_rows = segment_rows_out;
    return step_launch(own, h, audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off, n_thr,
                       redundancy, workspace, workspace_bytes, coef_flags, key_ids, n_keys, features_out, stats_out, stream);
}
