// Clips of different lengths in one front-end launch (SPEC.md 1.14, include/lsm_hip_ragged.h).  The kernels here are the
// RAGGED = true forms of the code that frontend.hip runs with RAGGED = false (spikes_body.h's device function,
// gammatone_spikes_kernel.inc's kernel text), in a translation unit of their own like the masked forms (mask.hip), and the
// ragged power_to_db, which has no twin to share text with.  The entry points of the two spike encoders fill a launch request
// in frontend.hip, which alone refuses, plans and builds the arguments, then calls the two launch functions below; the fused
// kernel's form is picked by the one table (launch_fused_form, gammatone_spikes_body.h).
//
// Every per-clip count is read on the device, by the kernel that uses it, and clamped there: the host never sees one.
#include "lsm_common.h"
#include "gammatone_spikes_body.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void spec_to_spikes_ragged_kernel(const lsm_fe::SpikeArgs<T> a, const lsm_fe::RaggedCounts rc)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lsm_fe::spec_to_spikes_body<T, false, true>(a, (int)blockIdx.x, smem, lsm_fe::MaskArgs{nullptr, nullptr}, rc);
}

// gammatone_spikes_ragged_kernel(const FusedArgs a, const lsm_fe::RaggedArgs rg): the fused kernel's text with RAGGED = true
#define LSM_FUSED_KERNEL gammatone_spikes_ragged_kernel
#define LSM_FUSED_QUALIFIERS __global__ __launch_bounds__(GT_MAX_WPB * 64)
#define LSM_FUSED_TAIL_INC "gammatone_spikes_raster_out.inc"
#define LSM_FUSED_PARAMS const FusedArgs a, const lsm_fe::RaggedArgs rg
#define LSM_FUSED_MASK constexpr bool MASK = false; const lsm_fe::MaskArgs m{nullptr, nullptr};
#define LSM_FUSED_RAGGED constexpr bool RAGGED = true;
#include "gammatone_spikes_kernel.inc"
#undef LSM_FUSED_KERNEL
#undef LSM_FUSED_QUALIFIERS
#undef LSM_FUSED_TAIL_INC
#undef LSM_FUSED_PARAMS
#undef LSM_FUSED_MASK
#undef LSM_FUSED_RAGGED

// this unit's kernel for the form table (gammatone_spikes_body.h, launch_fused_form)
struct RaggedFamily {
    template <int NW, bool FAST, int NCH, bool SHB0, bool PAIR>
    static auto kernel() { return gammatone_spikes_ragged_kernel<NW, FAST, NCH, SHB0, PAIR>; }
};

// librosa.power_to_db(S, ref=np.max) of clip b's first nf frames (mel.hip's power_to_db_body on rows of a stride): the
// reference maximum and the NaN rule over those frames only, columns past them written as 0.  One 256-thread workgroup.
__global__ __launch_bounds__(256) void power_to_db_ragged_kernel(const float *__restrict__ power, int n_mels, int n_frames,
                                                                 const int *__restrict__ clip_frames, float amin, float top_db,
                                                                 float *__restrict__ db_out)
{
    __shared__ float red[4];
    const int b = (int)blockIdx.x;
    const int nf = min(max(clip_frames[b], 0), n_frames);
    const float *p = power + (size_t)b * n_mels * n_frames;
    float *o = db_out + (size_t)b * n_mels * n_frames;
    const int n = n_mels * nf, total = n_mels * n_frames;
    float mx = -INFINITY;
    int nan_seen = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = i / nf;
        const float v = p[(size_t)r * n_frames + (i - r * nf)];
        mx = fmaxf(mx, v);
        nan_seen |= v != v;
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    const int any_nan = __syncthreads_or(nan_seen);       // np.max propagates NaN, fmaxf drops it (SPEC.md 1.5)
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float refdb = 10.0f * log10f(fmaxf(amin, mx));
    for (int i = threadIdx.x; i < total; i += 256) {
        const int c = i % n_frames;
        float v = 0.0f;
        if (c < nf) v = any_nan ? NAN : fmaxf(10.0f * log10f(fmaxf(amin, p[i])) - refdb, 0.0f - top_db);
        o[i] = v;
    }
}

}  // namespace

namespace lsm_fe {

template <typename T>
void launch_spec_to_spikes_ragged(const SpikeArgs<T> &a, const RaggedCounts &rc, int threads, size_t lds, void *stream)
{
    auto fn = spec_to_spikes_ragged_kernel<T>;
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
    hipLaunchKernelGGL(fn, dim3(a.n_clips), dim3(threads), lds, (hipStream_t)stream, a, rc);
}
template void launch_spec_to_spikes_ragged<double>(const SpikeArgs<double> &, const RaggedCounts &, int, size_t, void *);
template void launch_spec_to_spikes_ragged<float>(const SpikeArgs<float> &, const RaggedCounts &, int, size_t, void *);

void launch_gammatone_spikes_ragged(const FusedLaunch &l, const void *fused_args, const RaggedArgs &rg, void *stream)
{
    launch_fused_form<RaggedFamily>(l, stream, *static_cast<const FusedArgs *>(fused_args), rg);
}

}  // namespace lsm_fe

LSM_API int lsm_power_to_db_ragged_f32(const float *power, int n_clips, int n_mels, int n_frames, const int32_t *clip_frames,
                                       float amin, float top_db, float *db_out, void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_mels >= 1 && n_frames >= 1, "bad shape");
    LSM_REQUIRE((long)n_mels * n_frames <= 0x7fffffffL, "power_to_db_ragged: a clip of %d x %d values", n_mels, n_frames);
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(power && db_out, "power_to_db_ragged: null buffer");
    LSM_REQUIRE(clip_frames != nullptr, "power_to_db_ragged: null clip_frames");
    LSM_REQUIRE(((uintptr_t)clip_frames & 3u) == 0, "clip_frames must be 4-byte aligned");
    hipLaunchKernelGGL(power_to_db_ragged_kernel, dim3(n_clips), dim3(256), 0, (hipStream_t)stream, power, n_mels, n_frames,
                       clip_frames, amin, top_db, db_out);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
