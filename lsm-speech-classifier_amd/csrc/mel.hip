// Mel branch of the front end for gfx950 (SPEC.md §1.5).
//
// Replaces librosa.feature.melspectrogram(y, sr=16000, n_mels=F, hop_length=hop) and
// librosa.power_to_db(S, ref=np.max) as called at /root/reference/create_dataset.py:44-48 (librosa
// 0.11 defaults: n_fft = win_length = 2048, periodic Hann, centred frames with zero padding,
// power 2, Slaney mel basis; amin 1e-10, top_db 80).  librosa multiplies the float64 window into the
// float32 frame, transforms in float64 and stores complex64; the kernel follows the same dtypes.
// One WAVE = one frame (round 5; profiles/r05_mel_power_parts.txt: with a 256-thread workgroup per frame and five
// radix-4 passes the kernel spent 71 % of its time waiting at LDS round trips and workgroup barriers): the real-input
// FFT as 1024 complex points, sixteen per lane in registers, passes of radix 16, 16 and 4 through one 17 KB LDS
// buffer with no barrier; |.|^2 in float32; then the triangular mel filters, four lanes per filter.
#include "lsm_common.h"
#include "spikes_body.h"
#include "mel_body.h"
#include <cstdlib>

namespace {

using namespace lsm_mel;

struct MelArgs {
    const float *audio;
    int n_samples, hop, n_frames, n_mels;
    const double *window;
    const double2 *twiddle;     // W_2048^k, k < 1024
    const float *basis;
    const int *lo, *hi;
    float *power_out;
};

// frame t of clip b: centred on sample t * hop, zero padding outside the clip; its power values go to column t of the clip's rows
__device__ __forceinline__ void mel_clip_frame(const MelArgs &a, double2 *z, const int b, const int t)
{
    const Tables tab = {a.window, a.twiddle, a.basis, a.lo, a.hi, a.n_mels};
    const int n_samples = a.n_samples, n_frames = a.n_frames, n_mels = a.n_mels;
    const float *clip = a.audio + (size_t)b * n_samples;
    const int start = t * a.hop - NFFT / 2;
    float *__restrict__ power_out = a.power_out;
    mel_frame_wave(tab, z,
        [&](const int p, double &v0, double &v1) {
            // (samples outside the clip: the load goes to a clamped index and its value is dropped -- a guarded load is a branch
            //  with a wait of its own, and thirty-two of them in a row were most of this kernel's time)
            const int s0 = start + p, s1 = s0 + 1;
            const float x0 = clip[min(max(s0, 0), n_samples - 1)], x1 = clip[min(max(s1, 0), n_samples - 1)];
            v0 = (s0 >= 0 && s0 < n_samples) ? (double)x0 : 0.0;
            v1 = (s1 >= 0 && s1 < n_samples) ? (double)x1 : 0.0;
        },
        [&](const int m, const float acc) { power_out[((size_t)b * n_mels + m) * n_frames + t] = acc; });
}

// grid = (frames, clips), one wave each
__global__ __launch_bounds__(64) void mel_power_kernel(const MelArgs a)
{
    __shared__ double2 z[ZPAD];                 // 17 KB
    mel_clip_frame(a, z, (int)blockIdx.y, (int)blockIdx.x);
}

// librosa.power_to_db(S, ref=np.max): per clip, float32; one 256-thread workgroup, `red`: 4 floats of LDS.
__device__ __forceinline__ void power_to_db_body(const float *__restrict__ p, float *__restrict__ o, int n, float amin,
                                                 float top_db, float *red)
{
    float mx = -INFINITY;
    int nan_seen = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = p[i];
        mx = fmaxf(mx, v);
        nan_seen |= v != v;
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    // np.max / np.maximum propagate NaN (fmaxf drops it): one NaN power value makes the reference level, and with it every
    // dB value of the clip, NaN (librosa.power_to_db(S, ref=np.max), SPEC.md 1.5)
    const int any_nan = __syncthreads_or(nan_seen);
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (any_nan) {
        for (int i = threadIdx.x; i < n; i += 256) o[i] = NAN;
        return;
    }
    const float refdb = 10.0f * log10f(fmaxf(amin, mx));
    // the maximum of (10*log10(max(amin, S)) - refdb) is exactly 0, so the floor is -top_db
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = 10.0f * log10f(fmaxf(amin, p[i])) - refdb;
        o[i] = fmaxf(v, 0.0f - top_db);
    }
}

__global__ __launch_bounds__(256) void power_to_db_kernel(const float *__restrict__ power, int n,
                                                          float amin, float top_db,
                                                          float *__restrict__ db_out)
{
    __shared__ float red[4];
    power_to_db_body(power + (size_t)blockIdx.x * n, db_out + (size_t)blockIdx.x * n, n, amin, top_db, red);
}

// The whole mel front end of a batch in ONE launch (create_dataset.py:43-48 + :62-104 per clip): grid = (frames, clips)
// as in mel_power_kernel; every workgroup transforms its frame and projects it onto the mel filters, then counts itself
// in on its clip.  The workgroup that arrives LAST for a clip -- all of the clip's power values are in memory then --
// finishes the clip: power_to_db (the clip's maximum is the reference), min-max normalise, resize, hysteresis latches,
// raster (lsm_fe::spec_to_spikes_body, the code of the split path).  No workgroup ever waits for another one: the
// count is one atomic add whose returned value says who is last (the pattern MI355X_MICROARCH.md tabulates for a
// consumer "told by the value its add returned"; the adder's stores are made visible by the fence before the add,
// the finisher's loads are ordered by the fence after it).  The launch function zeroes the counters on the stream first.
struct MelSpikeArgs {
    MelArgs mel;                        // power_out = the power workspace (n_clips, n_mels, n_frames)
    lsm_fe::SpikeArgs<float> sp;        // db = the dB workspace, same shape: written and read by the finishing workgroup
    unsigned int *counters;             // (n_clips) zero
    float amin, top_db;
    int frames_per_wg;                  // a workgroup transforms this many consecutive frames: grid.x = ceil(n_frames / it)
};

constexpr size_t MEL_SPIKES_LDS = 4 * sizeof(double2) * ZPAD + 32;

#define LSM_MEL_KERNEL mel_spikes_kernel
#define LSM_MEL_PARAMS const MelSpikeArgs a
#define LSM_MEL_ENCODE lsm_fe::spec_to_spikes_body<float>(a.sp, b, mel_lds)
#include "mel_spikes_kernel.inc"
#undef LSM_MEL_KERNEL
#undef LSM_MEL_PARAMS
#undef LSM_MEL_ENCODE
#define LSM_MEL_KERNEL mel_spikes_masked_kernel
#define LSM_MEL_PARAMS const MelSpikeArgs a, const lsm_fe::MaskArgs m
#define LSM_MEL_ENCODE lsm_fe::spec_to_spikes_body<float, true>(a.sp, b, mel_lds, m)
#include "mel_spikes_kernel.inc"
#undef LSM_MEL_KERNEL
#undef LSM_MEL_PARAMS
#undef LSM_MEL_ENCODE

}  // namespace

LSM_API int lsm_mel_power_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop,
                              int n_frames, const double *window_dev, const double *twiddle_dev,
                              const float *basis_dev, const int32_t *lo_dev, const int32_t *hi_dev,
                              int n_mels, float *power_out, void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_samples >= 1 && hop >= 1 && n_frames >= 1 && n_mels >= 1, "bad shape");
    LSM_REQUIRE(n_fft == NFFT, "n_fft must be %d (librosa's default), got %d", NFFT, n_fft);
    LSM_REQUIRE(n_clips <= 65535, "at most 65535 clips per call (grid.y)");
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(audio && window_dev && twiddle_dev && basis_dev && lo_dev && hi_dev && power_out,
                "mel: null buffer");
    LSM_REQUIRE((((uintptr_t)window_dev | (uintptr_t)twiddle_dev) & 15u) == 0, "mel: window and twiddle tables must be 16-byte aligned");
    MelArgs a;
    a.audio = audio; a.n_samples = n_samples; a.hop = hop; a.n_frames = n_frames; a.n_mels = n_mels;
    a.window = window_dev; a.twiddle = reinterpret_cast<const double2 *>(twiddle_dev); a.basis = basis_dev;
    a.lo = lo_dev; a.hi = hi_dev; a.power_out = power_out;
    hipLaunchKernelGGL(mel_power_kernel, dim3(n_frames, n_clips), dim3(64), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API long lsm_mel_spikes_workspace(int n_clips, int n_mels, int n_frames)
{
    if (n_clips < 0 || n_mels < 1 || n_frames < 1) return 0;
    // power + dB spectrograms (float32 each) + one counter per clip, the counters first (they must start zeroed)
    return (long)(((size_t)n_clips * 4 + 255) / 256 * 256) + 2L * n_clips * n_mels * n_frames * (long)sizeof(float);
}

// lsm_mel_spikes_f32 and its masked twin (include/lsm_hip_mask.h): the same refusals and launch geometry; with a mask the
// kernel is the masked one, without one exactly the unmasked launch.
static int mel_spikes(const float *audio, int n_clips, int n_samples, int n_fft, int hop, int n_frames,
                      const double *window_dev, const double *twiddle_dev, const float *basis_dev,
                      const int32_t *lo_dev, const int32_t *hi_dev, int n_mels, float amin, float top_db,
                      int time_bins, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                      uint8_t *raster, void *workspace, long workspace_bytes, const uint32_t *freq_mask,
                      const uint32_t *time_mask, void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_samples >= 1 && hop >= 1 && n_frames >= 2 && n_mels >= 1 && time_bins >= 2, "bad shape");
    LSM_REQUIRE(n_fft == NFFT, "n_fft must be %d (librosa's default), got %d", NFFT, n_fft);
    LSM_REQUIRE(n_clips <= 65535, "at most 65535 clips per call (grid.y)");
    LSM_REQUIRE(n_thr >= 1 && n_thr <= lsm_fe::MAX_THR, "n_thr=%d outside [1, %d]", n_thr, lsm_fe::MAX_THR);
    LSM_REQUIRE(redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(thr_on && thr_off, "null threshold table");
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(audio && window_dev && twiddle_dev && basis_dev && lo_dev && hi_dev && raster && workspace,
                "mel_spikes: null buffer");
    LSM_REQUIRE((((uintptr_t)window_dev | (uintptr_t)twiddle_dev) & 15u) == 0, "mel_spikes: window and twiddle tables must be 16-byte aligned");
    LSM_REQUIRE(workspace_bytes >= lsm_mel_spikes_workspace(n_clips, n_mels, n_frames),
                "workspace of %ld bytes, need %ld (lsm_mel_spikes_workspace)", workspace_bytes,
                lsm_mel_spikes_workspace(n_clips, n_mels, n_frames));
    LSM_REQUIRE(((uintptr_t)workspace & 255u) == 0, "workspace must be 256-byte aligned");
    const int row_bytes = time_bins * n_thr;
    LSM_REQUIRE((row_bytes & 3) != 0 || ((uintptr_t)raster & 3u) == 0,
                "the raster must be 4-byte aligned when a row is a multiple of 4 bytes");
    // the finishing workgroup keeps its latch bit rows in the waves' point buffers
    const size_t stage = lsm_fe::spikes_lds_bytes(time_bins, n_thr);
    if (stage > 4 * sizeof(double2) * ZPAD) {
        lsm_set_error("mel_spikes: latch bit rows of %zu bytes exceed the kernel's %zu; use the split entry points", stage,
                      4 * sizeof(double2) * ZPAD);
        return LSM_ERR_UNSUPPORTED;
    }
    LSM_REQUIRE((((uintptr_t)freq_mask | (uintptr_t)time_mask) & 3u) == 0, "freq_mask and time_mask must be 4-byte aligned");
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const size_t cbytes = ((size_t)n_clips * 4 + 255) / 256 * 256;
    float *power = reinterpret_cast<float *>(ws + cbytes);
    float *db = power + (size_t)n_clips * n_mels * n_frames;
    MelSpikeArgs a;
    a.mel.audio = audio; a.mel.n_samples = n_samples; a.mel.hop = hop; a.mel.n_frames = n_frames; a.mel.n_mels = n_mels;
    a.mel.window = window_dev; a.mel.twiddle = reinterpret_cast<const double2 *>(twiddle_dev); a.mel.basis = basis_dev;
    a.mel.lo = lo_dev; a.mel.hi = hi_dev; a.mel.power_out = power;
    a.sp.db = db; a.sp.n_clips = n_clips; a.sp.n_filters = n_mels; a.sp.ncols = n_frames; a.sp.time_bins = time_bins;
    a.sp.apply_floor = 0;                       // the reference floors the gammatone branch only (create_dataset.py:60)
    a.sp.n_thr = n_thr; a.sp.redundancy = redundancy; a.sp.raster = raster; a.sp.norm_out = nullptr;
    for (int q = 0; q < lsm_fe::MAX_THR; ++q) { a.sp.on[q] = q < n_thr ? thr_on[q] : 0.0f; a.sp.off[q] = q < n_thr ? thr_off[q] : 0.0f; }
    a.counters = reinterpret_cast<unsigned int *>(ws);
    a.amin = amin; a.top_db = top_db;
    // Frames per workgroup (profiles/r04_mel_one_launch_ab.txt, 40 filters x 200 clips, ms per step front ends alone /
    // on one stream): 1 frame 1.72 / 1.75, 4: 0.89 / 0.79, 8: 0.58 / 0.60, 16: 0.45 / 0.54, 32: 0.36 / 0.55, the whole clip
    // (101) 0.30 / 0.90; the three split launches 0.28 / 0.33.  A batch that gives every other CU a clip takes the whole
    // clip per workgroup (best throughput when launches overlap), smaller batches 32 frames (more workgroups).
    int fpw = n_clips >= 128 ? n_frames : 32;
    fpw = fpw > n_frames ? n_frames : fpw;
    a.frames_per_wg = fpw;
    // The per-clip arrival counters are zeroed HERE, on the launch stream (4 bytes per clip; a memset node when captured): the
    // kernel resets a counter only when a clip's last workgroup arrives, so a launch that failed, or a workspace the caller
    // did not zero, would otherwise leave every later launch without a finishing workgroup.
    LSM_CHECK_HIP(hipMemsetAsync(a.counters, 0, (size_t)n_clips * sizeof(unsigned int), (hipStream_t)stream));
    if (freq_mask || time_mask) {               // SPEC.md 1.13
        lsm_allow_big_lds(reinterpret_cast<const void *>(mel_spikes_masked_kernel));
        hipLaunchKernelGGL(mel_spikes_masked_kernel, dim3((n_frames + fpw - 1) / fpw, n_clips), dim3(256), MEL_SPIKES_LDS,
                           (hipStream_t)stream, a, lsm_fe::MaskArgs{freq_mask, time_mask});
        LSM_CHECK_HIP(hipGetLastError());
        return LSM_OK;
    }
    lsm_allow_big_lds(reinterpret_cast<const void *>(mel_spikes_kernel));       // 68 KB of dynamic LDS
    hipLaunchKernelGGL(mel_spikes_kernel, dim3((n_frames + fpw - 1) / fpw, n_clips), dim3(256), MEL_SPIKES_LDS, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_mel_spikes_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop, int n_frames,
                               const double *window_dev, const double *twiddle_dev, const float *basis_dev,
                               const int32_t *lo_dev, const int32_t *hi_dev, int n_mels, float amin, float top_db,
                               int time_bins, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                               uint8_t *raster, void *workspace, long workspace_bytes, void *stream)
{
    return mel_spikes(audio, n_clips, n_samples, n_fft, hop, n_frames, window_dev, twiddle_dev, basis_dev, lo_dev, hi_dev,
                      n_mels, amin, top_db, time_bins, thr_on, thr_off, n_thr, redundancy, raster, workspace, workspace_bytes,
                      nullptr, nullptr, stream);
}

LSM_API int lsm_mel_spikes_masked_f32(const float *audio, int n_clips, int n_samples, int n_fft, int hop, int n_frames,
                                      const double *window_dev, const double *twiddle_dev, const float *basis_dev,
                                      const int32_t *lo_dev, const int32_t *hi_dev, int n_mels, float amin, float top_db,
                                      int time_bins, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                                      uint8_t *raster, void *workspace, long workspace_bytes, const uint32_t *freq_mask,
                                      const uint32_t *time_mask, void *stream)
{
    return mel_spikes(audio, n_clips, n_samples, n_fft, hop, n_frames, window_dev, twiddle_dev, basis_dev, lo_dev, hi_dev,
                      n_mels, amin, top_db, time_bins, thr_on, thr_off, n_thr, redundancy, raster, workspace, workspace_bytes,
                      freq_mask, time_mask, stream);
}

LSM_API int lsm_power_to_db_f32(const float *power, int n_clips, int n_per_clip, float amin,
                                float top_db, float *db_out, void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_per_clip >= 1, "bad shape");
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(power && db_out, "power_to_db: null buffer");
    hipLaunchKernelGGL(power_to_db_kernel, dim3(n_clips), dim3(256), 0, (hipStream_t)stream, power,
                       n_per_clip, amin, top_db, db_out);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
