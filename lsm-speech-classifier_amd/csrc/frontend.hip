// Front end for gfx950: gammatone filterbank -> dB -> min-max normalise -> linear resize ->
// hysteresis spike encoder (SPEC.md §1).
//
// Replaces /root/reference/create_dataset.py:49-60 (gammatone branch of audio_to_spectrogram,
// arithmetic in gammatone==1.0.3 / scipy.signal.lfilter), :62-78 (normalise, zoom, crop),
// :81-98 (convert_spectrogram_to_spikes_hysteresis) and :101-104 (create_pure_redundancy),
// batched over clips.  Every float operation is written in the reference's order and compiled
// with -ffp-contract=off so that results equal the CPU oracle bit for bit (log10 excepted: no
// two libms agree on its last bit).
#include "lsm_common.h"
#include "gammatone_body.h"
#include "spikes_body.h"
#include "gammatone_spikes_body.h"
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------------------------
// Gammatone spectrogram.  One lane = one channel, one wave = 64 channels of ONE clip, so the audio
// sample is wave-uniform and arrives through scalar loads (8 samples per fetch, next chunk
// requested before the current one is consumed).  Per sample: four cascaded second-order
// sections in float64 evaluated like scipy.signal.lfilter (direct form II transposed), / gain,
// squared, then per column the sequential ascending sum of nwin samples, / nwin, sqrt.  Up to
// NWIN_MAX overlapping windows are live at once (nwin <= NWIN_MAX * hop); they sit in named
// registers that shift by one at every hop boundary.  Serial in time, parallel over clips x
// channels: bound by float64 VALU issue (~36 operations per sample), not by memory.
//
// The coefficient load, the section step, the quotient by a reciprocal and the exactness notes (B2ZERO, FASTDIV) are in
// gammatone_body.h.
// ---------------------------------------------------------------------------------------------
// (NWIN_MAX and GT_MAX_WPB, the waves per workgroup at most: gammatone_spikes_body.h)

// NW = ceil(nwin / hop) windows are live at any sample.  In every hop block exactly one window
// completes: the one of age NW-1, after sample number pos = nwin - (NW-1)*hop of the block.  So a
// block is: [0, pos) with NW windows accumulating, finalise, [pos, hop) with NW-1, rotate.
template <int NW, bool B2ZERO, bool FASTDIV>
__global__ __launch_bounds__(GT_MAX_WPB * 64) void gammatone_kernel(
    const float *__restrict__ audio, int n_clips, int n_samples,
    const double *__restrict__ coefs, int n_filters, int nwin, int hop, int ncols,
    double *__restrict__ spec_out, double *__restrict__ db_out)
{
    // one wave = 64 channels of one clip; the waves of a workgroup are consecutive (clip, channel
    // group) pairs.  A workgroup of 4 waves occupies each SIMD of its CU once: single-wave workgroups
    // are packed by the dispatcher up to the occupancy limit of a CU before the next CU is used
    // (2048 of them ran on half the chip, 3.7 ms instead of 2.6 ms at 1024 clips).
    const int groups = (n_filters + 63) >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(
        (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int b = wid / groups;
    if (b >= n_clips) return;                            // wave-uniform; the kernel has no barrier
    const int chl = (wid - b * groups) * 64 + (int)(threadIdx.x & 63);
    const bool live = chl < n_filters;
    const int ch = live ? chl : n_filters - 1;
    const lsm_gt::Sections s = lsm_gt::load_sections(coefs, ch);
    const double b0 = s.b0, b2 = s.b2, b11 = s.b1[0], b12 = s.b1[1], b13 = s.b1[2], b14 = s.b1[3];
    const double a1 = s.a1, a2 = s.a2, gain = s.gain, rgain = s.rgain;
    const float *__restrict__ x = audio + (size_t)b * n_samples;      // wave-uniform

    double z01 = 0, z11 = 0, z02 = 0, z12 = 0, z03 = 0, z13 = 0, z04 = 0, z14 = 0;
    double win[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) win[q] = 0.0;

    auto filt = [&](float xf) -> double {
        const double x0 = (double)xf;
        const double y1 = lsm_gt::section<B2ZERO>(z01, b0, x0, z11, b11, a1, a2, b2);
        const double y2 = lsm_gt::section<B2ZERO>(z02, b0, y1, z12, b12, a1, a2, b2);
        const double y3 = lsm_gt::section<B2ZERO>(z03, b0, y2, z13, b13, a1, a2, b2);
        const double y4 = lsm_gt::section<B2ZERO>(z04, b0, y3, z14, b14, a1, a2, b2);
        double o;
        lsm_gt::quot<FASTDIV>(o, y4, gain, rgain);
        return o * o;
    };
    // samples [n, n_to) with the NACT youngest windows accumulating; the scalar load of the next
    // 8 samples is issued before the current 8 are consumed (clamped inside the clip: the extra chunk
    // at the end of a run is loaded but never used)
#define LSM_RUN(n_to, NACT)                                                         \
    {                                                                               \
        if (n + 8 <= (n_to)) {                                                      \
            float xs[8], nx[8];                                                     \
            _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = x[n + u];         \
            for (; n + 8 <= (n_to); n += 8) {                                       \
                const float *pn = x + min(n + 8, n_samples - 8);                    \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) nx[u] = pn[u];        \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) {                     \
                    const double e = filt(xs[u]);                                   \
                    _Pragma("unroll") for (int q = 0; q < (NACT); ++q) win[q] += e; \
                }                                                                   \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = nx[u];        \
            }                                                                       \
        }                                                                           \
        for (; n < (n_to); ++n) {                                                   \
            const double e = filt(x[n]);                                            \
            _Pragma("unroll") for (int q = 0; q < (NACT); ++q) win[q] += e;         \
        }                                                                           \
    }

    const int pos = nwin - (NW - 1) * hop;               // in (0, hop]
    const int n_end = (ncols - 1) * hop + nwin;          // samples past this feed no column
    const double dn = (double)nwin;
    const size_t obase = ((size_t)b * n_filters + ch) * ncols;
    int n = 0;
    for (int h = 0; n < n_end; ++h) {
        const int base = h * hop;
        const int mid = min(base + pos, n_end);
        LSM_RUN(mid, NW)
        const int c = h - (NW - 1);                      // the column that just completed
        if (n == base + pos && c >= 0 && c < ncols) {
            const double y = sqrt(win[NW - 1] / dn);
            if (live) {
                if (spec_out) spec_out[obase + c] = y;
                if (db_out) db_out[obase + c] = 20 * log10(y + 1e-9);
            }
        }
        const int stop = min(base + hop, n_end);
        LSM_RUN(stop, NW - 1)
#pragma unroll
        for (int q = NW - 1; q > 0; --q) win[q] = win[q - 1];
        win[0] = 0.0;
    }
#undef LSM_RUN
}

// ---------------------------------------------------------------------------------------------
// Per clip: floor (optional) -> min/max -> normalise -> linear resize to time_bins -> hysteresis
// encoder -> uint8 raster (n_filters*redundancy, time_bins*n_thr), staged in LDS and written out
// with coalesced 4-byte stores.  One workgroup of 256 threads per clip; a thread owns a channel
// for the serial part (time_bins x n_thr latch updates).
// ---------------------------------------------------------------------------------------------
using lsm_fe::MAX_THR;
using lsm_fe::fill_thresholds;
using lsm_fe::SpikeArgs;

// Threads of a spec_to_spikes_kernel workgroup (one clip).  Alone on the GPU sixteen waves are faster than four (21.5 against
// 32.7 us per 200 clips: with one wave per SIMD every dependent instruction waits out its latency), inside the overlapped
// pipeline the small workgroup is (cfg1: 1.26-1.29 M clips/s with 256 threads, 1.22-1.26 M with 512, 1.13-1.15 M with 1024,
// which must find a whole CU's wave slots free; profiles/r05_mel_wave_per_frame.txt)
constexpr int SPK_THREADS = 256;
template <typename T>
__global__ __launch_bounds__(SPK_THREADS) void spec_to_spikes_kernel(const SpikeArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lsm_fe::spec_to_spikes_body<T>(a, (int)blockIdx.x, smem);
}

// The fused front end (gammatone_spikes_kernel: filterbank to raster in one launch) has its body in gammatone_spikes_body.h.

// Stand-alone encoder on an already normalised spectrogram (B, F, n_bins): one lane per channel.
template <typename T>
__global__ __launch_bounds__(64) void encode_kernel(const T *__restrict__ spec, int n_rows,
                                                    int n_bins, int n_thr, SpikeArgs<T> thr,
                                                    uint8_t *__restrict__ out)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    const T *row = spec + (size_t)r * n_bins;
    uint8_t *o = out + (size_t)r * n_bins * n_thr;
    bool active[MAX_THR];
#pragma unroll
    for (int q = 0; q < MAX_THR; ++q) active[q] = false;
    for (int j = 0; j < n_bins; ++j) {
        const T val = row[j];
#pragma unroll
        for (int q = 0; q < MAX_THR; ++q) {
            if (q < n_thr) {
                const bool rising = (val > thr.on[q]) && !active[q];
                const bool falling = (val < thr.off[q]) && active[q];
                if (rising) active[q] = true;
                if (falling) active[q] = false;
                o[j * n_thr + q] = active[q] ? 1 : 0;
            }
        }
    }
}

// The masked entry points' own refusal, after their twins' (include/lsm_hip_mask.h)
int check_masks(const uint32_t *freq_mask, const uint32_t *time_mask)
{
    LSM_REQUIRE((((uintptr_t)freq_mask | (uintptr_t)time_mask) & 3u) == 0, "freq_mask and time_mask must be 4-byte aligned");
    return LSM_OK;
}

// The ragged entry points' own refusals, after their twins' (include/lsm_hip_ragged.h): the count arrays, then the strides
int check_ragged(const void *counts_a, const void *counts_b, int time_bins, long n_samples, long hop)
{
    LSM_REQUIRE(counts_a != nullptr && counts_b != nullptr, "ragged: null per-clip count array");
    LSM_REQUIRE((((uintptr_t)counts_a | (uintptr_t)counts_b) & 3u) == 0, "ragged: per-clip count arrays must be 4-byte aligned");
    LSM_REQUIRE(time_bins >= 3, "ragged: time_bins=%d, a clip has at least 3 time bins", time_bins);
    LSM_REQUIRE(n_samples >= hop * time_bins, "ragged: rows of %ld samples, need hop * time_bins = %ld", n_samples,
                hop * time_bins);
    return LSM_OK;
}

// Which launch an export of the two spike encoders asks for: the export's own choice, never inferred from pointers -- but a
// masked export given two null masks makes exactly the plain launch (include/lsm_hip_mask.h).
enum class FrontForm { Plain, Masked, Ragged, Step };

// One launch of spec_to_spikes: every lsm_spec_to_spikes_* export fills the members by name (split_request, then its form's),
// launch_spec_to_spikes refuses in one order and launches.  A member that is not the form's is never read.
template <typename T>
struct SplitRequest {
    FrontForm form = FrontForm::Plain;
    const T *db = nullptr, *thr_on = nullptr, *thr_off = nullptr;
    int n_clips = 0, n_filters = 0, ncols = 0, time_bins = 0, apply_floor = 0, n_thr = 0, redundancy = 0;
    uint8_t *raster = nullptr;
    T *norm_out = nullptr;
    void *stream = nullptr;
    const uint32_t *freq_mask = nullptr, *time_mask = nullptr;     // Masked (SPEC.md 1.13), and Ragged with masks (1.16)
    const int32_t *clip_cols = nullptr, *clip_bins = nullptr;      // Ragged (1.14): DEVICE counts; ncols, time_bins the strides
};

template <typename T>           // what all eight exports are given
SplitRequest<T> split_request(const T *db, int n_clips, int n_filters, int ncols, int time_bins, int apply_floor,
                              const T *thr_on, const T *thr_off, int n_thr, int redundancy, uint8_t *raster, T *norm_out,
                              void *stream)
{
    SplitRequest<T> r;
    r.db = db; r.n_clips = n_clips; r.n_filters = n_filters; r.ncols = ncols; r.time_bins = time_bins;
    r.apply_floor = apply_floor; r.thr_on = thr_on; r.thr_off = thr_off; r.n_thr = n_thr; r.redundancy = redundancy;
    r.raster = raster; r.norm_out = norm_out; r.stream = stream;
    return r;
}

template <typename T>
int launch_spec_to_spikes(const SplitRequest<T> &r)
{
    LSM_REQUIRE(r.n_clips >= 0 && r.n_filters >= 1 && r.ncols >= 2 && r.time_bins >= 2, "bad shape");
    LSM_REQUIRE(r.db != nullptr || r.n_clips == 0, "spec_to_spikes: null input");
    LSM_REQUIRE(r.n_thr >= 0 && r.n_thr <= MAX_THR, "n_thr=%d outside [0, %d]", r.n_thr, MAX_THR);
    LSM_REQUIRE(r.redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(r.n_thr == 0 || (r.thr_on && r.thr_off), "null threshold table");
    LSM_REQUIRE(r.raster == nullptr || r.n_thr >= 1, "a raster needs at least one threshold");
    if (r.n_clips == 0) return LSM_OK;
    SpikeArgs<T> a;
    a.db = r.db; a.n_clips = r.n_clips; a.n_filters = r.n_filters; a.ncols = r.ncols;
    a.time_bins = r.time_bins; a.apply_floor = r.apply_floor; a.n_thr = r.n_thr;
    a.redundancy = r.redundancy; a.raster = r.raster; a.norm_out = r.norm_out;
    fill_thresholds<T>(a.on, a.off, r.thr_on, r.thr_off, r.n_thr, (T)0, (T)0);
    const size_t lds = lsm_fe::spikes_lds_bytes(r.time_bins, r.n_thr);
    LSM_REQUIRE(lds <= 160 * 1024, "latch bit rows of %zu bytes (time_bins x thresholds) exceed one CU's LDS", lds);
    if (r.form == FrontForm::Masked && (r.freq_mask || r.time_mask)) {     // without a mask the launch is the plain one
        if (const int rc = check_masks(r.freq_mask, r.time_mask)) return rc;
        lsm_fe::launch_spec_to_spikes_masked<T>(a, lsm_fe::MaskArgs{r.freq_mask, r.time_mask}, SPK_THREADS, lds, r.stream);
    } else if (r.form == FrontForm::Ragged) {
        if (const int rc = check_ragged(r.clip_cols, r.clip_bins, r.time_bins, 0, 0)) return rc;
        // the masked ragged exports' own refusal behind the ragged twin's (include/lsm_hip_ragged_augment.h; the ragged
        // exports leave both masks null); without a mask exactly the ragged launch
        if (const int rc = check_masks(r.freq_mask, r.time_mask)) return rc;
        const lsm_fe::RaggedCounts counts{r.clip_cols, r.clip_bins};
        if (r.freq_mask || r.time_mask)
            lsm_fe::launch_spec_to_spikes_ragged_masked<T>(a, counts, lsm_fe::MaskArgs{r.freq_mask, r.time_mask}, SPK_THREADS, lds,
                                                           r.stream);
        else
            lsm_fe::launch_spec_to_spikes_ragged<T>(a, counts, SPK_THREADS, lds, r.stream);
    } else {
        auto fn = spec_to_spikes_kernel<T>;
        if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
        hipLaunchKernelGGL(fn, dim3(r.n_clips), dim3(SPK_THREADS), lds, (hipStream_t)r.stream, a);
    }
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

template <typename T>
int launch_encode(const T *spec, int n_rows, int n_bins, const T *thr_on, const T *thr_off,
                  int n_thr, uint8_t *out, void *stream)
{
    LSM_REQUIRE(n_rows >= 0 && n_bins >= 1, "encode: bad shape (%d rows, %d bins)", n_rows, n_bins);
    LSM_REQUIRE(n_thr >= 1 && n_thr <= MAX_THR, "n_thr=%d outside [1, %d]", n_thr, MAX_THR);
    if (n_rows == 0) return LSM_OK;
    LSM_REQUIRE(spec && out && thr_on && thr_off, "encode: null buffer");
    SpikeArgs<T> a{};
    fill_thresholds<T>(a.on, a.off, thr_on, thr_off, n_thr, (T)0, (T)0);
    hipLaunchKernelGGL(encode_kernel<T>, dim3((n_rows + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       spec, n_rows, n_bins, n_thr, a, out);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

// Bit-packed rasters (File 1, packed variant): byte q of a row holds time steps 8q..8q+7, step 8q+k in
// bit k.  One thread per packed byte; rows whose length is a multiple of 8 move 8 raster bytes per
// thread as one 64-bit access (a wave then touches 512 contiguous raster bytes and 64 packed ones).
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t *__restrict__ raster,
                                                        long n_rows, int T, int TP,
                                                        uint8_t *__restrict__ packed)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * TP) return;
    const long r = i / TP;
    const int q = (int)(i - r * TP);
    const uint8_t *src = raster + r * T + (long)q * 8;
    uint32_t byte = 0;
    if ((T & 7) == 0) {
        const uint2 v = *reinterpret_cast<const uint2 *>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            byte |= ((v.x >> (8 * k)) & 0xFFu) ? (1u << k) : 0u;
            byte |= ((v.y >> (8 * k)) & 0xFFu) ? (1u << (k + 4)) : 0u;
        }
    } else {
        for (int k = 0; k < 8 && q * 8 + k < T; ++k) byte |= src[k] ? (1u << k) : 0u;
    }
    packed[i] = (uint8_t)byte;
}

__global__ __launch_bounds__(256) void unpack_bits_kernel(const uint8_t *__restrict__ packed,
                                                          long n_rows, int T, int TP,
                                                          uint8_t *__restrict__ raster)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * TP) return;
    const long r = i / TP;
    const int q = (int)(i - r * TP);
    const uint32_t byte = packed[i];
    uint8_t *dst = raster + r * T + (long)q * 8;
    if ((T & 7) == 0) {
        uint2 v;
        v.x = (byte & 1u) | ((byte & 2u) << 7) | ((byte & 4u) << 14) | ((byte & 8u) << 21);
        v.y = ((byte >> 4) & 1u) | ((byte & 32u) << 3) | ((byte & 64u) << 10) | ((byte & 128u) << 17);
        *reinterpret_cast<uint2 *>(dst) = v;
    } else {
        for (int k = 0; k < 8 && q * 8 + k < T; ++k) dst[k] = (uint8_t)((byte >> k) & 1u);
    }
}

}  // namespace

// CU count and LDS per CU of the current device (queried once per device)
struct DevInfo { int cus; long lds_per_cu; };
static DevInfo dev_info()
{
    constexpr int MAXDEV = 64;
    static DevInfo tab[MAXDEV];
    static std::once_flag once[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) {
        (void)hipGetLastError();
        return DevInfo{0, 0};
    }
    std::call_once(once[dev], [dev] {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
            tab[dev] = DevInfo{prop.multiProcessorCount, (long)prop.maxSharedMemoryPerMultiProcessor};
        else
            (void)hipGetLastError();
    });
    return tab[dev];
}

// SPEC.md 1.1: one channel would take NumPy's pairwise window sums in the reference; these kernels sum element by element
static const char NEED_TWO_FILTERS[] =
    "the gammatone filterbank needs n_filters >= 2 (one channel: NumPy's pairwise window sums, SPEC.md 1.1)";

// What the filter loop asks of the windows, refused in this order by both gammatone entry points
static int check_windows(int n_samples, int nwin, int hop, int ncols)
{
    LSM_REQUIRE(nwin <= NWIN_MAX * hop, "nwin=%d needs more than %d overlapping windows of hop=%d",
                nwin, NWIN_MAX, hop);
    LSM_REQUIRE((long)(ncols - 1) * hop + nwin <= n_samples, "columns exceed the clip");
    LSM_REQUIRE(n_samples >= 8, "clips shorter than 8 samples are not supported");
    return LSM_OK;
}

// CU-exclusive placement for small launches: the dynamic LDS to request for a launch of `n_wgs` workgroups that use
// `used_bytes` each.  The reservation (half of a CU's LDS plus 1 KB) only caps the dispatcher at ONE gammatone
// workgroup per CU, so launches that overlap on other streams spread over the free CUs instead of stacking their waves
// on the SIMDs an earlier launch already occupies (measured at 256 clips x 128 filters, 3 streams: 0.85 -> 0.68 ms per
// launch, whole pipeline 1.18 -> 0.95 ms).  The other half of the LDS stays free for the reservoir workgroups (21.5 KB
// each at cfg2; two or three per CU is best).  Launches with more workgroups than CUs need several per CU and get no
// reservation, nor do those that use more than the reservation themselves.
static long cu_exclusive_lds(long n_wgs, long used_bytes)
{
    const DevInfo di = dev_info();
    const long resv = di.lds_per_cu / 2 + 1024;
    if (di.cus > 0 && n_wgs <= di.cus && di.lds_per_cu >= 4096 && resv > used_bytes && resv <= di.lds_per_cu)
        return resv;
    return used_bytes;
}

LSM_API int lsm_gammatone_spec_f64(const float *audio, int n_clips, int n_samples,
                                   const double *coefs, int n_filters, int nwin, int hop,
                                   int ncols, double *spec_out, double *db_out, int coef_flags,
                                   void *stream)
{
    LSM_REQUIRE(n_clips >= 0 && n_filters >= 1 && n_samples >= 1, "bad shape");
    LSM_REQUIRE(n_filters >= 2, "%s", NEED_TWO_FILTERS);
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(audio && coefs, "gammatone: null input");
    LSM_REQUIRE(spec_out || db_out, "gammatone: both outputs null");
    LSM_REQUIRE(nwin >= 1 && hop >= 1 && ncols >= 1, "bad window");
    if (const int rc = check_windows(n_samples, nwin, hop, ncols)) return rc;
    constexpr int wpb = 4;
    const long n_wgs = ((long)((n_filters + 63) / 64) * n_clips + wpb - 1) / wpb;
    const long lds = cu_exclusive_lds(n_wgs, 0);          // the kernel itself uses no LDS
    LSM_REQUIRE(n_wgs <= 0x7fffffffL, "too many clips for one launch");
    const dim3 grid((unsigned)n_wgs), block((unsigned)(64 * wpb));
    const bool fast = (coef_flags & 3) == 3;       // both properties verified by the host
    const int nw = (nwin + hop - 1) / hop;
    auto launch = [&](auto fn) {
        if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
        hipLaunchKernelGGL(fn, grid, block, (size_t)lds, (hipStream_t)stream, audio, n_clips, n_samples, coefs,
                           n_filters, nwin, hop, ncols, spec_out, db_out);
    };
    switch (nw) {
    case 1: launch(fast ? gammatone_kernel<1, true, true> : gammatone_kernel<1, false, false>); break;
    case 2: launch(fast ? gammatone_kernel<2, true, true> : gammatone_kernel<2, false, false>); break;
    case 3: launch(fast ? gammatone_kernel<3, true, true> : gammatone_kernel<3, false, false>); break;
    default: launch(fast ? gammatone_kernel<4, true, true> : gammatone_kernel<4, false, false>); break;
    }
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

// Layout of the fused launch for `n_filters` x `n_clips`: chains per lane, lane pair or not, waves per clip, waves per
// workgroup.
struct FusedPlan { int nch, groups, wpb; bool pair; };

// Hardware queues HIP gives this process: GPU_MAX_HW_QUEUES, or the runtime's default of 4 where it is unset (the package
// sets 12 before HIP starts unless the user chose a value).  Read at every plan, like the variable itself a per-process
// setting.
static int hw_queues()
{
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 4;
}

static bool fused_plan(int n_filters, int n_clips, int launch_flags, FusedPlan *p, bool step = false)
{
    // The lane pair for 2..256 filters, whatever the low-latency flag says, where queues are scarce: at 128 filters a clip
    // is 4 waves of 0.4 times the two-chain wave's time, so one 256-clip launch covers all 1024 SIMDs and the pipeline
    // needs no five launches in flight.  Its cost: 25 issue slots per 32 channel-samples (22 float64, 2 swaps, 1 move),
    // i.e. 100 per 128 against the two-chain layout's 70 (+43 %).  So
    //   * with more than 4 hardware queues the two-chain launches overlap enough to fill the chip and win (cfg2, 12 queues,
    //     medians of 5: profiles/r06_lane_pair_ab.txt); values between 5 and 11 are not measured;
    //   * a launch that the two-chain layout alone spreads over every SIMD (n_clips x groups >= 4 x CUs: cfg4's 1024
    //     clips) keeps the layouts below.
    const DevInfo di = dev_info();
    bool pair = n_filters <= 32 * GT_MAX_WPB && hw_queues() <= 4 &&
                (di.cus <= 0 || (long)n_clips * ((n_filters + 127) / 128) < 4L * di.cus);
    // (the fused step launch, step_fused.hip, is written for the lane pair and takes it wherever the pair's text can run)
    if (step) pair = n_filters <= 32 * GT_MAX_WPB;
    // otherwise two chains per lane above 64 filters (fewest CU-cycles per clip), unless the caller asks for the
    // low-latency layout: one chain per lane = twice the waves, each half as long (1.47 against 2.43 ms for 256 clips x
    // 128 filters on an idle GPU, for 12 % more CU time)
    int nch = (n_filters > 64 && !(launch_flags & 1)) ? 2 : 1;       // (bit 1 of the flags concerns the LDS reservation only)
    if (pair) nch = 1;
    // the low-latency flag is a layout hint, never a reason to refuse: 513..1024 filters need more than GT_MAX_WPB
    // one-chain waves per clip, so they keep the two-chain layout whatever the flag says
    if (nch == 1 && (n_filters + 63) / 64 > GT_MAX_WPB) nch = 2;
    const int cpw = pair ? 32 : 64;                              // channels per chain group
    const int groups = (n_filters + cpw * nch - 1) / (cpw * nch);
    if (groups > GT_MAX_WPB) return false;
    const int wpb = groups >= 4 ? groups : groups * (4 / groups);   // a multiple of `groups`, about 4 waves
    p->nch = nch; p->groups = groups; p->wpb = wpb; p->pair = pair;
    return true;
}

LSM_API int lsm_gammatone_spikes_layout(int n_clips, int n_filters, int launch_flags)
{
    FusedPlan pl;
    if (n_clips < 1 || n_filters < 1) return LSM_ERR_ARG;
    if (!fused_plan(n_filters, n_clips, launch_flags, &pl)) return LSM_ERR_UNSUPPORTED;
    return pl.pair ? 0 : pl.nch;
}

LSM_API long lsm_gammatone_spikes_workspace(int n_clips, int n_filters, int ncols)
{
    if (n_clips < 0 || n_filters < 1 || ncols < 1) return 0;
    // 64-channel groups padded to an even number: covers the one- and the two-chain layout and the lane pair (32-channel
    // groups)
    return (long)n_clips * ncols * (((n_filters + 127) / 128) * 2) * 64 * (long)sizeof(double);
}

// One launch of the fused front end: lsm_gammatone_spikes_f64, its masked and ragged twins and step_front_args fill the members
// by name (front_request, then their own), plan_front and gammatone_spikes read them; never one that is not the form's.
struct FrontRequest {
    FrontForm form = FrontForm::Plain;
    const float *audio = nullptr;
    const double *coefs = nullptr, *thr_on = nullptr, *thr_off = nullptr;
    int n_clips = 0, n_samples = 0, n_filters = 0, nwin = 0, hop = 0, ncols = 0, time_bins = 0, n_thr = 0, redundancy = 0;
    void *workspace = nullptr;
    long workspace_bytes = 0;
    int coef_flags = 0, launch_flags = 0;   // (a step's front half has no launch_flags, raster or stream: they stay 0)
    uint8_t *raster = nullptr;              // (n_clips, n_filters * redundancy, time_bins * n_thr)
    void *stream = nullptr;
    const uint32_t *freq_mask = nullptr, *time_mask = nullptr;     // Masked (SPEC.md 1.13), and Ragged with masks (1.16)
    const int32_t *clip_bins = nullptr;     // Ragged (1.14): DEVICE counts in and out; ncols, time_bins and n_samples the strides
    int32_t *clip_steps_out = nullptr;
    lsm_fe::StepFront *step = nullptr;      // Step (step_fused.hip): checked and planned into it, not launched
};

// what all six callers are given
static FrontRequest front_request(const float *audio, int n_clips, int n_samples, const double *coefs, int n_filters, int nwin,
                                  int hop, int ncols, int time_bins, const double *thr_on, const double *thr_off, int n_thr,
                                  int redundancy, void *workspace, long workspace_bytes, int coef_flags)
{
    FrontRequest r;
    r.audio = audio; r.n_clips = n_clips; r.n_samples = n_samples; r.coefs = coefs; r.n_filters = n_filters; r.nwin = nwin;
    r.hop = hop; r.ncols = ncols; r.time_bins = time_bins; r.thr_on = thr_on; r.thr_off = thr_off; r.n_thr = n_thr;
    r.redundancy = redundancy; r.workspace = workspace; r.workspace_bytes = workspace_bytes; r.coef_flags = coef_flags;
    return r;
}

// What a launch refuses, in the order that decides which reason a caller with two bad arguments reads (the form's own last),
// the plan, the kernel's arguments and the launch geometry.  An empty batch is accepted before its buffers are: l->grid = 0.
static int plan_front(const FrontRequest &r, FusedArgs *args, lsm_fe::FusedLaunch *l)
{
    const bool step = r.form == FrontForm::Step;
    l->grid = 0;
    LSM_REQUIRE((r.launch_flags & ~3) == 0, "launch_flags: only bit 0 (low-latency layout) and bit 1 (no LDS reservation) are defined");
    LSM_REQUIRE(r.n_clips >= 0 && r.n_filters >= 1 && r.n_samples >= 1, "bad shape");
    LSM_REQUIRE(r.n_filters >= 2, "%s", NEED_TWO_FILTERS);
    LSM_REQUIRE(r.nwin >= 1 && r.hop >= 1 && r.ncols >= 2 && r.time_bins >= 2, "bad window");
    if (const int rc = check_windows(r.n_samples, r.nwin, r.hop, r.ncols)) return rc;
    LSM_REQUIRE(r.n_thr >= 1 && r.n_thr <= MAX_THR, "n_thr=%d outside [1, %d]", r.n_thr, MAX_THR);
    LSM_REQUIRE(r.redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(r.thr_on && r.thr_off, "null threshold table");
    if (r.n_clips == 0) return LSM_OK;
    LSM_REQUIRE(r.audio && r.coefs && (r.raster || step) && r.workspace, "gammatone_spikes: null buffer");
    LSM_REQUIRE(r.workspace_bytes >= lsm_gammatone_spikes_workspace(r.n_clips, r.n_filters, r.ncols),
                "workspace of %ld bytes, need %ld (lsm_gammatone_spikes_workspace)", r.workspace_bytes,
                lsm_gammatone_spikes_workspace(r.n_clips, r.n_filters, r.ncols));
    LSM_REQUIRE(((uintptr_t)r.workspace & 7u) == 0, "workspace must be 8-byte aligned");
    const int row_bytes = r.time_bins * r.n_thr;
    LSM_REQUIRE((row_bytes & 3) != 0 || ((uintptr_t)r.raster & 3u) == 0,
                "the raster must be 4-byte aligned when a row is a multiple of 4 bytes");
    FusedPlan pl;
    if (!fused_plan(r.n_filters, r.n_clips, r.launch_flags, &pl, step)) {
        lsm_set_error("gammatone_spikes: %d filters need more than %d waves per clip; use the split entry points",
                      r.n_filters, GT_MAX_WPB);
        return LSM_ERR_UNSUPPORTED;
    }
    FusedArgs &a = *args;
    a.audio = r.audio; a.coefs = r.coefs; a.ws = static_cast<double *>(r.workspace); a.raster = r.raster;
    a.n_clips = r.n_clips; a.n_samples = r.n_samples; a.n_filters = r.n_filters; a.nwin = r.nwin; a.hop = r.hop;
    a.ncols = r.ncols; a.time_bins = r.time_bins; a.n_thr = r.n_thr; a.redundancy = r.redundancy; a.groups = pl.groups;
    a.prio = 0;
    // unused table entries never fire: nothing is > +inf or < -inf (the kernel compares 4 or 8 thresholds)
    fill_thresholds<double>(a.on, a.off, r.thr_on, r.thr_off, r.n_thr);
    const long n_waves = (long)pl.groups * r.n_clips;
    const long n_wgs = (n_waves + pl.wpb - 1) / pl.wpb;
    LSM_REQUIRE(n_wgs <= 0x7fffffffL, "too many clips for one launch");
    // per lane row: the raster bits of the channel (time_bins * n_thr bits), staged for the coalesced write-out
    const int RW = (r.time_bins * r.n_thr + 31) / 32;
    long lds = 2 * GT_MAX_WPB * (long)sizeof(double) + (long)pl.wpb * pl.nch * (pl.pair ? 32 : 64) * RW * 4;
    LSM_REQUIRE(lds <= 160 * 1024, "raster stage of %ld bytes exceeds one CU's LDS", lds);
    // CU-exclusive placement of small launches (cu_exclusive_lds), with two exceptions.
    // launch_flags bit 1: the caller runs LDS-hungry workgroups of another kernel beside this launch (the ring-row
    // reservoir kernel: 64-74 KB per clip, two per CU) -- no reservation then: the launch asks for what it uses
    // (27 KB per 4-wave workgroup at 4 thresholds x 100 bins) and fits beside such a pair
    // The lane pair takes none: its launch already has a wave on every SIMD, and the reservation would only keep the
    // next step's launch off the CUs until this one has left (cfg2, 4 hardware queues, medians of 3 runs: 1.10 -> 1.00
    // ms/step at 20 steps, 1.11 -> 0.98 at 200; 12 queues, one run each: 1.03 -> 1.00 and 0.98 -> 0.86;
    // profiles/r06_lane_pair_placement.txt)
    if (!pl.pair && !(r.launch_flags & 2)) lds = cu_exclusive_lds(n_wgs, lds);
    const bool fast = (r.coef_flags & 3) == 3;
    const bool shb0 = fast && (r.coef_flags & 4) != 0;     // one b0 for every channel: shared between the two chains,
                                                           // wave-uniform in the lane pair
    const int nw = (r.nwin + r.hop - 1) / r.hop;
    *l = lsm_fe::FusedLaunch{nw > 4 ? 4 : nw, pl.nch, fast, shb0, pl.pair, (unsigned)n_wgs, (unsigned)(64 * pl.wpb), (size_t)lds};
    // the forms' own refusals, behind the twin's
    if (const int rc = r.form == FrontForm::Masked ? check_masks(r.freq_mask, r.time_mask) : LSM_OK) return rc;
    if (r.form == FrontForm::Ragged) {
        if (const int rc = check_ragged(r.clip_bins, r.clip_bins, r.time_bins, r.n_samples, r.hop)) return rc;
        LSM_REQUIRE(((uintptr_t)r.clip_steps_out & 3u) == 0, "ragged: clip_steps_out must be 4-byte aligned");
        if (const int rc = check_masks(r.freq_mask, r.time_mask)) return rc;    // (the ragged export leaves both null)
    }
    return LSM_OK;
}

// this unit's kernel for the form table (gammatone_spikes_body.h, launch_fused_form)
struct PlainFamily {
    template <int NW, bool FAST, int NCH, bool SHB0, bool PAIR>
    static auto kernel() { return gammatone_spikes_kernel<NW, FAST, NCH, SHB0, PAIR>; }
};

// Every caller ends here with the request it filled: checked and planned, then the form's launch, or a step's plan handed over.
static int gammatone_spikes(const FrontRequest &r)
{
    FusedArgs a;
    lsm_fe::FusedLaunch l;
    const int rc = plan_front(r, &a, &l);
    if (rc != LSM_OK || l.grid == 0) return rc;         // refused, or an empty batch
    if (r.form == FrontForm::Step) {
        r.step->l = l;
        static_assert(sizeof(r.step->args) == sizeof(FusedArgs), "StepFront carries a FusedArgs");
        memcpy(r.step->args, &a, sizeof(FusedArgs));
        return LSM_OK;
    }
    if (r.form == FrontForm::Masked && (r.freq_mask || r.time_mask))       // without a mask exactly the plain launch
        lsm_fe::launch_gammatone_spikes_masked(l, &a, lsm_fe::MaskArgs{r.freq_mask, r.time_mask}, r.stream);
    else if (r.form == FrontForm::Ragged && (r.freq_mask || r.time_mask))
        lsm_fe::launch_gammatone_spikes_ragged_masked(l, &a, lsm_fe::RaggedArgs{r.clip_bins, r.clip_steps_out},
                                                      lsm_fe::MaskArgs{r.freq_mask, r.time_mask}, r.stream);
    else if (r.form == FrontForm::Ragged)                                  // without a mask exactly the ragged launch
        lsm_fe::launch_gammatone_spikes_ragged(l, &a, lsm_fe::RaggedArgs{r.clip_bins, r.clip_steps_out}, r.stream);
    else
        launch_fused_form<PlainFamily>(l, r.stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_gammatone_spikes_f64(const float *audio, int n_clips, int n_samples,
                                     const double *coefs, int n_filters, int nwin, int hop, int ncols,
                                     int time_bins, const double *thr_on, const double *thr_off, int n_thr,
                                     int redundancy, uint8_t *raster, void *workspace, long workspace_bytes,
                                     int coef_flags, int launch_flags, void *stream)
{
    FrontRequest r = front_request(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                                   n_thr, redundancy, workspace, workspace_bytes, coef_flags);
    r.raster = raster; r.launch_flags = launch_flags; r.stream = stream;
    return gammatone_spikes(r);
}

// step_fused.hip: lsm_gammatone_spikes_f64's refusals, plan and arguments for the front-end half of a fused step (no raster)
int lsm_fe::step_front_args(const float *audio, int n_clips, int n_samples, const double *coefs, int n_filters, int nwin,
                            int hop, int ncols, int time_bins, const double *thr_on, const double *thr_off, int n_thr,
                            int redundancy, void *workspace, long workspace_bytes, int coef_flags, StepFront *out)
{
    FrontRequest r = front_request(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                                   n_thr, redundancy, workspace, workspace_bytes, coef_flags);
    r.form = FrontForm::Step; r.step = out;
    return gammatone_spikes(r);
}

// step_fused.hip: the masked and the ragged step's own refusals are the masked and the ragged front end's, made there behind
// the reservoir's (a ragged step has one count array and no clip_steps_out)
int lsm_fe::step_check_masks(const uint32_t *freq_mask, const uint32_t *time_mask)
{
    return check_masks(freq_mask, time_mask);
}

int lsm_fe::step_check_ragged(const int32_t *clip_bins, int time_bins, long n_samples, long hop)
{
    return check_ragged(clip_bins, clip_bins, time_bins, n_samples, hop);
}

LSM_API int lsm_gammatone_spikes_masked_f64(const float *audio, int n_clips, int n_samples,
                                            const double *coefs, int n_filters, int nwin, int hop, int ncols,
                                            int time_bins, const double *thr_on, const double *thr_off, int n_thr,
                                            int redundancy, uint8_t *raster, void *workspace, long workspace_bytes,
                                            int coef_flags, int launch_flags, const uint32_t *freq_mask,
                                            const uint32_t *time_mask, void *stream)
{
    FrontRequest r = front_request(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                                   n_thr, redundancy, workspace, workspace_bytes, coef_flags);
    r.raster = raster; r.launch_flags = launch_flags; r.stream = stream;
    r.form = FrontForm::Masked; r.freq_mask = freq_mask; r.time_mask = time_mask;
    return gammatone_spikes(r);
}

// include/lsm_hip_ragged.h (SPEC.md 1.14): the twins' parameters with per-clip DEVICE counts; kernels in ragged_frontend.hip
LSM_API int lsm_gammatone_spikes_ragged_f64(const float *audio, int n_clips, int n_samples,
                                            const double *coefs, int n_filters, int nwin, int hop, int ncols,
                                            int time_bins, const int32_t *clip_bins, const double *thr_on,
                                            const double *thr_off, int n_thr, int redundancy, uint8_t *raster,
                                            int32_t *clip_steps_out, void *workspace, long workspace_bytes,
                                            int coef_flags, int launch_flags, void *stream)
{
    FrontRequest r = front_request(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                                   n_thr, redundancy, workspace, workspace_bytes, coef_flags);
    r.raster = raster; r.launch_flags = launch_flags; r.stream = stream;
    r.form = FrontForm::Ragged; r.clip_bins = clip_bins; r.clip_steps_out = clip_steps_out;
    return gammatone_spikes(r);
}

// include/lsm_hip_ragged_augment.h (SPEC.md 1.16): the ragged twins' parameters with freq_mask, time_mask before the stream;
// kernels in ragged_masked_frontend.hip
LSM_API int lsm_gammatone_spikes_ragged_masked_f64(const float *audio, int n_clips, int n_samples,
                                                   const double *coefs, int n_filters, int nwin, int hop, int ncols,
                                                   int time_bins, const int32_t *clip_bins, const double *thr_on,
                                                   const double *thr_off, int n_thr, int redundancy, uint8_t *raster,
                                                   int32_t *clip_steps_out, void *workspace, long workspace_bytes,
                                                   int coef_flags, int launch_flags, const uint32_t *freq_mask,
                                                   const uint32_t *time_mask, void *stream)
{
    FrontRequest r = front_request(audio, n_clips, n_samples, coefs, n_filters, nwin, hop, ncols, time_bins, thr_on, thr_off,
                                   n_thr, redundancy, workspace, workspace_bytes, coef_flags);
    r.raster = raster; r.launch_flags = launch_flags; r.stream = stream;
    r.form = FrontForm::Ragged; r.clip_bins = clip_bins; r.clip_steps_out = clip_steps_out;
    r.freq_mask = freq_mask; r.time_mask = time_mask;
    return gammatone_spikes(r);
}

LSM_API int lsm_spec_to_spikes_ragged_masked_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins,
                                                 const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                                 const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                                                 uint8_t *raster, double *norm_out, const uint32_t *freq_mask,
                                                 const uint32_t *time_mask, void *stream)
{
    SplitRequest<double> r = split_request<double>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                   redundancy, raster, norm_out, stream);
    r.form = FrontForm::Ragged; r.clip_cols = clip_cols; r.clip_bins = clip_bins;
    r.freq_mask = freq_mask; r.time_mask = time_mask;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_ragged_masked_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins,
                                                 const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                                 const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                                                 uint8_t *raster, float *norm_out, const uint32_t *freq_mask,
                                                 const uint32_t *time_mask, void *stream)
{
    SplitRequest<float> r = split_request<float>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                 redundancy, raster, norm_out, stream);
    r.form = FrontForm::Ragged; r.clip_cols = clip_cols; r.clip_bins = clip_bins;
    r.freq_mask = freq_mask; r.time_mask = time_mask;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_ragged_f64(const double *db, int n_clips, int n_filters, int ncols, int time_bins,
                                          const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                          const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                                          uint8_t *raster, double *norm_out, void *stream)
{
    SplitRequest<double> r = split_request<double>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                   redundancy, raster, norm_out, stream);
    r.form = FrontForm::Ragged; r.clip_cols = clip_cols; r.clip_bins = clip_bins;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_ragged_f32(const float *db, int n_clips, int n_filters, int ncols, int time_bins,
                                          const int32_t *clip_cols, const int32_t *clip_bins, int apply_floor,
                                          const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                                          uint8_t *raster, float *norm_out, void *stream)
{
    SplitRequest<float> r = split_request<float>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                 redundancy, raster, norm_out, stream);
    r.form = FrontForm::Ragged; r.clip_cols = clip_cols; r.clip_bins = clip_bins;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_masked_f64(const double *db, int n_clips, int n_filters, int ncols,
                                          int time_bins, int apply_floor, const double *thr_on,
                                          const double *thr_off, int n_thr, int redundancy,
                                          uint8_t *raster, double *norm_out, const uint32_t *freq_mask,
                                          const uint32_t *time_mask, void *stream)
{
    SplitRequest<double> r = split_request<double>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                   redundancy, raster, norm_out, stream);
    r.form = FrontForm::Masked; r.freq_mask = freq_mask; r.time_mask = time_mask;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_masked_f32(const float *db, int n_clips, int n_filters, int ncols,
                                          int time_bins, int apply_floor, const float *thr_on,
                                          const float *thr_off, int n_thr, int redundancy,
                                          uint8_t *raster, float *norm_out, const uint32_t *freq_mask,
                                          const uint32_t *time_mask, void *stream)
{
    SplitRequest<float> r = split_request<float>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off, n_thr,
                                                 redundancy, raster, norm_out, stream);
    r.form = FrontForm::Masked; r.freq_mask = freq_mask; r.time_mask = time_mask;
    return launch_spec_to_spikes(r);
}

LSM_API int lsm_spec_to_spikes_f64(const double *db, int n_clips, int n_filters, int ncols,
                                   int time_bins, int apply_floor, const double *thr_on,
                                   const double *thr_off, int n_thr, int redundancy,
                                   uint8_t *raster, double *norm_out, void *stream)
{
    return launch_spec_to_spikes(split_request<double>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off,
                                                       n_thr, redundancy, raster, norm_out, stream));
}

LSM_API int lsm_spec_to_spikes_f32(const float *db, int n_clips, int n_filters, int ncols,
                                   int time_bins, int apply_floor, const float *thr_on,
                                   const float *thr_off, int n_thr, int redundancy,
                                   uint8_t *raster, float *norm_out, void *stream)
{
    return launch_spec_to_spikes(split_request<float>(db, n_clips, n_filters, ncols, time_bins, apply_floor, thr_on, thr_off,
                                                      n_thr, redundancy, raster, norm_out, stream));
}

LSM_API int lsm_encode_hysteresis_f64(const double *spec, int n_rows, int n_bins,
                                      const double *thr_on, const double *thr_off, int n_thr,
                                      uint8_t *out, void *stream)
{
    return launch_encode<double>(spec, n_rows, n_bins, thr_on, thr_off, n_thr, out, stream);
}

LSM_API int lsm_encode_hysteresis_f32(const float *spec, int n_rows, int n_bins,
                                      const float *thr_on, const float *thr_off, int n_thr,
                                      uint8_t *out, void *stream)
{
    return launch_encode<float>(spec, n_rows, n_bins, thr_on, thr_off, n_thr, out, stream);
}

// Launch of pack_bits_kernel or unpack_bits_kernel (same parameters): `src` -> `dst`, one of which is `raster`.
static int launch_bits(void (*kernel)(const uint8_t *, long, int, int, uint8_t *), const uint8_t *src, uint8_t *dst,
                       const uint8_t *raster, long n_rows, int T, const char *what, void *stream)
{
    LSM_REQUIRE(n_rows >= 0 && T >= 1, "%s: bad shape", what);
    if (n_rows == 0) return LSM_OK;                     // nothing to do
    LSM_REQUIRE(src && dst, "%s: null buffer", what);
    // rows of a multiple of 8 steps move as 64-bit words; other lengths go byte by byte
    LSM_REQUIRE((T & 7) != 0 || ((uintptr_t)raster & 7u) == 0,
                "%s: the raster must be 8-byte aligned when n_steps is a multiple of 8", what);
    const int TP = (T + 7) / 8;
    LSM_REQUIRE(n_rows * (long)TP <= 0x7fffffffL * 256L, "%s: too many rows", what);
    const long n = n_rows * TP;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, n_rows, T, TP,
                       dst);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_raster_pack_bits(const uint8_t *raster, long n_rows, int n_steps, uint8_t *packed,
                                 void *stream)
{
    return launch_bits(pack_bits_kernel, raster, packed, raster, n_rows, n_steps, "pack_bits", stream);
}

LSM_API int lsm_raster_unpack_bits(const uint8_t *packed, long n_rows, int n_steps, uint8_t *raster,
                                   void *stream)
{
    return launch_bits(unpack_bits_kernel, packed, raster, raster, n_rows, n_steps, "unpack_bits", stream);
}
