// Streamed gammatone front end for gfx950 (SPEC.md §1.6, include/lsm_hip_audio.h): gammatone filterbank -> dB ->
// fixed-range normalise -> hysteresis spike encoder, continued from a saved per-stream state.  A stream cut into launches at
// any hop boundaries gives, bit for bit, the raster of its one uncut run: the filter state, the window sums open across the
// boundary and the latches travel in the state block, the normalisation range is fixed for the stream's life, and there is
// one time bin per column (no resize).  Every float operation of the filter and the window sums is the one of
// gammatone_kernel (frontend.hip) in its order (gammatone_body.h); compiled with -ffp-contract=off.
// state_in, state_out and stream_hops follow DESIGN.md "The state block" (stream_state.h).
#include "lsm_common.h"
#include "gammatone_body.h"
#include "spikes_body.h"
#include "stream_state.h"
#include <cmath>
#include <type_traits>

namespace {

using lsm_fe::MAX_THR;
using namespace lsm_state;
constexpr int NWIN_MAX = 4;             // windows live at any sample, at most (nwin <= NWIN_MAX * hop)
constexpr int GTS_WPB = 4;              // waves per workgroup: one per SIMD of its CU

// One stream's state block, arrays over the n_filters channels one after the other:
//   (8 + NW - 1) x float64   z0, z1 of sections 1..4, then the NW - 1 open window sums, youngest first
//   uint32                   latch bits (bit k: threshold k)
//   uint32                   hops seen, saturating at NW - 1
// rounded up to a multiple of 16 bytes.  All zeros: the start of a stream.
__host__ __device__ inline size_t state_doubles(int nw) { return (size_t)(8 + nw - 1); }
__host__ __device__ inline size_t state_used_bytes(int n_filters, int nw)
{
    return (state_doubles(nw) * 8 + 8) * (size_t)n_filters;
}
__host__ __device__ inline size_t state_block_bytes(int n_filters, int nw)
{
    return state_round16(state_used_bytes(n_filters, nw));
}

struct StreamArgs {
    const int32_t *stream_hops;         // (n_streams) or null
    const unsigned char *state_in;      // or null
    unsigned char *state_out;           // or null; may be state_in
    uint8_t *raster;                    // (n_streams, F * R, H * n_thr)
    double *spec_out, *db_out;          // (n_streams, F, H) or null
    int n_streams, n_hops, n_filters, nwin, hop, n_thr, redundancy;
    double db_lo, db_hi;
    double on[MAX_THR], off[MAX_THR];   // entries from n_thr on never fire (+inf / -inf)
};

// One lane = one channel, one wave = 64 channels of ONE stream, so the audio sample is wave-uniform and arrives through
// scalar loads (8 samples per fetch, the next chunk requested before the current one is consumed), as in gammatone_kernel.
// NW = ceil(nwin / hop) windows are live at any sample; in every hop exactly one of them closes, after sample
// pos = nwin - (NW - 1) * hop of the hop.  Whether it is a column is a matter of the hops the stream has seen: the first
// NW - 1 hops of a stream close windows that would have begun before its first sample.  Nothing else depends on where the
// stream is on its timeline.
template <int NW, bool FAST>
__global__ __launch_bounds__(GTS_WPB * 64) void gammatone_stream_kernel(const float *__restrict__ audio,
                                                                         const double *__restrict__ coefs,
                                                                         const StreamArgs a)
{
    const int F = a.n_filters, hop = a.hop, nwin = a.nwin, H = a.n_hops;
    const int groups = (F + 63) >> 6;
    const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    const int b = wid / groups;
    if (b >= a.n_streams) return;                       // wave-uniform; the kernel has no barrier
    const int chl = (wid - b * groups) * 64 + (int)(threadIdx.x & 63);
    const bool live = chl < F;
    const int ch = live ? chl : F - 1;
    const int hb = __builtin_amdgcn_readfirstlane(stream_count(a.stream_hops, b, H));     // wave-uniform

    constexpr int ND = 8 + NW - 1;                      // doubles per channel in the state block
    const size_t block = state_block_bytes(F, NW), used = state_used_bytes(F, NW);
    const StateBlock blk = state_block(a.state_in, a.state_out, b, block);
    const unsigned char *sin = blk.sin;
    unsigned char *sout = blk.sout;
    // out of place: the padding (the stream's first wave) and an idle stream's block (every lane its channel, below) travel
    if (wid == b * groups) carry_padding<unsigned char>(blk, used, block, (int)(threadIdx.x & 63));

    double st[ND];
    uint32_t act = 0u, cnt = 0u;
#pragma unroll
    for (int k = 0; k < ND; ++k) st[k] = 0.0;
    if (sin) {
        const double *sd = reinterpret_cast<const double *>(sin);
#pragma unroll
        for (int k = 0; k < ND; ++k) st[k] = sd[(size_t)k * F + ch];
        const uint32_t *su = reinterpret_cast<const uint32_t *>(sin + (size_t)ND * 8 * F);
        act = su[ch];
        cnt = __builtin_amdgcn_readfirstlane(su[F + ch]);       // every channel of a stream has seen the same hops
    }
    if (hb == 0) {
        if (blk.copy && live) {
            double *dd = reinterpret_cast<double *>(sout);
#pragma unroll
            for (int k = 0; k < ND; ++k) dd[(size_t)k * F + ch] = st[k];
            uint32_t *du = reinterpret_cast<uint32_t *>(sout + (size_t)ND * 8 * F);
            du[ch] = act;
            du[F + ch] = cnt;
        }
        return;
    }

    const lsm_gt::Sections s = lsm_gt::load_sections(coefs, ch);
    const double b0 = s.b0, b2 = s.b2, b11 = s.b1[0], b12 = s.b1[1], b13 = s.b1[2], b14 = s.b1[3];
    const double a1 = s.a1, a2 = s.a2, gain = s.gain, rgain = s.rgain;
    const int n_row = H * hop;                          // samples of a row of `audio`
    const float *__restrict__ x = audio + (size_t)b * n_row;          // wave-uniform

    double z01 = st[0], z11 = st[1], z02 = st[2], z12 = st[3], z03 = st[4], z13 = st[5], z04 = st[6], z14 = st[7];
    double win[NW];
    win[0] = 0.0;
#pragma unroll
    for (int q = 1; q < NW; ++q) win[q] = st[7 + q];

    auto filt = [&](float xf) -> double {
        const double x0 = (double)xf;
        const double y1 = lsm_gt::section<FAST>(z01, b0, x0, z11, b11, a1, a2, b2);
        const double y2 = lsm_gt::section<FAST>(z02, b0, y1, z12, b12, a1, a2, b2);
        const double y3 = lsm_gt::section<FAST>(z03, b0, y2, z13, b13, a1, a2, b2);
        const double y4 = lsm_gt::section<FAST>(z04, b0, y3, z14, b14, a1, a2, b2);
        double o;
        lsm_gt::quot<FAST>(o, y4, gain, rgain);
        return o * o;
    };
    // samples [n, n_to) with the NACT youngest windows accumulating; the prefetch is clamped inside the row (the extra
    // chunk at the end of a run is loaded but never used; a run of 8 samples or more implies a row of 8 or more)
#define LSM_RUNS(n_to, NACT)                                                        \
    {                                                                               \
        if (n + 8 <= (n_to)) {                                                      \
            float xs[8], nx[8];                                                     \
            _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = x[n + u];         \
            for (; n + 8 <= (n_to); n += 8) {                                       \
                const float *pn = x + min(n + 8, n_row - 8);                        \
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

    const int pos = nwin - (NW - 1) * hop;              // in (0, hop]
    const double dn = (double)nwin;
    const double fl = a.db_hi - 80.0, lo = a.db_lo;
    const double den = (a.db_hi - a.db_lo) + 1e-8;
    const int n_thr = a.n_thr, R = a.redundancy;
    const uint32_t tmask = (1u << n_thr) - 1u;
    const size_t row_bytes = (size_t)H * n_thr;
    uint8_t *rrow = a.raster + ((size_t)b * F + ch) * R * row_bytes;  // this channel's first raster row
    const size_t obase = ((size_t)b * F + ch) * H;
    int col = 0;                                        // columns this launch has emitted (wave-uniform)
    int n = 0;
    for (int h = 0; h < hb; ++h) {
        const int base = h * hop;
        LSM_RUNS(base + pos, NW)
        if (cnt >= (uint32_t)(NW - 1)) {                // wave-uniform
            const double y = sqrt(win[NW - 1] / dn);
            const double v = 20 * log10(y + 1e-9);
            // a NaN stays a NaN through the floor and compares false with every threshold: the latches keep their state
            const double val = lsm_fe::floored_value(v, fl, lo, den);
            uint32_t S = 0u, Rr = 0u;
#pragma unroll
            for (int t = 0; t < MAX_THR; ++t) {
                S |= (val > a.on[t] ? 1u : 0u) << t;
                Rr |= (val < a.off[t] ? 1u : 0u) << t;
            }
            act = lsm_fe::latch_step(act, S, Rr, tmask);
            if (live) {
                if (a.spec_out) a.spec_out[obase + col] = y;
                if (a.db_out) a.db_out[obase + col] = v;
                lsm_fe::store_column(rrow, row_bytes, col, n_thr, R, act);
            }
            ++col;
        } else {
            ++cnt;
        }
        LSM_RUNS(base + hop, NW - 1)
#pragma unroll
        for (int q = NW - 1; q > 0; --q) win[q] = win[q - 1];
        win[0] = 0.0;
    }
#undef LSM_RUNS

    if (sout && live) {
        double *dd = reinterpret_cast<double *>(sout);
        dd[(size_t)0 * F + ch] = z01; dd[(size_t)1 * F + ch] = z11; dd[(size_t)2 * F + ch] = z02; dd[(size_t)3 * F + ch] = z12;
        dd[(size_t)4 * F + ch] = z03; dd[(size_t)5 * F + ch] = z13; dd[(size_t)6 * F + ch] = z04; dd[(size_t)7 * F + ch] = z14;
#pragma unroll
        for (int q = 1; q < NW; ++q) dd[(size_t)(7 + q) * F + ch] = win[q];
        uint32_t *du = reinterpret_cast<uint32_t *>(sout + (size_t)ND * 8 * F);
        du[ch] = act;
        du[F + ch] = cnt;
    }
}

template <int N> using Int = std::integral_constant<int, N>;

bool windows_ok(int nwin, int hop) { return hop >= 1 && nwin >= hop && (long)nwin <= (long)NWIN_MAX * hop; }

}  // namespace

LSM_API long lsm_gammatone_stream_state_bytes(int n_filters, int nwin, int hop)
{
    if (n_filters < 2 || !windows_ok(nwin, hop)) return 0;
    return (long)state_block_bytes(n_filters, (nwin + hop - 1) / hop);
}

LSM_API int lsm_gammatone_stream_f64(const float *audio, int n_streams, int n_hops, const double *coefs, int n_filters,
                                     int nwin, int hop, const int32_t *stream_hops, double db_lo, double db_hi,
                                     const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                                     const void *state_in, void *state_out, uint8_t *raster_out, double *spec_out,
                                     double *db_out, int coef_flags, void *stream)
{
    LSM_REQUIRE(n_filters >= 2,
                "the gammatone filterbank needs n_filters >= 2 (one channel: NumPy's pairwise window sums, SPEC.md 1.1)");
    LSM_REQUIRE(n_streams >= 0, "n_streams=%d must be >= 0", n_streams);
    LSM_REQUIRE(hop >= 1, "hop=%d must be >= 1", hop);
    LSM_REQUIRE((long)nwin <= (long)NWIN_MAX * hop, "nwin=%d needs more than %d overlapping windows of hop=%d", nwin,
                NWIN_MAX, hop);
    LSM_REQUIRE(nwin >= hop, "nwin=%d is shorter than hop=%d: samples between two windows would feed no column", nwin, hop);
    LSM_REQUIRE(n_hops >= 1, "n_hops=%d: a launch's row stride H must be >= 1", n_hops);
    LSM_REQUIRE((long)n_hops * hop <= 0x7fffffffL, "n_hops * hop exceeds 2^31 - 1 samples per row");
    LSM_REQUIRE(std::isfinite(db_lo) && std::isfinite(db_hi), "db_lo and db_hi (the calibration range) must be finite");
    LSM_REQUIRE(db_lo < db_hi, "the calibration range needs db_lo < db_hi, got [%g, %g]", db_lo, db_hi);
    LSM_REQUIRE(n_thr >= 1 && n_thr <= MAX_THR, "n_thr=%d outside [1, %d]", n_thr, MAX_THR);
    LSM_REQUIRE(redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(thr_on && thr_off, "null threshold table");
    LSM_REQUIRE(raster_out != nullptr, "raster_out is required");
    LSM_REQUIRE_ALIGNED(raster_out, 4);
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE_ALIGNED(coefs, 8);
    LSM_REQUIRE_ALIGNED(stream_hops, 4);
    LSM_REQUIRE_ALIGNED(state_in, 16);
    LSM_REQUIRE_ALIGNED(state_out, 16);
    LSM_REQUIRE_ALIGNED(spec_out, 8);
    LSM_REQUIRE_ALIGNED(db_out, 8);
    if (n_streams == 0) return LSM_OK;
    LSM_REQUIRE(audio && coefs, "gammatone_stream: null input");
    StreamArgs a;
    a.stream_hops = stream_hops;
    a.state_in = static_cast<const unsigned char *>(state_in);
    a.state_out = static_cast<unsigned char *>(state_out);
    a.raster = raster_out; a.spec_out = spec_out; a.db_out = db_out;
    a.n_streams = n_streams; a.n_hops = n_hops; a.n_filters = n_filters; a.nwin = nwin; a.hop = hop;
    a.n_thr = n_thr; a.redundancy = redundancy; a.db_lo = db_lo; a.db_hi = db_hi;
    lsm_fe::fill_thresholds<double>(a.on, a.off, thr_on, thr_off, n_thr);
    const long n_wgs = ((long)((n_filters + 63) / 64) * n_streams + GTS_WPB - 1) / GTS_WPB;
    LSM_REQUIRE(n_wgs <= 0x7fffffffL, "too many streams for one launch");
    const dim3 grid((unsigned)n_wgs), block((unsigned)(64 * GTS_WPB));
    const bool fast = (coef_flags & 3) == 3;            // both properties verified by the host (frontend.coef_flags)
    auto launch_nw = [&](auto nw_c) {
        constexpr int NW = decltype(nw_c)::value;
        if (fast) hipLaunchKernelGGL((gammatone_stream_kernel<NW, true>), grid, block, 0, (hipStream_t)stream, audio, coefs, a);
        else hipLaunchKernelGGL((gammatone_stream_kernel<NW, false>), grid, block, 0, (hipStream_t)stream, audio, coefs, a);
    };
    switch ((nwin + hop - 1) / hop) {
    case 1: launch_nw(Int<1>{}); break;
    case 2: launch_nw(Int<2>{}); break;
    case 3: launch_nw(Int<3>{}); break;
    default: launch_nw(Int<4>{}); break;
    }
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
