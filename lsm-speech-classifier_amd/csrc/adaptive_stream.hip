// Adaptive-range spike encoder for gfx950 (SPEC.md §1.9, include/lsm_hip_adaptive.h): the dB columns a streamed front end
// completed -> normalised with the minimum and maximum of the stream's last L columns (the causal form of the reference's
// per-clip range, create_dataset.py:59-67) -> hysteresis latches -> raster.  Minimum and maximum do not depend on the order
// they are taken in, so a stream cut into launches anywhere gives the raster and the state of its uncut run byte for byte.
// Every operation is in the dB array's type T in the order SPEC.md §1.9 writes; compiled with -ffp-contract=off.
//
// One workgroup of ADP_WAVES waves per stream walks its new columns in chunks of 64, a lane a column:
//   1. column extrema: a wave takes every ADP_WAVES-th filter row, so consecutive lanes read consecutive columns of a row;
//      the waves' partial extrema meet in LDS and land behind the carried ones (`ext`: at most L - 1 carried + 64 new);
//   2. window extrema: the at most L entries ending at a lane's column, again split over the waves and joined in LDS;
//   3. a wave takes a filter row (the loads of eight rows issued together): normalised value, one ballot per threshold and
//      comparison, and the latch over the chunk's
//      64 columns as the carry chain of an addition started from the carried latch bit (spikes_body.h's step 2; all of it
//      wave-uniform); lane c holds column c's bits and stores them, a word per column where n_thr = 4;
//   4. the last min(L - 1, columns so far) extrema move to the front of `ext` for the next chunk, and at the end into the state.
// LDS: 2 * (L - 1 + 64) + 2 * ADP_WAVES * 64 values of T and a latch word per filter -- nothing that grows with H.
// state_in, state_out and stream_cols follow DESIGN.md "The state block" (stream_state.h).
#include "spikes_body.h"
#include "stream_state.h"
#include <math.h>

namespace {

using lsm_fe::MAX_THR;
using namespace lsm_state;
constexpr int ADP_WAVES = 4;                // waves per workgroup: one per SIMD of its CU
constexpr int ADP_THREADS = ADP_WAVES * 64;
constexpr int ADP_CHUNK = 64;               // columns per chunk: a lane each
constexpr int ADP_ROWS = 8;                 // filter rows a wave loads together in step 3
constexpr int ADP_MAX_WINDOW = 4096;
constexpr int ADP_MAX_FILTERS = 16384;      // a latch word each in LDS: 64 KB

// One stream's state block:
//   (L - 1) x T   cmin of the carried columns, oldest first; slots not in use hold zero
//   (L - 1) x T   cmax likewise
//   F x uint32    latch bits of every filter (bit k: threshold k)
//   uint32        carried columns, saturating at L - 1
// rounded up to a multiple of 16 bytes.  All zeros: the start of a stream.
__host__ __device__ inline size_t state_used_bytes(int n_filters, int window, int elem)
{
    return 2 * (size_t)(window - 1) * elem + 4 * (size_t)n_filters + 4;
}
__host__ __device__ inline size_t state_block_bytes(int n_filters, int window, int elem)
{
    return state_round16(state_used_bytes(n_filters, window, elem));
}
inline size_t lds_bytes(int n_filters, int window, int elem)
{
    return (2 * (size_t)(window - 1 + ADP_CHUNK) + 2 * (size_t)ADP_WAVES * ADP_CHUNK) * elem + 4 * (size_t)n_filters;
}
inline bool shape_ok(int n_filters, int window)
{
    return n_filters >= 1 && n_filters <= ADP_MAX_FILTERS && window >= 1 && window <= ADP_MAX_WINDOW;
}

template <typename T>
struct AdaptiveArgs {
    const T *db;                        // (n_streams, F, H)
    const int32_t *stream_cols;         // (n_streams) or null
    const unsigned char *state_in;      // or null
    unsigned char *state_out;           // or null; may be state_in
    uint8_t *raster;                    // (n_streams, F * R, H * n_thr)
    T *lo_out, *hi_out;                 // (n_streams, H) or null
    int n_cols, n_filters, window, n_thr, redundancy;
    T on[MAX_THR], off[MAX_THR];
};

// the waves' partial extrema of a lane's column, joined in wave order (the order does not matter: SPEC.md §1.9)
template <typename T>
__device__ __forceinline__ void join_waves(const T *pmin, const T *pmax, int lane, T &mn, T &mx)
{
    mn = pmin[lane]; mx = pmax[lane];
#pragma unroll
    for (int w = 1; w < ADP_WAVES; ++w) {
        const T a = pmin[w * ADP_CHUNK + lane], b = pmax[w * ADP_CHUNK + lane];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
}

template <typename T>
__global__ __launch_bounds__(ADP_THREADS) void adaptive_encode_kernel(const AdaptiveArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char adp_smem[];
    const int F = a.n_filters, H = a.n_cols, L = a.window, nq = a.n_thr, R = a.redundancy;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cap = L - 1 + ADP_CHUNK;
    T *emin = reinterpret_cast<T *>(adp_smem);                  // [cap] carried extrema, then the chunk's
    T *emax = emin + cap;
    T *pmin = emax + cap;                                       // [wave][lane] partial extrema
    T *pmax = pmin + ADP_WAVES * ADP_CHUNK;
    uint32_t *latch = reinterpret_cast<uint32_t *>(pmax + ADP_WAVES * ADP_CHUNK);   // [F]

    const int hb = __builtin_amdgcn_readfirstlane(stream_count(a.stream_cols, b, H));   // workgroup-uniform
    const size_t block = state_block_bytes(F, L, (int)sizeof(T));
    // (the block's pointers formed here and not by state_block: the compiler keeps its register use only this way)
    const unsigned char *sin = a.state_in ? a.state_in + (size_t)b * block : nullptr;
    unsigned char *sout = a.state_out ? a.state_out + (size_t)b * block : nullptr;
    const StateBlock blk{sin, sout, sout != nullptr && sout != sin};
    if (hb == 0) {
        carry_idle_block<ADP_THREADS>(blk, block, tid);
        return;
    }

    // ---- the state: carried extrema to the front of `ext`, the latches, the count ----
    const T *smin = reinterpret_cast<const T *>(sin);
    const T *smax = smin + (L - 1);
    const uint32_t *slat = reinterpret_cast<const uint32_t *>(sin + 2 * (size_t)(L - 1) * sizeof(T));
    int cnt = 0;
    if (sin) cnt = __builtin_amdgcn_readfirstlane((int)min(slat[F], (uint32_t)(L - 1)));   // clamped: never an index outside `ext`
    for (int i = tid; i < cnt; i += ADP_THREADS) { emin[i] = smin[i]; emax[i] = smax[i]; }
    for (int i = tid; i < F; i += ADP_THREADS) latch[i] = sin ? slat[i] : 0u;
    __syncthreads();

    const T *db = a.db + (size_t)b * F * H;
    const size_t row_bytes = (size_t)H * nq;
    uint8_t *dst = a.raster + (size_t)b * F * R * row_bytes;

    for (int c0 = 0; c0 < hb; c0 += ADP_CHUNK) {
        const int n = min(ADP_CHUNK, hb - c0);                  // columns of this chunk
        const bool valid = lane < n;
        const int col = c0 + (valid ? lane : n - 1);            // lanes past the chunk repeat its last column, nothing is kept
        // ---- 1. column extrema ----
        {
            T mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
            for (int f = wv; f < F; f += ADP_WAVES) {
                const T v = db[(size_t)f * H + col];
                mx = v > mx ? v : mx;                           // a NaN compares false: skipped
                mn = v < mn ? v : mn;
            }
            pmin[wv * ADP_CHUNK + lane] = mn;
            pmax[wv * ADP_CHUNK + lane] = mx;
        }
        __syncthreads();
        if (tid < n) {
            T mn, mx;
            join_waves(pmin, pmax, tid, mn, mx);
            emin[cnt + tid] = mn;
            emax[cnt + tid] = mx;
        }
        __syncthreads();
        // ---- 2. window extrema: entries max(0, e - L + 1) .. e of `ext`, e the lane's column ----
        {
            const int e = cnt + (valid ? lane : n - 1);
            T mn = INFINITY, mx = -INFINITY;
            for (int i = max(0, e - L + 1) + wv; i <= e; i += ADP_WAVES) {
                const T lo_i = emin[i], hi_i = emax[i];
                mn = lo_i < mn ? lo_i : mn;
                mx = hi_i > mx ? hi_i : mx;
            }
            pmin[wv * ADP_CHUNK + lane] = mn;
            pmax[wv * ADP_CHUNK + lane] = mx;
        }
        __syncthreads();
        T mn, hi;
        join_waves(pmin, pmax, lane, mn, hi);
        // the floor comes before the minimum (create_dataset.py:60)
        const T fl = hi - (T)80.0;
        const T lo = mn > fl ? mn : fl;
        const bool flat = (hi - lo) < (T)1e-8;                  // also a window with no non-NaN value: -inf < 1e-8
        const T den = (hi - lo) + (T)1e-8;
        if (wv == 0 && valid) {
            if (a.lo_out) a.lo_out[(size_t)b * H + col] = lo;
            if (a.hi_out) a.hi_out[(size_t)b * H + col] = hi;
        }
        // ---- 3. values, comparison bits, latches, raster bytes: a wave a filter row ----
        for (int f0 = wv; f0 < F; f0 += ADP_ROWS * ADP_WAVES) {
            T vs[ADP_ROWS];                                     // their loads together; a row past the end repeats the last one
#pragma unroll
            for (int e = 0; e < ADP_ROWS; ++e) vs[e] = db[(size_t)min(f0 + e * ADP_WAVES, F - 1) * H + col];
#pragma unroll
            for (int e = 0; e < ADP_ROWS; ++e) {
                const int f = f0 + e * ADP_WAVES;
                if (f >= F) break;                                  // wave-uniform
                const T v = vs[e];
                const T val = flat ? (T)0 : lsm_fe::floored_value(v, fl, lo, den);
                const uint32_t act = latch[f];                      // wave-uniform
                uint32_t next = 0u, mine = 0u;
#pragma unroll
                for (int q = 0; q < MAX_THR; ++q) {
                    if (q < nq) {
                        const uint64_t up = __ballot(valid && val > a.on[q]);
                        const uint64_t dn = __ballot(valid && val < a.off[q]);
                        uint64_t res, carry = (act >> q) & 1u;
                        if ((up & dn) == 0ull) {
                            // active' = above | (active & ~below): the carry chain of p + g, generate = above, propagate = ~below,
                            // 32 columns per 64-bit addition.  Columns past the chunk propagate: the carry out is the latch after
                            // the chunk's last column.
                            uint64_t g = (uint32_t)up, p = (uint32_t)~dn;
                            uint64_t c = (p + g + carry) ^ p ^ g;   // bit k: carry into bit k; bit k + 1: the latch after column k
                            res = (uint32_t)(c >> 1);
                            carry = (c >> 32) & 1u;
                            g = (uint32_t)(up >> 32); p = (uint32_t)~(dn >> 32);
                            c = (p + g + carry) ^ p ^ g;
                            res |= (uint64_t)(uint32_t)(c >> 1) << 32;
                            carry = (c >> 32) & 1u;
                        } else {
                            // an off-threshold ABOVE its on-threshold (negative gap): a value between them flips the latch
                            res = 0ull;
                            for (int k = 0; k < 64; ++k) {
                                carry = carry ? (~(dn >> k) & 1ull) : ((up >> k) & 1ull);
                                res |= carry << k;
                            }
                        }
                        next |= (uint32_t)carry << q;
                        mine |= (uint32_t)((res >> lane) & 1ull) << q;
                    }
                }
                if (lane == 0) latch[f] = next;                     // read again by this wave only, in the next chunk
                // (the rows taken at the lane's column, so that the column's offset is formed once for the R rows)
                if (valid) lsm_fe::store_column(dst + (size_t)f * R * row_bytes + (size_t)col * nq, row_bytes, 0, nq, R, mine);
            }
        }
        // ---- 4. the last min(L - 1, cnt + n) entries move to the front: new[j] = old[j + shift], minimum and maximum as a pair
        //      (stream_state.h; here the entries past `keep` are in `ext` as well) ----
        const int keep = min(L - 1, cnt + n), shift = cnt + n - keep;
        if (shift > 0) {
            struct Ext { T mn, mx; };
            const auto at = [&](const int i) { return Ext{emin[i], emax[i]}; };
            shift_history<ADP_THREADS>(keep, shift, tid, at, [&](const int i) { return at(keep + i); },
                                       [&](const int j, const Ext &e) { emin[j] = e.mn; emax[j] = e.mx; });
        }
        cnt = keep;
        __syncthreads();                                        // `ext`, the partial extrema and the latches are the next chunk's
    }

    // ---- the state out: the carried extrema, zeros in the slots not in use, the latches, the count; the padding travels ----
    if (sout) {
        T *dmin = reinterpret_cast<T *>(sout);
        T *dmax = dmin + (L - 1);
        uint32_t *dlat = reinterpret_cast<uint32_t *>(sout + 2 * (size_t)(L - 1) * sizeof(T));
        for (int i = tid; i < L - 1; i += ADP_THREADS) {
            dmin[i] = i < cnt ? emin[i] : (T)0;
            dmax[i] = i < cnt ? emax[i] : (T)0;
        }
        for (int i = tid; i < F; i += ADP_THREADS) dlat[i] = latch[i];
        if (tid == 0) dlat[F] = (uint32_t)cnt;
        carry_padding<unsigned char>(blk, state_used_bytes(F, L, (int)sizeof(T)), block, tid);
    }
}

template <typename T>
int adaptive_encode(const T *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols, int window_cols,
                    const T *thr_on, const T *thr_off, int n_thr, int redundancy, const void *state_in, void *state_out,
                    uint8_t *raster_out, T *lo_out, T *hi_out, void *stream)
{
    LSM_REQUIRE(n_filters >= 1 && n_filters <= ADP_MAX_FILTERS, "n_filters=%d outside [1, %d]", n_filters, ADP_MAX_FILTERS);
    LSM_REQUIRE(n_streams >= 0, "n_streams=%d must be >= 0", n_streams);
    LSM_REQUIRE(window_cols >= 1 && window_cols <= ADP_MAX_WINDOW, "window_cols=%d outside [1, %d]", window_cols,
                ADP_MAX_WINDOW);
    LSM_REQUIRE(n_cols >= 1, "n_cols=%d: a launch's row stride H must be >= 1", n_cols);
    LSM_REQUIRE(n_thr >= 1 && n_thr <= MAX_THR, "n_thr=%d outside [1, %d]", n_thr, MAX_THR);
    LSM_REQUIRE(redundancy >= 1, "redundancy must be >= 1");
    LSM_REQUIRE(thr_on && thr_off, "null threshold table");
    LSM_REQUIRE(raster_out != nullptr, "raster_out is required");
    LSM_REQUIRE_ALIGNED(raster_out, 4);
    LSM_REQUIRE_ALIGNED(stream_cols, 4);
    LSM_REQUIRE_ALIGNED(db, sizeof(T));
    LSM_REQUIRE_ALIGNED(lo_out, sizeof(T));
    LSM_REQUIRE_ALIGNED(hi_out, sizeof(T));
    LSM_REQUIRE_ALIGNED(state_in, 16);
    LSM_REQUIRE_ALIGNED(state_out, 16);
    if (n_streams == 0) return LSM_OK;
    LSM_REQUIRE(db != nullptr, "adaptive_encode: null db");
    AdaptiveArgs<T> a;
    a.db = db; a.stream_cols = stream_cols;
    a.state_in = static_cast<const unsigned char *>(state_in);
    a.state_out = static_cast<unsigned char *>(state_out);
    a.raster = raster_out; a.lo_out = lo_out; a.hi_out = hi_out;
    a.n_cols = n_cols; a.n_filters = n_filters; a.window = window_cols; a.n_thr = n_thr; a.redundancy = redundancy;
    lsm_fe::fill_thresholds<T>(a.on, a.off, thr_on, thr_off, n_thr);
    const size_t lds = lds_bytes(n_filters, window_cols, (int)sizeof(T));
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(adaptive_encode_kernel<T>));
    hipLaunchKernelGGL(adaptive_encode_kernel<T>, dim3((unsigned)n_streams), dim3(ADP_THREADS), lds, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

}  // namespace

LSM_API long lsm_adaptive_state_bytes(int n_filters, int window_cols, int elem_bytes)
{
    if (!shape_ok(n_filters, window_cols) || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return (long)state_block_bytes(n_filters, window_cols, elem_bytes);
}

LSM_API int lsm_adaptive_encode_f64(const double *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols,
                                    int window_cols, const double *thr_on, const double *thr_off, int n_thr, int redundancy,
                                    const void *state_in, void *state_out, uint8_t *raster_out, double *lo_out,
                                    double *hi_out, void *stream)
{
    return adaptive_encode<double>(db, n_streams, n_cols, n_filters, stream_cols, window_cols, thr_on, thr_off, n_thr,
                                   redundancy, state_in, state_out, raster_out, lo_out, hi_out, stream);
}

LSM_API int lsm_adaptive_encode_f32(const float *db, int n_streams, int n_cols, int n_filters, const int32_t *stream_cols,
                                    int window_cols, const float *thr_on, const float *thr_off, int n_thr, int redundancy,
                                    const void *state_in, void *state_out, uint8_t *raster_out, float *lo_out, float *hi_out,
                                    void *stream)
{
    return adaptive_encode<float>(db, n_streams, n_cols, n_filters, stream_cols, window_cols, thr_on, thr_off, n_thr,
                                  redundancy, state_in, state_out, raster_out, lo_out, hi_out, stream);
}
