// spikes_body.h -- dB spectrogram of one clip -> normalised spectrogram -> hysteresis spike raster, as a device
// function (/root/reference/create_dataset.py:62-104: min-max normalise with the gammatone branch's floor, zoom to
// TIME_BINS columns, crop, convert_spectrogram_to_spikes_hysteresis, create_pure_redundancy).
#pragma once
#include "lsm_common.h"

namespace lsm_fe {

template <typename T> struct Acc;          // arithmetic type of the normalise step per input dtype
template <> struct Acc<double> { typedef double type; };
template <> struct Acc<float> { typedef float type; };

constexpr int MAX_THR = 8;

template <typename T>
struct SpikeArgs {
    const T *db;            // (B, F, ncols)
    int n_clips, n_filters, ncols, time_bins, apply_floor, n_thr, redundancy;
    T on[MAX_THR], off[MAX_THR];
    uint8_t *raster;        // (B, F*redundancy, time_bins*n_thr) or null
    T *norm_out;            // (B, F, time_bins) or null
};

// SpecAugment-style masks of a batch (SPEC.md 1.13), the masked kernels' argument beside their twins' own: one bit per filter
// row / time bin and clip, bit i in bit i & 31 of word i >> 5; either pointer may be null (no mask of that kind)
struct MaskArgs {
    const uint32_t *freq;   // (n_clips, ceil(n_filters / 32)) or null
    const uint32_t *time;   // (n_clips, ceil(time_bins / 32)) or null
};

// Per-clip lengths of a ragged batch (SPEC.md 1.14), the ragged kernels' argument beside their twins' own: DEVICE int32
// arrays of n_clips entries that no host code reads; the kernels clamp what they find (clip_counts below, and the fused
// kernel's own statement of it).
struct RaggedCounts {       // the split encoder
    const int *cols;        // dB columns of clip b
    const int *bins;        // time bins of clip b
};
struct RaggedArgs {         // the fused gammatone kernel
    const int *bins;        // time bins of clip b; its columns are bins - (time_bins - ncols)
    int *steps_out;         // bins * n_thr per clip, or null
};

// A clip's counts as the ragged encoder uses them, whatever the arrays hold: bins 0 or 3..time_bins, columns 1..ncols; a clip
// without a column or with fewer than 3 bins is empty (0 bins, 0 columns).
__device__ __forceinline__ void clip_counts(const RaggedCounts &rc, int b, int ncols, int time_bins, int &nc, int &Tb)
{
    const int c = min(max(rc.cols[b], 0), ncols), t = min(max(rc.bins[b], 0), time_bins);
    const bool live = c >= 1 && t >= 3;
    nc = live ? c : 0;
    Tb = live ? t : 0;
}

// ---- the column tail of the streamed encoders: one dB value of a column -> normalised value -> latch -> raster bytes ----

// The launch functions' threshold tables: entries from n_thr on hold the pads.  The default pads never fire -- nothing is
// > +inf or < -inf -- so a kernel may compare all MAX_THR entries.
template <typename T>
void fill_thresholds(T (&on)[MAX_THR], T (&off)[MAX_THR], const T *thr_on, const T *thr_off, int n_thr, T pad_on = (T)INFINITY,
                     T pad_off = (T)-INFINITY)
{
    for (int q = 0; q < MAX_THR; ++q) {
        on[q] = q < n_thr ? thr_on[q] : pad_on;
        off[q] = q < n_thr ? thr_off[q] : pad_off;
    }
}

// A dB value floored at `fl` and normalised to the range [lo, lo + den).  A NaN stays a NaN through the floor and compares
// false with every threshold: the latches keep their state.
template <typename T>
__device__ __forceinline__ T floored_value(T v, T fl, T lo, T den)
{
    const T vf = v < fl ? fl : v;
    return (vf - lo) / den;
}

// (The MAX_THR-wide compare of a value with the launch's tables stays written out in the two kernels that have it: handed to
// a function, the tables' kernel-argument loads are grouped differently and the kernels need more scalar registers.)

// rising and falling are both taken from the latch before the update (SPEC.md §1.3)
__device__ __forceinline__ uint32_t latch_step(uint32_t act, uint32_t up, uint32_t dn, uint32_t tmask)
{
    return ((up & ~act) | (act & ~dn)) & tmask;
}

// Column `col` of one filter's raster rows, threshold t's byte from bit t of `bits`: a word where n_thr = 4 (the multiply
// spreads bits 0..3 over the word's four bytes), bytes otherwise.  Redundancy: the filter's R output rows, `rrow` the
// first, repeat it (SPEC.md §1.4).
__device__ __forceinline__ void store_column(uint8_t *rrow, size_t row_bytes, int col, int n_thr, int R, uint32_t bits)
{
    if (n_thr == 4) {
        const uint32_t word = (bits * 0x00204081u) & 0x01010101u;
        for (int r = 0; r < R; ++r) *reinterpret_cast<uint32_t *>(rrow + (size_t)r * row_bytes + (size_t)col * 4) = word;
    } else {
        for (int r = 0; r < R; ++r)
            for (int t = 0; t < n_thr; ++t) rrow[(size_t)r * row_bytes + (size_t)col * n_thr + t] = (uint8_t)((bits >> t) & 1u);
    }
}

template <typename T>
__device__ __forceinline__ T block_reduce(T v, bool is_max, T *scratch)
{
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = is_max ? (o > v ? o : v) : (o < v ? o : v);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[w] = v;
    __syncthreads();
    T r = scratch[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i)
        r = is_max ? (scratch[i] > r ? scratch[i] : r) : (scratch[i] < r ? scratch[i] : r);
    return r;
}

constexpr int SPK_ROWS = 64;               // spectrogram rows (filters) a workgroup encodes at a time

// LDS bytes of spec_to_spikes_body: 128 of reduction scratch (sixteen waves) + two bit arrays (value above the on-threshold / below the
// off-threshold; the first becomes the latch state) of SPK_ROWS rows x n_thr thresholds x ceil(time_bins / 32) words
__host__ __device__ inline size_t spikes_lds_bytes(int time_bins, int n_thr)
{
    return 128 + 2 * (size_t)SPK_ROWS * (size_t)(n_thr > 0 ? n_thr : 1) * (size_t)((time_bins + 31) / 32) * 4;
}

// One workgroup of 4 to 16 waves, one clip `b`: min/max, floor, normalise, SciPy-exact resize, hysteresis latches, raster.
// `smem`: spikes_lds_bytes(time_bins, n_thr).  Shared by spec_to_spikes_kernel (frontend.hip) and the one-launch mel front
// end (mel.hip), whose last workgroup of a clip runs it on the dB values it has just formed.
// Three passes over groups of SPK_ROWS rows (round 5; before, ONE thread walked a row's time bins, its two loads per bin
// in series with the latch: 40 busy threads and 71 us per 200 clips at 40 filters):
//   1. every wave takes rows, a lane a time bin: normalised value (the reference's arithmetic, element by element), then
//      one ballot per threshold and comparison -> the bit rows "above on[q]" and "below off[q]";
//   2. one thread per (row, threshold) runs the latch over the bits: active' = active ? !below : above
//      (create_dataset.py:88-96: rising and falling are both taken from the latch before the update), 32 bins per addition;
//   3. the raster bytes, four per store, from the latch bits.
// MASK (SPEC.md 1.13): a value whose row or time bin is masked becomes +0.0 where the zero bin's does, after maximum, floor,
// minimum and resize.  The row is wave-uniform (its bit is a scalar), the 64 time bits of a piece are one 64-bit scalar.
// RAGGED (SPEC.md 1.14): clip b has its own columns and bins (`rc`, clamped by clip_counts); a.ncols and a.time_bins are then
// the strides of db, raster and norm_out -- and size the LDS -- while the minimum and maximum, zf, jz, the no-zoom case, the
// flat test and a row's bit count are the clip's.  Past the clip's bins the raster rows and norm_out are written as 0.
template <typename T, bool MASK = false, bool RAGGED = false>
__device__ __forceinline__ void spec_to_spikes_body(const SpikeArgs<T> &a, const int b, unsigned char *smem,
                                                    const MaskArgs m = MaskArgs{nullptr, nullptr},
                                                    const RaggedCounts rc = RaggedCounts{nullptr, nullptr})
{
    T *scratch = reinterpret_cast<T *>(smem);                 // 16 entries: one per wave of up to 1024 threads
    const int F = a.n_filters, ncs = a.ncols, Tbs = a.time_bins, nq = a.n_thr;      // ncs, Tbs: the launch's strides
    int nc_clip = 0, tb_clip = 0;
    if constexpr (RAGGED) clip_counts(rc, b, ncs, Tbs, nc_clip, tb_clip);
    const int nc = RAGGED ? nc_clip : ncs, Tb = RAGGED ? tb_clip : Tbs;
    const int W = (Tb + 31) >> 5;                             // words of a bit row
    uint32_t *onb = reinterpret_cast<uint32_t *>(smem + 128); // [row in group][q][W]: above on[q]; then the latch state
    uint32_t *offb = onb + (size_t)SPK_ROWS * (nq > 0 ? nq : 1) * W;
    const T *db = a.db + (size_t)b * F * ncs;
    const int n = F * nc;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwv = (int)(blockDim.x >> 6);

    if constexpr (RAGGED) {
        const int rest = Tbs - Tb;                            // bins of a row the clip does not own
        if (a.norm_out)
            for (int i = tid; i < F * rest; i += blockDim.x) {
                const int r = i / rest;
                a.norm_out[((size_t)b * F + r) * Tbs + Tb + (i - r * rest)] = (T)0;
            }
        if (Tb == 0) {                                        // an empty clip: zero rows (uniform over the workgroup)
            if (a.raster) {
                const size_t nb = (size_t)F * a.redundancy * Tbs * nq;
                for (size_t i = tid; i < nb; i += blockDim.x) a.raster[(size_t)b * nb + i] = 0;
            }
            return;
        }
    }

    T mx = -INFINITY, mn = INFINITY;
    int nan_seen = 0;
    if constexpr (RAGGED) {
        for (int i = tid; i < n; i += blockDim.x) {
            const int r = i / nc;
            const T v = db[(size_t)r * ncs + (i - r * nc)];
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
            nan_seen |= v != v;
        }
    } else {
#pragma unroll 8
        for (int i = tid; i < n; i += blockDim.x) {
            const T v = db[i];
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
            nan_seen |= v != v;
        }
    }
    mx = block_reduce(mx, true, scratch);
    mn = block_reduce(mn, false, scratch);
    // ndarray.max() / .min() / np.maximum (create_dataset.py:59-63) propagate NaN, the comparisons above skip it: one NaN
    // among the dB values makes the maximum, the floor and the minimum NaN, hence every normalised value NaN and the
    // raster all zeros (tests/golden/postfilter_nonfinite.npz: the reference's own output for such inputs)
    if (__syncthreads_or(nan_seen)) mx = mn = (T)NAN;
    // create_dataset.py:60 floors at max-80 before the min is taken: min' = max(min, max-80)
    const T fl = a.apply_floor ? mx - (T)80.0 : -INFINITY;
    const T lo = (mn > fl || mn != mn) ? mn : fl;
    const T hi = mx;
    const bool flat = (hi - lo) < (T)1e-8;
    const T den = (hi - lo) + (T)1e-8;
    const int row_bytes = Tb * nq;                            // the clip's bytes of a raster row
    const int rbs = RAGGED ? Tbs * nq : row_bytes;            // the row's length in memory
    const double zf = (double)(nc - 1) / (double)(Tb - 1);
    // Where the last bin's coordinate (Tb-1)*zf rounds to a double ABOVE nc-1 it lies outside the input, and SciPy's constant
    // boundary mode answers cval = +0.0 for that bin, whatever the row holds (SPEC.md 1.2).  The overshoot is an ulp, so no
    // earlier bin has it: one uniform test per launch, jz = the bin that is zero (-1: none).
    const int jz = (nc != Tb && (double)(Tb - 1) * zf > (double)(nc - 1)) ? Tb - 1 : -1;
    const int C = F * a.redundancy;
    uint8_t *dst = a.raster ? a.raster + (size_t)b * C * rbs : nullptr;
    const uint32_t *fmc = nullptr, *tmc = nullptr;            // this clip's mask words
    if constexpr (MASK) {
        fmc = m.freq ? m.freq + (size_t)b * ((F + 31) >> 5) : nullptr;
        // (RAGGED: the mask rows keep the launch's stride; the clip reads the first W words of its row, and the bits at or
        // behind Tb meet lanes that are not `valid`)
        tmc = m.time ? m.time + (size_t)b * (RAGGED ? (Tbs + 31) >> 5 : W) : nullptr;
    }

    for (int r0 = 0; r0 < F; r0 += SPK_ROWS) {
        const int rows = min(SPK_ROWS, F - r0);
        // ---- 1. values and comparison bits: a wave takes (row, 64 time bins) pieces four at a time, their loads together ----
        const int nh = (Tb + 63) >> 6, npiece = rows * nh;
        for (int p0 = wv; p0 < npiece; p0 += 4 * nwv) {
            T x0[4], x1[4];
            double w0[4], w1[4];
            bool two[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pc = min(p0 + e * nwv, npiece - 1);     // (a piece past the end repeats the last one; nothing of it is kept)
                const int rl = pc / nh, j = (pc - rl * nh) * 64 + lane;
                const int jc = j < Tb ? j : Tb - 1;               // (lanes past the row recompute its last bin, likewise)
                const T *row = db + (size_t)(r0 + rl) * ncs;
                if (nc == Tb) {
                    x0[e] = row[jc]; x1[e] = x0[e]; w0[e] = 1.0; w1[e] = 0.0; two[e] = false;
                } else {
                    // scipy.ndimage.zoom(order=1): double coordinate and weights, w1 = 1 - w0
                    const double cc = (double)jc * zf;
                    const double fc = floor(cc);
                    const int f = (int)fc;
                    w0[e] = 1.0 - (cc - fc);
                    w1[e] = 1.0 - w0[e];
                    two[e] = f + 1 <= nc - 1;
                    x0[e] = row[f]; x1[e] = row[two[e] ? f + 1 : f];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pc = p0 + e * nwv;
                if (pc >= npiece) break;                          // wave-uniform
                const int rl = pc / nh, j0 = (pc - rl * nh) * 64, j = j0 + lane;
                const bool valid = j < Tb;
                T val;
                if (flat) {
                    val = (T)0;
                } else if (nc == Tb) {
                    const T c0 = x0[e] > fl ? x0[e] : fl;
                    val = (c0 - lo) / den;
                } else {
                    const T c0 = x0[e] > fl ? x0[e] : fl;
                    const T n0 = (c0 - lo) / den;
                    double acc = (double)n0 * w0[e];
                    if (two[e]) {
                        const T c1 = x1[e] > fl ? x1[e] : fl;
                        const T n1 = (c1 - lo) / den;
                        acc = acc + (double)n1 * w1[e];
                    }
                    val = (T)acc;
                }
                val = j == jz ? (T)0 : val;
                if constexpr (MASK) {
                    const int f = r0 + rl, w = j0 >> 5;           // wave-uniform: scalar loads
                    const uint32_t rowm = fmc ? (fmc[f >> 5] >> (f & 31)) & 1u : 0u;
                    unsigned long long tb = 0ull;                 // the piece's 64 time bits (words past the row: clear)
                    if (tmc) tb = (unsigned long long)tmc[w] | (w + 1 < W ? (unsigned long long)tmc[w + 1] << 32 : 0ull);
                    val = (rowm || ((tb >> lane) & 1ull)) ? (T)0 : val;
                }
                if (a.norm_out && valid) a.norm_out[((size_t)b * F + r0 + rl) * Tbs + j] = val;
#pragma unroll
                for (int q = 0; q < MAX_THR; ++q) {
                    if (q < nq) {
                        const unsigned long long up = __ballot(valid && val > a.on[q]);
                        const unsigned long long dn = __ballot(valid && val < a.off[q]);
                        if (lane == 0) {
                            uint32_t *o = onb + ((size_t)rl * nq + q) * W + (j0 >> 5), *d = offb + ((size_t)rl * nq + q) * W + (j0 >> 5);
                            o[0] = (uint32_t)up; d[0] = (uint32_t)dn;
                            if ((j0 >> 5) + 1 < W) { o[1] = (uint32_t)(up >> 32); d[1] = (uint32_t)(dn >> 32); }
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- 2. the latches: where above and below exclude each other (off <= on), active' = above | (active & ~below) is the
        //      carry chain of an addition: generate = above, propagate = ~below, so a word of 32 time bins is one 64-bit add ----
        for (int i = tid; i < rows * nq; i += blockDim.x) {
            uint32_t *o = onb + (size_t)i * W;
            const uint32_t *d = offb + (size_t)i * W;
            uint64_t active = 0u;
            for (int w = 0; w < W; ++w) {
                const uint32_t up = o[w], dn = d[w];
                if ((up & dn) == 0u) {
                    const uint64_t g = up, p = (uint32_t)~dn;
                    const uint64_t c = (p + g + active) ^ p ^ g;  // bit k: carry INTO bit k; bit k + 1: the latch after bin k
                    o[w] = (uint32_t)(c >> 1);
                    active = (c >> 32) & 1u;
                } else {
                    // an off-threshold ABOVE its on-threshold (negative gap): a value between them flips the latch
                    uint32_t res = 0u, act = (uint32_t)active;
                    for (int k = 0; k < 32; ++k) {
                        act = act ? (~(dn >> k) & 1u) : ((up >> k) & 1u);
                        res |= act << k;
                    }
                    o[w] = res;
                    active = act;
                }
            }
        }
        __syncthreads();
        // ---- 3. raster bytes of the group's rows (create_pure_redundancy: output row c reads filter row c / redundancy) ----
        if (dst) {
            const int c0 = r0 * a.redundancy, nrow = rows * a.redundancy;
            // (RAGGED: a row is rbs bytes long, the clip's latches fill its first row_bytes, the rest is 0)
            if ((rbs & 3) == 0) {
                const int rw = rbs / 4;
                uint32_t *d4 = reinterpret_cast<uint32_t *>(dst) + (size_t)c0 * rw;
                for (int i = tid; i < nrow * rw; i += blockDim.x) {
                    const int c = i / rw;
                    const int p = (i - c * rw) * 4;
                    const uint32_t *o = onb + (size_t)(c / a.redundancy) * nq * W;
                    uint32_t v = 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (RAGGED && p + e >= row_bytes) break;
                        const int j = (p + e) / nq, q = (p + e) - j * nq;           // raster byte p + e = time bin j, threshold q
                        v |= ((o[q * W + (j >> 5)] >> (j & 31)) & 1u) << (8 * e);
                    }
                    d4[i] = v;
                }
            } else {
                uint8_t *d1 = dst + (size_t)c0 * rbs;
                for (int i = tid; i < nrow * rbs; i += blockDim.x) {
                    const int c = i / rbs;
                    const int p = i - c * rbs;
                    const int j = p / nq, q = p - j * nq;
                    d1[i] = (RAGGED && p >= row_bytes) ? (uint8_t)0
                            : (uint8_t)((onb[((size_t)(c / a.redundancy) * nq + q) * W + (j >> 5)] >> (j & 31)) & 1u);
                }
            }
        }
        __syncthreads();                                      // the bit rows are free for the next group
    }
}

}  // namespace lsm_fe
