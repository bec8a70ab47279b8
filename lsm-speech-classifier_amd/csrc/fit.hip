// Streaming ridge fit for gfx950 (SPEC.md §7, include/lsm_hip_fit.h): one launch adds a block of feature rows to the lower
// triangle of X^T X, the per-class sums, the class counts and the column ranges.
//
// Layout.  Every output element is owned by exactly one thread for the whole launch, which reads it once, runs over the rows
// in ascending order and stores it once: no split over rows, no atomics, no scratch.  One grid of 256-thread workgroups in
// three roles, told apart by the block index (uniform over a workgroup):
//   range   ceil(D / 256) workgroups: thread d keeps col_min[d] and col_max[d] and reads its column of every row.
//   class   ceil(D / 256) * C workgroups, one per (column chunk, class c): thread d keeps class_sums[c][d].  The workgroup
//           compacts the rows labelled c, 256 labels at a time (ballot and prefix count, ascending), and only those rows are
//           read -- over all classes every row once --, four loads in flight, added in order.  The chunk-0 workgroup of a
//           class also owns class_counts[c].
//   gram    nt * (nt + 1) / 2 workgroups, nt = ceil(D / TILE): one TILE x TILE tile (ti, tj), tj <= ti, of the triangle.  A
//           thread owns 4 x 4 entries as sixteen float64 accumulators: rows i0 + 4 * ty + a, columns j0 + 2 * tx + {0, 1}
//           and j0 + 32 + 2 * tx + {0, 1} (so that a 16-lane group of a 128-bit LDS read covers 256 contiguous bytes).  The
//           feature rows go through LDS STAGE rows at a time, already converted to float64: TILE columns for the tile's rows
//           and TILE for its columns (one image on the diagonal), loaded into registers one stage ahead.  A skipped row is
//           a uniform branch around its sixteen fused multiply-adds.  Entries with j > i or behind D are never loaded or
//           stored; a staged column behind D is 0.0 and a staged row behind n_rows is never used.
// The small roles come first in the grid: they are bound by latency, not by arithmetic, and finish under the tiles.
#include "lsm_common.h"

namespace {

constexpr int TILE = 64, STAGE = 16;             // LSM_FIT_TILE and LSM_FIT_STAGE_ROWS of include/lsm_hip_fit.h
constexpr int THREADS = 256, CHUNK = 256;
constexpr int MAX_D = 16384, MAX_CLASSES = 64;
static_assert(TILE == 64 && THREADS == 256, "the thread tiles below are written for a 64 x 64 tile of 256 threads");
static_assert(STAGE >= 1 && STAGE <= 32 && (2 * STAGE * TILE) % THREADS == 0, "a stage is shared out evenly, its rows one mask");

struct FitArgs {
    const float *x;                 // (n_rows, D)
    const int32_t *labels;          // (n_rows)
    double *gram, *class_sums;      // (D, D), (C, D)
    long long *class_counts;        // (C)
    float *col_min, *col_max;       // (D)
    int n_rows, D, C, n_chunks;
};

__device__ __forceinline__ bool in_range(int y, int C) { return (unsigned)y < (unsigned)C; }

__device__ void range_role(const FitArgs &a, int chunk)
{
    const int d = chunk * CHUNK + (int)threadIdx.x;
    if (d >= a.D) return;                                            // no barrier in this role
    float mn = a.col_min[d], mx = a.col_max[d];
    const float *col = a.x + d;
#pragma unroll 8
    for (int r = 0; r < a.n_rows; ++r) {
        const float v = col[(size_t)r * a.D];
        if (in_range(a.labels[r], a.C)) {                            // uniform
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
    }
    a.col_min[d] = mn;
    a.col_max[d] = mx;
}

__device__ void class_role(const FitArgs &a, int chunk, int c)
{
    __shared__ int s_rows[CHUNK];
    __shared__ int s_wave[THREADS / LSM_WAVE];
    const int tid = threadIdx.x, lane = tid & (LSM_WAVE - 1), wave = tid / LSM_WAVE;
    const int d = chunk * CHUNK + tid;
    const bool mine = d < a.D;                                       // the others only help with the labels
    const float *col = a.x + (mine ? d : 0);
    double sum = mine ? a.class_sums[(size_t)c * a.D + d] : 0.0;
    long long count = 0;
    for (int r0 = 0; r0 < a.n_rows; r0 += CHUNK) {                   // uniform: every thread meets every barrier
        const int r = r0 + tid;
        const bool hit = r < a.n_rows && a.labels[r] == c;
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / LSM_WAVE; ++w) {
            before += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (hit) s_rows[before + __popcll(ballot & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (mine) {
            for (int k = 0; k < total; k += 4) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = k + u < total ? col[(size_t)s_rows[k + u] * a.D] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u < total) sum = sum + (double)v[u];     // uniform
            }
        }
        count += total;
        __syncthreads();                                             // the list has been read
    }
    if (mine) a.class_sums[(size_t)c * a.D + d] = sum;
    if (chunk == 0 && tid == 0) a.class_counts[c] = a.class_counts[c] + count;
}

__device__ void gram_role(const FitArgs &a, int pair)
{
    __shared__ __attribute__((aligned(16))) double s_a[STAGE][TILE];
    __shared__ __attribute__((aligned(16))) double s_b[STAGE][TILE];
    // pair = ti * (ti + 1) / 2 + tj, 0 <= tj <= ti
    int ti = (int)((sqrtf(8.0f * (float)pair + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= pair) ++ti;
    while (ti * (ti + 1) / 2 > pair) --ti;
    const int tj = pair - ti * (ti + 1) / 2;
    const bool diagonal = ti == tj;
    const int i0 = ti * TILE, j0 = tj * TILE;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const double (*sb)[TILE] = diagonal ? s_a : s_b;

    int jl[4];                                                       // the thread's columns inside the tile
#pragma unroll
    for (int b = 0; b < 4; ++b) jl[b] = (b >> 1) * 32 + tx * 2 + (b & 1);
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty * 4 + p, j = j0 + jl[b];
            acc[p][b] = (i < a.D && j <= i) ? a.gram[(size_t)i * a.D + j] : 0.0;
        }
    }

    // what this thread stages: element e = tid + THREADS * k of (2, STAGE, TILE); the second image is skipped on the diagonal
    constexpr int PER = 2 * STAGE * TILE / THREADS;
    const int n_mine = diagonal ? PER / 2 : PER;
    float pre[PER];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = tid + THREADS * k, image = e / (STAGE * TILE), rr = (e / TILE) % STAGE, cc = e % TILE;
            const int r = r0 + rr, col = (image ? j0 : i0) + cc;
            pre[k] = (k < n_mine && r < a.n_rows && col < a.D) ? a.x[(size_t)r * a.D + col] : 0.0f;
        }
    };
    fetch(0);
    for (int r0 = 0; r0 < a.n_rows; r0 += STAGE) {                   // uniform: every thread meets every barrier
        if (r0) __syncthreads();                                     // the stage before has been read
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = tid + THREADS * k, image = e / (STAGE * TILE), rr = (e / TILE) % STAGE, cc = e % TILE;
            if (k < n_mine) (image ? s_b : s_a)[rr][cc] = (double)pre[k];
        }
        unsigned valid = 0;                                          // uniform loads: the rows of this stage that count
#pragma unroll
        for (int rr = 0; rr < STAGE; ++rr)
            if (r0 + rr < a.n_rows && in_range(a.labels[r0 + rr], a.C)) valid |= 1u << rr;
        __syncthreads();
        if (r0 + STAGE < a.n_rows) fetch(r0 + STAGE);                // in flight under the arithmetic below
#pragma unroll
        for (int rr = 0; rr < STAGE; ++rr) {
            if (!((valid >> rr) & 1u)) continue;                     // uniform
            const double2 a01 = *reinterpret_cast<const double2 *>(&s_a[rr][ty * 4]);
            const double2 a23 = *reinterpret_cast<const double2 *>(&s_a[rr][ty * 4 + 2]);
            const double2 b01 = *reinterpret_cast<const double2 *>(&sb[rr][tx * 2]);
            const double2 b23 = *reinterpret_cast<const double2 *>(&sb[rr][32 + tx * 2]);
            const double xi[4] = {a01.x, a01.y, a23.x, a23.y}, xj[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[p][b] = __builtin_fma(xi[p], xj[b], acc[p][b]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty * 4 + p, j = j0 + jl[b];
            if (i < a.D && j <= i) a.gram[(size_t)i * a.D + j] = acc[p][b];
        }
    }
}

__global__ __launch_bounds__(THREADS) void fit_kernel(const FitArgs a)
{
    const int block = blockIdx.x, n_class_blocks = a.n_chunks * a.C;
    if (block < a.n_chunks)
        range_role(a, block);
    else if (block < a.n_chunks + n_class_blocks)
        class_role(a, (block - a.n_chunks) % a.n_chunks, (block - a.n_chunks) / a.n_chunks);
    else
        gram_role(a, block - a.n_chunks - n_class_blocks);
}

bool aligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

LSM_API int lsm_fit_supported(int n_keys, int n_out, int n_classes)
{
    return n_keys >= 1 && n_keys <= 8 && n_out >= 1 && (long)n_keys * n_out <= MAX_D && n_classes >= 1
                   && n_classes <= MAX_CLASSES ? 1 : 0;
}

LSM_API int lsm_fit_accumulate_f32(const float *features, const int32_t *labels, int n_rows, int n_keys, int n_out,
                                   int n_classes, double *gram, double *class_sums, int64_t *class_counts, float *col_min,
                                   float *col_max, void *stream)
{
    LSM_REQUIRE(n_rows >= 0, "n_rows=%d must be >= 0", n_rows);
    LSM_REQUIRE(n_keys >= 1 && n_keys <= 8, "n_keys=%d must be in [1, 8]", n_keys);
    LSM_REQUIRE(n_out >= 1, "n_out=%d must be >= 1", n_out);
    LSM_REQUIRE((long)n_keys * n_out <= MAX_D, "D = n_keys * n_out = %ld must be <= %d", (long)n_keys * n_out, MAX_D);
    LSM_REQUIRE(n_classes >= 1 && n_classes <= MAX_CLASSES, "n_classes=%d must be in [1, %d]", n_classes, MAX_CLASSES);
    LSM_REQUIRE(gram && class_sums && class_counts && col_min && col_max,
                "fit: gram, class_sums, class_counts, col_min and col_max are required");
    LSM_REQUIRE(aligned(gram, 8) && aligned(class_sums, 8) && aligned(class_counts, 8),
                "gram, class_sums and class_counts must be 8-byte aligned");
    LSM_REQUIRE(aligned(features, 4) && aligned(labels, 4) && aligned(col_min, 4) && aligned(col_max, 4),
                "features, labels, col_min and col_max must be 4-byte aligned");
    if (n_rows == 0) return LSM_OK;
    LSM_REQUIRE(features && labels, "fit: null features or labels");
    FitArgs a{};
    a.x = features; a.labels = labels; a.gram = gram; a.class_sums = class_sums;
    a.class_counts = reinterpret_cast<long long *>(class_counts); a.col_min = col_min; a.col_max = col_max;
    a.n_rows = n_rows; a.D = n_keys * n_out; a.C = n_classes; a.n_chunks = (a.D + CHUNK - 1) / CHUNK;
    const int nt = (a.D + TILE - 1) / TILE;
    const unsigned blocks = (unsigned)(a.n_chunks * (1 + a.C) + nt * (nt + 1) / 2);
    hipLaunchKernelGGL(fit_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
