// Noise mixer for gfx950 (SPEC.md §1.10, include/lsm_hip_mix.h): shift, level and a noise row at a requested SNR, in front
// of the front ends.  Three kernels over the shared pieces of mix_body.h, one workgroup of 256 threads per row each:
//   mix_power_kernel    the row power P of float32 rows;
//   mix_kernel          the batch form: one pass takes Px and Pv, the tree joins both side by side, then the mixing pass;
//                       and its RAGGED form on rows of a stride whose clips have their own lengths (SPEC §1.16), which
//                       then fills the rest of the row with zeros;
//   mix_stream_kernel   the streamed form: the mixing pass alone, from a caller's gain and a per-stream noise position.
//
// Layout.  Thread l owns the partial sum p[l] of SPEC §1.10, so a wave reads 256 contiguous bytes per step of the power
// pass.  The mixing pass reads the clip a second time: it is re-read from L2, not kept in LDS -- a row may have 2^24 samples,
// and the 64 KB of a one-second clip would leave two workgroups per CU where the re-read costs one more trip to a cache the
// clip has just been pulled through.  The stores are 16 bytes wide behind a head of up to three samples (store_row); the
// loads stay scalar, because a shift and a noise offset put them at any 4-byte address.
#include "mix_body.h"
#include "stream_state.h"

namespace {

using namespace lsm_mix;
using lsm_state::clamped_at;

struct MixArgs {
    const float *audio;                 // (rows, n)
    const float *noise;                 // (M, L)
    float *out;                         // (rows, n)
    const int32_t *noise_row, *noise_offset, *shift, *count, *pos_in;      // (rows) or null
    int32_t *pos_out;                   // (rows) or null
    const float *scale;                 // (rows) or null
    const double *ratio, *gain;         // (rows): batch / streamed
    double *gain_out, *power_out;       // (rows), (rows, 2), or null
    int n, M, L;
    const int32_t *clip_samples;        // (rows): the ragged batch form's lengths, n is then the rows' stride (last: the
};                                      // members above keep their offsets)

__global__ __launch_bounds__(THREADS) void mix_power_kernel(const float *x, int n, double *power_out)
{
    __shared__ double p[1][THREADS];
    const float *row = x + (size_t)blockIdx.x * n;
    double acc[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += THREADS) {
        const double u = (double)row[k];
        acc[0] = acc[0] + u * u;
    }
    power_tree<1>(p, acc);
    if (threadIdx.x == 0) power_out[blockIdx.x] = p[0][0];
}

// RAGGED (SPEC §1.16): a.n is the rows' stride and clip b has n = clamp(clip_samples[b], 0, a.n) samples -- everything that
// says how much of the row is the clip takes n, where the row lies takes the stride.  Samples of the row from n on are never
// read (shifted_sample clamps its index below n; with n = 0 neither the loop nor the store calls it) and are written as +0.0.
template <bool RAGGED>
__global__ __launch_bounds__(THREADS) void mix_kernel(const MixArgs a)
{
    __shared__ double p[2][THREADS];
    const int b = blockIdx.x, l = threadIdx.x, stride = a.n;
    const int n = RAGGED ? clamped_at(a.clip_samples, b, 0, stride, 0) : stride;
    const uint32_t L = (uint32_t)a.L;
    const float *row = a.audio + (size_t)b * stride;
    const int s = clamped_at(a.shift, b, -n, n, 0);
    const double sc = a.scale ? (double)a.scale[b] : 1.0;
    const float *nrow = a.noise + (size_t)clamped_at(a.noise_row, b, 0, a.M - 1, 0) * L;
    const uint32_t o = mod_nonneg(a.noise_offset ? a.noise_offset[b] : 0, a.L);
    const double q = a.ratio[b];

    // both powers in one pass; the noise index walks on by 256 mod L
    double acc[2] = {0.0, 0.0};
    uint32_t idx = noise_index(o, (uint32_t)l, L);
    const uint32_t step = (uint32_t)THREADS % L;
    for (int k = l; k < n; k += THREADS) {
        const double x = shifted_sample(row, n, s, sc, k);
        acc[0] = acc[0] + x * x;
        const double v = (double)nrow[idx];
        acc[1] = acc[1] + v * v;
        idx += step;
        if (idx >= L) idx -= L;
    }
    power_tree<2>(p, acc);
    const double Px = p[0][0], Pv = p[1][0];
    const bool noisy = q > 0.0 && Pv > 0.0;
    const double g = noisy ? sqrt((Px * q) / Pv) : 0.0;
    if (l == 0) {
        if (a.gain_out) a.gain_out[b] = g;
        if (a.power_out) {
            a.power_out[2 * (size_t)b] = Px;
            a.power_out[2 * (size_t)b + 1] = Pv;
        }
    }

    float *orow = a.out + (size_t)b * stride;
    store_row(orow, n,
              [&](const int i) {
                  const double v = noisy ? (double)nrow[noise_index(o, (uint32_t)i, L)] : 0.0;
                  return mixed_sample(shifted_sample(row, n, s, sc, i), noisy, g, v);
              },
              [&](const int i, float4 &y) {
                  uint32_t j = noisy ? noise_index(o, (uint32_t)i, L) : 0u;
                  float *ys = reinterpret_cast<float *>(&y);
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                      const double v = noisy ? (double)nrow[j] : 0.0;
                      ys[e] = mixed_sample(shifted_sample(row, n, s, sc, i + e), noisy, g, v);
                      j = noise_next(j, L);
                  }
              });
    // the fill has a head of its own: out + n has whatever alignment the stride and n leave it
    if constexpr (RAGGED) fill_row(orow + n, stride - n);
}

__global__ __launch_bounds__(THREADS) void mix_stream_kernel(const MixArgs a)
{
    const int b = blockIdx.x, H = a.n;
    const uint32_t L = (uint32_t)a.L;
    const int c = lsm_state::stream_count(a.count, b, H);
    const uint32_t pos = mod_nonneg(a.pos_in ? a.pos_in[b] : 0, a.L);
    __syncthreads();                    // pos_out may be pos_in: every thread has read the position before thread 0 writes it
    if (threadIdx.x == 0 && a.pos_out) a.pos_out[b] = (int32_t)noise_index(pos, (uint32_t)c, L);
    const float *row = a.audio + (size_t)b * H;             // out may be audio: a thread reads the samples it then writes
    const double sc = a.scale ? (double)a.scale[b] : 1.0;
    const double g = a.gain[b];
    const bool noisy = !(g == 0.0);
    const float *nrow = a.noise + (size_t)clamped_at(a.noise_row, b, 0, a.M - 1, 0) * L;

    store_row(a.out + (size_t)b * H, c,
              [&](const int i) {
                  const double v = noisy ? (double)nrow[noise_index(pos, (uint32_t)i, L)] : 0.0;
                  return mixed_sample(sc * (double)row[i], noisy, g, v);
              },
              [&](const int i, float4 &y) {
                  uint32_t j = noisy ? noise_index(pos, (uint32_t)i, L) : 0u;
                  float x[4];
#pragma unroll
                  for (int e = 0; e < 4; ++e) x[e] = row[i + e];
                  float *ys = reinterpret_cast<float *>(&y);
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                      const double v = noisy ? (double)nrow[j] : 0.0;
                      ys[e] = mixed_sample(sc * (double)x[e], noisy, g, v);
                      j = noise_next(j, L);
                  }
              });
}

// what the three entry points ask of a row length and a noise bank's shape
int check_shape(const char *what, int n, int n_rows)
{
    LSM_REQUIRE(n >= 1 && n <= MAX_SAMPLES, "%s=%d outside [1, %d]", what, n, MAX_SAMPLES);
    LSM_REQUIRE(n_rows >= 0, "a negative number of rows (%d)", n_rows);
    return LSM_OK;
}

int check_bank(int n_noise_rows, int noise_len)
{
    LSM_REQUIRE(noise_len >= 1, "noise_len=%d must be >= 1", noise_len);
    LSM_REQUIRE(n_noise_rows >= 1, "n_noise_rows=%d must be >= 1", n_noise_rows);
    return LSM_OK;
}

}  // namespace

LSM_API int lsm_mix_power_f32(const float *x, int n_rows, int n_samples, double *power_out, void *stream)
{
    const int rc = check_shape("n_samples", n_samples, n_rows);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE_ALIGNED(x, 4);
    LSM_REQUIRE_ALIGNED(power_out, 8);
    if (n_rows == 0) return LSM_OK;
    LSM_REQUIRE(x && power_out, "mix power: null buffer");
    hipLaunchKernelGGL(mix_power_kernel, dim3(n_rows), dim3(THREADS), 0, (hipStream_t)stream, x, n_samples, power_out);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

// The batch form's two entry points: lsm_mix_f32's refusals in their order, then the ragged form's own
static int mix_batch(bool ragged, const float *audio, int n_clips, int n_samples, const int32_t *clip_samples, const float *noise,
                     int n_noise_rows, int noise_len, const int32_t *noise_row, const int32_t *noise_offset,
                     const int32_t *shift, const float *scale, const double *ratio, float *out, double *gain_out,
                     double *power_out, void *stream)
{
    int rc = check_shape("n_samples", n_samples, n_clips);
    if (rc == LSM_OK) rc = check_bank(n_noise_rows, noise_len);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE_ALIGNED(noise, 4);
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE_ALIGNED(noise_row, 4);
    LSM_REQUIRE_ALIGNED(noise_offset, 4);
    LSM_REQUIRE_ALIGNED(shift, 4);
    LSM_REQUIRE_ALIGNED(scale, 4);
    LSM_REQUIRE_ALIGNED(ratio, 8);
    LSM_REQUIRE_ALIGNED(gain_out, 8);
    LSM_REQUIRE_ALIGNED(power_out, 8);
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(audio && noise && ratio && out, "mix: null buffer (audio, noise, ratio and out are required)");
    LSM_REQUIRE(out != audio, "out must not be audio: a shift reads across what it would write");
    if (ragged) {
        LSM_REQUIRE(clip_samples != nullptr, "mix ragged: null clip_samples");
        LSM_REQUIRE_ALIGNED(clip_samples, 4);
    }
    MixArgs a{};
    a.audio = audio; a.noise = noise; a.out = out;
    a.noise_row = noise_row; a.noise_offset = noise_offset; a.shift = shift; a.scale = scale; a.ratio = ratio;
    a.gain_out = gain_out; a.power_out = power_out; a.clip_samples = clip_samples;
    a.n = n_samples; a.M = n_noise_rows; a.L = noise_len;
    hipLaunchKernelGGL(ragged ? mix_kernel<true> : mix_kernel<false>, dim3(n_clips), dim3(THREADS), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

LSM_API int lsm_mix_f32(const float *audio, int n_clips, int n_samples, const float *noise, int n_noise_rows, int noise_len,
                        const int32_t *noise_row, const int32_t *noise_offset, const int32_t *shift, const float *scale,
                        const double *ratio, float *out, double *gain_out, double *power_out, void *stream)
{
    return mix_batch(false, audio, n_clips, n_samples, nullptr, noise, n_noise_rows, noise_len, noise_row, noise_offset, shift,
                     scale, ratio, out, gain_out, power_out, stream);
}

// include/lsm_hip_ragged_augment.h (SPEC.md §1.16): lsm_mix_f32 on rows of n_samples whose clips have clip_samples[b] samples
LSM_API int lsm_mix_ragged_f32(const float *audio, int n_clips, int n_samples, const int32_t *clip_samples, const float *noise,
                               int n_noise_rows, int noise_len, const int32_t *noise_row, const int32_t *noise_offset,
                               const int32_t *shift, const float *scale, const double *ratio, float *out, double *gain_out,
                               double *power_out, void *stream)
{
    return mix_batch(true, audio, n_clips, n_samples, clip_samples, noise, n_noise_rows, noise_len, noise_row, noise_offset,
                     shift, scale, ratio, out, gain_out, power_out, stream);
}

LSM_API int lsm_mix_stream_f32(const float *audio, int n_streams, int n_cols, const float *noise, int n_noise_rows,
                               int noise_len, const int32_t *count, const double *gain, const float *scale,
                               const int32_t *noise_row, const int32_t *pos_in, int32_t *pos_out, float *out, void *stream)
{
    int rc = check_shape("n_cols", n_cols, n_streams);
    if (rc == LSM_OK) rc = check_bank(n_noise_rows, noise_len);
    if (rc != LSM_OK) return rc;
    LSM_REQUIRE_ALIGNED(audio, 4);
    LSM_REQUIRE_ALIGNED(noise, 4);
    LSM_REQUIRE_ALIGNED(out, 4);
    LSM_REQUIRE_ALIGNED(count, 4);
    LSM_REQUIRE_ALIGNED(gain, 8);
    LSM_REQUIRE_ALIGNED(scale, 4);
    LSM_REQUIRE_ALIGNED(noise_row, 4);
    LSM_REQUIRE_ALIGNED(pos_in, 4);
    LSM_REQUIRE_ALIGNED(pos_out, 4);
    if (n_streams == 0) return LSM_OK;
    LSM_REQUIRE(audio && noise && gain && out, "mix stream: null buffer (audio, noise, gain and out are required)");
    MixArgs a{};
    a.audio = audio; a.noise = noise; a.out = out;
    a.count = count; a.gain = gain; a.scale = scale; a.noise_row = noise_row; a.pos_in = pos_in; a.pos_out = pos_out;
    a.n = n_cols; a.M = n_noise_rows; a.L = noise_len;
    hipLaunchKernelGGL(mix_stream_kernel, dim3(n_streams), dim3(THREADS), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
