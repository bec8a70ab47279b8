// mel_body.h -- one STFT frame -> mel power values, as a device function of ONE wave (SPEC.md §1.5): the transform of the
// batch kernels (mel.hip) and of the streamed front end (mel_stream.hip), which differ only in where a frame's samples
// come from and where its power values go.
#pragma once
#include "lsm_common.h"

namespace lsm_mel {

constexpr int NFFT = 2048;
constexpr int N2 = NFFT / 2;                 // the real frame is transformed as N2 complex points
constexpr int NBINS = NFFT / 2 + 1;
constexpr int ZPAD = N2 + N2 / 16;           // a wave's point buffer: one pad element after every 16 (see zpad)

// W_2048^m for any m in [0, 2048) from the table of the first 1024 powers (W^(m+1024) = -W^m)
__device__ __forceinline__ double2 tw2048(const double2 *__restrict__ t, int m)
{
    const double2 w = t[m & (N2 - 1)];
    return (m & N2) ? make_double2(-w.x, -w.y) : w;
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// four-point transform in place: a_c <- sum_q a_q W_4^(q c), W_4 = -i
__device__ __forceinline__ void bfly4(double2 &a0, double2 &a1, double2 &a2, double2 &a3)
{
    const double2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3);
    const double2 t3 = make_double2(a1.y - a3.y, -(a1.x - a3.x));          // -i (a1 - a3)
    a0 = cadd(t0, t2); a1 = cadd(t1, t3); a2 = csub(t0, t2); a3 = csub(t1, t3);
}
// sixteen-point transform in registers, as 4 x 4: input q = 4a + b sits in u[q]; output r = c + 4d ends in u[d + 4c]
__device__ __forceinline__ void bfly16(double2 (&u)[16])
{
    constexpr double C1 = 0.92387953251128673848, S1 = 0.38268343236508978178, H = 0.70710678118654752440;
#pragma unroll
    for (int b = 0; b < 4; ++b) bfly4(u[b], u[b + 4], u[b + 8], u[b + 12]);     // u[b + 4c] = sum_a u[4a + b] W_4^(a c)
    // times W_16^(b c)
    u[1 + 4] = cmul(u[1 + 4], make_double2(C1, -S1));
    u[1 + 8] = cmul(u[1 + 8], make_double2(H, -H));
    u[1 + 12] = cmul(u[1 + 12], make_double2(S1, -C1));
    u[2 + 4] = cmul(u[2 + 4], make_double2(H, -H));
    u[2 + 8] = make_double2(u[2 + 8].y, -u[2 + 8].x);                          // W_16^4 = -i
    u[2 + 12] = cmul(u[2 + 12], make_double2(-H, -H));
    u[3 + 4] = cmul(u[3 + 4], make_double2(S1, -C1));
    u[3 + 8] = cmul(u[3 + 8], make_double2(-H, -H));
    u[3 + 12] = cmul(u[3 + 12], make_double2(-C1, S1));
#pragma unroll
    for (int c = 0; c < 4; ++c) bfly4(u[4 * c], u[4 * c + 1], u[4 * c + 2], u[4 * c + 3]);
}
// LDS element of point e: a pad element after every sixteen points, so that the sixteen consecutive points a lane writes
// in the first pass (and the runs of sixteen of the second) start in different banks from lane to lane
__device__ __forceinline__ int zpad(int e) { return e + (e >> 4); }
// a wave's LDS accesses of one pass are seen by its other lanes in the next (LDS keeps a wave's order; this keeps the compiler's)
__device__ __forceinline__ void mel_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W_32^i = exp(-2 pi i / 32), i <= 16, as {cos, sin} of pi i / 16
__device__ constexpr double W32_COS[17] = {1.0, 0.98078528040323044913, 0.92387953251128673848, 0.83146961230254523708,
                                           0.70710678118654752440, 0.55557023301960222474, 0.38268343236508978178,
                                           0.19509032201612826785, 0.0, -0.19509032201612826785, -0.38268343236508978178,
                                           -0.55557023301960222474, -0.70710678118654752440, -0.83146961230254523708,
                                           -0.92387953251128673848, -0.98078528040323044913, -1.0};
__device__ constexpr double W32_SIN[17] = {0.0, 0.19509032201612826785, 0.38268343236508978178, 0.55557023301960222474,
                                           0.70710678118654752440, 0.83146961230254523708, 0.92387953251128673848,
                                           0.98078528040323044913, 1.0, 0.98078528040323044913, 0.92387953251128673848,
                                           0.83146961230254523708, 0.70710678118654752440, 0.55557023301960222474,
                                           0.38268343236508978178, 0.19509032201612826785, 0.0};

// The parameter tables of a transform (mel.py builds them): periodic Hann window (2048 float64), W_2048^k for k < 1024,
// the mel basis (n_mels, 1025) float32 and the half-open range [lo, hi) of every filter's non-zero bins.
struct Tables {
    const double *window;
    const double2 *twiddle;
    const float *basis;
    const int *lo, *hi;
    int n_mels;
};

// One wave = one frame.  `samples(p, v0, v1)` gives the frame's samples p and p + 1 (p even, < 2048) as float64, zero where the
// frame lies outside its signal; `sink(m, value)` takes the power of filter m, from ONE lane per filter.  The 2048 windowed
// real samples are packed as 1024 complex points
// z[n] = x[2n] + i x[2n+1]; lane l holds the points l + 64 s, s < 16, of every pass.  Stockham passes (natural order in and
// out) with strides p = 1 (radix 16, inputs straight from memory, no twiddles), p = 16 (radix 16) and p = 256 (radix 4, four
// butterflies per lane): out[j + r p] = sum_q W_R^(q r) W_(R p)^(q k) in[i + q N/R], k = i mod p, j = (i - k) R + k.  Then
// the 1025 bins of the real transform, X[k] = E[k] - i W^k O[k], E/O = (Z[k] +- conj Z[N2-k]) / 2.  All in float64.
// `z`: this wave's ZPAD points of LDS; the power values reuse its first NBINS floats.  (Twiddle products instead of table entries move the float64
// spectrum by a few 1e-16 relative: the table's own rounding.)
template <typename Samples, typename Sink>
__device__ __forceinline__ void mel_frame_wave(const Tables &a, double2 *z, const Samples &samples, const Sink &sink)
{
    float *pw = reinterpret_cast<float *>(z);
    const int n_mels = a.n_mels;
    const double *__restrict__ window = a.window;
    const double2 *__restrict__ twiddle = a.twiddle;
    const float *__restrict__ basis = a.basis;
    const int *__restrict__ lo = a.lo, *__restrict__ hi = a.hi;
    const int lane = threadIdx.x & 63;

    // Every twiddle factor of the frame is a product of EIGHT table entries fetched here, with the samples (one exposed memory
    // latency per frame), and of constants: W_2048^(8 q k) from the powers 1, 2, 4, 8 of W_256^k (second pass), W_2048^(2 q (l + 64 c))
    // = W_1024^(q l) W_16^(q c) (third pass), W_2048^(l + 64 i) = W_2048^l W_32^i (unpacking).
    const int k = lane & 15;
    const double2 wb1 = twiddle[8 * k], wb2 = twiddle[16 * k], wb4 = twiddle[32 * k], wb8 = twiddle[64 * k];
    const double2 wc1 = twiddle[2 * lane], wc2 = twiddle[4 * lane], wc3 = twiddle[6 * lane];
    const double2 wu = twiddle[lane];
    double2 u[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int n = lane + 64 * s;
        double v0, v1;
        samples(2 * n, v0, v1);
        const double2 wn = *reinterpret_cast<const double2 *>(window + 2 * n);
        u[s] = make_double2(wn.x * v0, wn.y * v1);
    }
    constexpr double C1 = 0.92387953251128673848, S1 = 0.38268343236508978178, H = 0.70710678118654752440;
    // p = 1: i = lane, k = 0, j = 16 lane
    bfly16(u);
#pragma unroll
    for (int s = 0; s < 16; ++s) z[zpad(16 * lane + (s >> 2) + 4 * (s & 3))] = u[s];
    mel_wave_fence();
    // p = 16: i = lane, k = lane mod 16, j = (lane - k) 16 + k; twiddles W_256^(q k) = W_2048^(8 q k)
#pragma unroll
    for (int s = 0; s < 16; ++s) u[s] = z[zpad(lane + 64 * s)];
    {
        const double2 w3 = cmul(wb2, wb1), w5 = cmul(wb4, wb1), w6 = cmul(wb4, wb2), w7 = cmul(wb4, w3);
        u[1] = cmul(u[1], wb1); u[2] = cmul(u[2], wb2); u[3] = cmul(u[3], w3); u[4] = cmul(u[4], wb4);
        u[5] = cmul(u[5], w5); u[6] = cmul(u[6], w6); u[7] = cmul(u[7], w7); u[8] = cmul(u[8], wb8);
        u[9] = cmul(u[9], cmul(wb8, wb1)); u[10] = cmul(u[10], cmul(wb8, wb2)); u[11] = cmul(u[11], cmul(wb8, w3));
        u[12] = cmul(u[12], cmul(wb8, wb4)); u[13] = cmul(u[13], cmul(wb8, w5)); u[14] = cmul(u[14], cmul(wb8, w6));
        u[15] = cmul(u[15], cmul(wb8, w7));
    }
    bfly16(u);
    mel_wave_fence();                       // every lane has read its points before any is overwritten
    const int j = (lane - k) * 16 + k;
#pragma unroll
    for (int s = 0; s < 16; ++s) z[zpad(j + 16 * ((s >> 2) + 4 * (s & 3)))] = u[s];
    mel_wave_fence();
    // p = 256, radix 4: butterflies i = lane + 64 c, k = i, j = i; twiddles W_1024^(q k) = W_1024^(q lane) W_16^(q c)
#pragma unroll
    for (int s = 0; s < 16; ++s) u[s] = z[zpad(lane + 64 * s)];
    mel_wave_fence();
    const double2 w16[10] = {make_double2(1.0, 0.0), make_double2(C1, -S1), make_double2(H, -H), make_double2(S1, -C1),
                             make_double2(0.0, -1.0), make_double2(0.0, 0.0), make_double2(-H, -H), make_double2(0.0, 0.0),
                             make_double2(0.0, 0.0), make_double2(-C1, S1)};        // W_16^m for m = q c
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int kk = lane + 64 * c;
        if (c == 0) {
            u[4] = cmul(u[4], wc1); u[8] = cmul(u[8], wc2); u[12] = cmul(u[12], wc3);
        } else {
            u[c + 4] = cmul(u[c + 4], cmul(wc1, w16[c]));
            u[c + 8] = cmul(u[c + 8], cmul(wc2, w16[2 * c]));
            u[c + 12] = cmul(u[c + 12], cmul(wc3, w16[3 * c]));
        }
        bfly4(u[c], u[c + 4], u[c + 8], u[c + 12]);
#pragma unroll
        for (int r = 0; r < 4; ++r) z[zpad(kk + 256 * r)] = u[c + 4 * r];
    }
    mel_wave_fence();
    // The 1025 power values go where the points were (`pw` aliases `z`): every lane forms its seventeen first, then they are stored.
    float pv[17];
#pragma unroll
    for (int i = 0; i <= 16; ++i) {
        const int f = lane + 64 * i;
        pv[i] = 0.0f;
        if (i < 16 || lane == 0) {
            const double2 zk = z[zpad(f & (N2 - 1))];
            const double2 zr = z[zpad((N2 - f) & (N2 - 1))];
            const double2 E = make_double2(0.5 * (zk.x + zr.x), 0.5 * (zk.y - zr.y));    // (Zk + conj Zr)/2
            const double2 O = make_double2(0.5 * (zk.x - zr.x), 0.5 * (zk.y + zr.y));    // (Zk - conj Zr)/2
            const double2 wf = i == 0 ? wu : cmul(wu, make_double2(W32_COS[i], -W32_SIN[i]));      // W_2048^f
            const double2 D = cmul(wf, O);
            const float re = (float)(E.x + D.y), im = (float)(E.y - D.x);               // complex64 storage
            const float mag = hypotf(re, im);                   // np.abs on complex64
            pv[i] = mag * mag;                                  // ** 2.0 in float32
        }
    }
    mel_wave_fence();                           // every lane has read its points
#pragma unroll
    for (int i = 0; i <= 16; ++i)
        if (i < 16 || lane == 0) pw[lane + 64 * i] = pv[i];
    mel_wave_fence();
    // mel projection: four lanes per filter, lane q takes bins lo+q, lo+q+4, ... (ascending), the four
    // partial sums are combined as (p0 + p1) + (p2 + p3)
    for (int m0 = 0; m0 < n_mels; m0 += 16) {
        const int m = m0 + (lane >> 2), q = lane & 3;
        float acc = 0.0f;
        if (m < n_mels) {
            const float *row = basis + (size_t)m * NBINS;
            const int h = hi[m];
            int f = lo[m] + q;
            for (; f + 28 < h; f += 32) {       // eight terms at a time, their loads together; the additions keep their order
                float r[8], pq[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { r[e] = row[f + 4 * e]; pq[e] = pw[f + 4 * e]; }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += r[e] * pq[e];
            }
            if (f + 12 < h) {
                const float r0 = row[f], r1 = row[f + 4], r2 = row[f + 8], r3 = row[f + 12];
                const float p0 = pw[f], p1 = pw[f + 4], p2 = pw[f + 8], p3 = pw[f + 12];
                acc += r0 * p0; acc += r1 * p1; acc += r2 * p2; acc += r3 * p3;
                f += 16;
            }
            for (; f < h; f += 4) acc += row[f] * pw[f];
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if (m < n_mels && q == 0) sink(m, acc);
    }
}

}  // namespace lsm_mel
