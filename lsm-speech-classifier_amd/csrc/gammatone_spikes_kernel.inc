// gammatone_spikes_kernel.inc -- the text of the fused gammatone kernel, included once per form: the includer defines the
// kernel's name (LSM_FUSED_KERNEL), its parameters (LSM_FUSED_PARAMS) and MASK (LSM_FUSED_MASK) -- gammatone_spikes_body.h
// for gammatone_spikes_kernel(const FusedArgs a), mask.hip for gammatone_spikes_masked_kernel(a, const lsm_fe::MaskArgs m) --
// and RAGGED (LSM_FUSED_RAGGED): ragged_frontend.hip for gammatone_spikes_ragged_kernel(a, const lsm_fe::RaggedArgs rg), and
// ragged_masked_frontend.hip for gammatone_spikes_ragged_masked_kernel(a, rg, m) with both on (SPEC.md 1.16).
// The function's qualifiers are the includer's too (LSM_FUSED_QUALIFIERS: for these three `__global__
// __launch_bounds__(GT_MAX_WPB * 64)`), and so is what follows the staged rows, a file the includer names
// (LSM_FUSED_TAIL_INC): the three write the uint8 raster (gammatone_spikes_raster_out.inc); step_fused.hip hands the staged
// bits to the reservoir's time loop in the same workgroup instead (step_fused_tail.inc) and writes no raster.
// One text, three kernels -- and not one device function called by three kernels: behind a call, even a forced-inline one, the
// compiler allocated and scheduled 32 of the unmasked kernel's 34 forms differently (profiles/spec_mask.txt), and those
// forms are measured code.
//
// SHB0: every channel has the same first-section gain b0 = A0/B0 (the host verified it, coef_flags bit 2: this filter
// design has A0 = 1/fs and B0 = 1 everywhere), so the product b0*x of a sample is formed once per lane and feeds both
// chains: 70 instead of 71 instructions per sample and lane.
//
// MASK (SPEC.md 1.13): `m` holds the batch's frequency and time mask words; a masked value becomes +0.0 in the epilogue,
// where the zero bin's does.  A lane is a channel there, so its row bit is loaded once; the bin loop is uniform, so a
// group's time bits are one scalar word.  With MASK = false `m` is a dead local and the code is the unmasked kernel's.
//
// RAGGED (SPEC.md 1.14, LSM_FUSED_RAGGED, ragged_frontend.hip): clip b has its own number of time bins, rg.clip_bins[b],
// clamped here into 0 or 3..time_bins.  Everything that says how much of the clip there is -- the samples filtered (n_end),
// its columns `nc`, its bins `Tb` and with them zf, jz and the row's bit count -- comes from that count, a wave-uniform scalar
// loaded once; everything that says where the clip lies -- the audio row, the scratch, the LDS stage and the raster row --
// keeps the launch's strides a.ncols and a.time_bins.  A clip of 0 bins filters nothing and encodes nothing, reaches every
// barrier and writes zero rows.  With RAGGED = false `nc` is a.ncols, `Tb` is a.time_bins and the code is the twin's.
template <int NW, bool FAST, int NCH, bool SHB0 = false, bool PAIR = false>
LSM_FUSED_QUALIFIERS void LSM_FUSED_KERNEL(LSM_FUSED_PARAMS)
{
    LSM_FUSED_MASK                                      // constexpr bool MASK, and `m` where it is no parameter
    LSM_FUSED_RAGGED                                    // constexpr bool RAGGED (`rg` is a parameter where it is true)
    static_assert(!PAIR || NCH == 1, "the lane pair carries one chain per lane pair");
    constexpr int CPW = PAIR ? 32 : 64;                                   // channels of a chain group (of a wave)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *xch = reinterpret_cast<double *>(smem);                       // 2 * GT_MAX_WPB doubles
    uint32_t *stage_all = reinterpret_cast<uint32_t *>(smem + 2 * GT_MAX_WPB * sizeof(double));
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    const int groups = a.groups;                                          // waves per clip
    const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb)) + wave;
    const int b_raw = wid / groups;
    const bool valid = b_raw < a.n_clips;
    const int b = valid ? b_raw : a.n_clips - 1;
    const int g = wid - b_raw * groups;
    const int F = a.n_filters, nwin = a.nwin, hop = a.hop, ncols = a.ncols, n_samples = a.n_samples;
    // RAGGED: the clip's bins and columns (0, or 3..time_bins bins with at least one column: whatever the array holds)
    int tb_clip = 0, nc_clip = 0;
    if constexpr (RAGGED) {
        const int t = min(max(__builtin_amdgcn_readfirstlane(rg.bins[b]), 0), a.time_bins);
        nc_clip = t - (a.time_bins - ncols);
        tb_clip = (t >= 3 && nc_clip >= 1) ? t : 0;
        if (rg.steps_out != nullptr && valid && g == 0 && lane == 0) rg.steps_out[b] = tb_clip * a.n_thr;
    }
    const int nc = RAGGED ? nc_clip : ncols;                              // columns of this clip
    const bool run = valid && (!RAGGED || tb_clip > 0);                   // this wave filters and encodes
    const int NG = groups * NCH;                                          // chain groups per clip (padded)
    const int cl = PAIR ? (lane & 31) : lane;                             // this lane's channel within its group
    const bool owner = !PAIR || lane >= 32;                               // the lane whose output is the channel's

    bool live[NCH];
    double b0[NCH], b11[NCH], b12[NCH], b13[NCH], b14[NCH], b2[NCH], a1[NCH], a2[NCH], gain[NCH], rgain[NCH];
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const int chl = (g * NCH + q) * CPW + cl;
        live[q] = chl < F;
        const lsm_gt::Sections s = lsm_gt::load_sections(a.coefs, live[q] ? chl : F - 1);
        b0[q] = s.b0; b2[q] = s.b2; b11[q] = s.b1[0]; b12[q] = s.b1[1]; b13[q] = s.b1[2]; b14[q] = s.b1[3];
        a1[q] = s.a1; a2[q] = s.a2; gain[q] = s.gain; rgain[q] = s.rgain;
    }
    const float *__restrict__ x = a.audio + (size_t)b * n_samples;        // wave-uniform

    double z01[NCH], z11[NCH], z02[NCH], z12[NCH], z03[NCH], z13[NCH], z04[NCH], z14[NCH];
    double win[NCH][NW];
    double mx[NCH], mn[NCH];
    bool nan_seen = false;                              // a NaN among my dB values (the comparisons below skip it)
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        z01[q] = z11[q] = z02[q] = z12[q] = z03[q] = z13[q] = z04[q] = z14[q] = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) win[q][w] = 0.0;
        mx[q] = -INFINITY; mn[q] = INFINITY;
    }

    // PAIR: this half's section coefficients (head: sections 1-2, tail: 3-4) and its last section-2 output.  With SHB0
    // the one b0 of the table is channel 0's, read once per wave (scalar registers).
    const double bp1 = owner ? b13[0] : b11[0], bp2 = owner ? b14[0] : b12[0];
    const double b0p = SHB0 ? uniform_f64(a.coefs[0] / a.coefs[6]) : b0[0];
    double u2 = 0.0;
    auto pfilt = [&](double x0) __attribute__((always_inline)) -> double {
        const double u = pair_up(x0, u2);               // head: the next sample; tail: the head's y2 of its sample
        const double y1 = lsm_gt::section<FAST>(z01[0], b0p, u, z11[0], bp1, a1[0], a2[0], b2[0]);
        const double y2 = lsm_gt::section<FAST>(z02[0], b0p, y1, z12[0], bp2, a1[0], a2[0], b2[0]);
        u2 = y2;
        double o;
        lsm_gt::quot<FAST>(o, y2, gain[0], rgain[0]);
        return o * o;
    };
    // lsm_gt::section four times, written out: called through section() this cascade compiles to other code, whatever the
    // form of the call (profiles/frontend_shared_filter.txt); the split kernel's cascade and pfilt do call it
    auto filt = [&](int q, double x0, double bx) __attribute__((always_inline)) -> double {
        const double y1 = z01[q] + (SHB0 ? bx : b0[q] * x0);
        z01[q] = (z11[q] + x0 * b11[q]) - y1 * a1[q];
        z11[q] = FAST ? -(y1 * a2[q]) : x0 * b2[q] - y1 * a2[q];
        const double y2 = z02[q] + b0[q] * y1;
        z02[q] = (z12[q] + y1 * b12[q]) - y2 * a1[q];
        z12[q] = FAST ? -(y2 * a2[q]) : y1 * b2[q] - y2 * a2[q];
        const double y3 = z03[q] + b0[q] * y2;
        z03[q] = (z13[q] + y2 * b13[q]) - y3 * a1[q];
        z13[q] = FAST ? -(y3 * a2[q]) : y2 * b2[q] - y3 * a2[q];
        const double y4 = z04[q] + b0[q] * y3;
        z04[q] = (z14[q] + y3 * b14[q]) - y4 * a1[q];
        z14[q] = FAST ? -(y4 * a2[q]) : y3 * b2[q] - y4 * a2[q];
        double o;
        lsm_gt::quot<FAST>(o, y4, gain[q], rgain[q]);
        return o * o;
    };
#define LSM_RUNF(n_to, NACT)                                                        \
    {                                                                               \
        if (n + 8 <= (n_to)) {                                                      \
            float xs[8], nx[8];                                                     \
            _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = x[n + u];         \
            for (; n + 8 <= (n_to); n += 8) {                                       \
                const float *pn = x + min(n + 8, n_samples - 8);                    \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) nx[u] = pn[u];        \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) {                     \
                    const double x0 = (double)xs[u];                                \
                    const double bx = b0[0] * x0;                                   \
                    _Pragma("unroll") for (int q = 0; q < NCH; ++q) {               \
                        const double e = filt(q, x0, bx);                           \
                        _Pragma("unroll") for (int w = 0; w < (NACT); ++w) win[q][w] += e; \
                    }                                                               \
                }                                                                   \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = nx[u];        \
            }                                                                       \
        }                                                                           \
        for (; n < (n_to); ++n) {                                                   \
            const double x0 = (double)x[n];                                         \
            const double bx = b0[0] * x0;                                           \
            _Pragma("unroll") for (int q = 0; q < NCH; ++q) {                       \
                const double e = filt(q, x0, bx);                                   \
                _Pragma("unroll") for (int w = 0; w < (NACT); ++w) win[q][w] += e;  \
            }                                                                       \
        }                                                                           \
    }

    // PAIR: the tail processes sample n while the head takes x[n + 1] (clamped inside the clip: the head's output of
    // the sample past the last one is never used); full chunks stop where x[n + 8] would leave the clip
#define LSM_RUNP(n_to, NACT)                                                        \
    {                                                                               \
        const int n_blk = min((n_to), n_samples - 1);                               \
        if (n + 8 <= n_blk) {                                                       \
            float xs[8], nx[8];                                                     \
            _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = x[n + 1 + u];     \
            for (; n + 8 <= n_blk; n += 8) {                                        \
                const float *pn = x + 1 + min(n + 8, n_samples - 9);                \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) nx[u] = pn[u];        \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) {                     \
                    const double e = pfilt((double)xs[u]);                          \
                    _Pragma("unroll") for (int w = 0; w < (NACT); ++w) win[0][w] += e; \
                }                                                                   \
                _Pragma("unroll") for (int u = 0; u < 8; ++u) xs[u] = nx[u];        \
            }                                                                       \
        }                                                                           \
        for (; n < (n_to); ++n) {                                                   \
            const double e = pfilt((double)x[min(n + 1, n_samples - 1)]);           \
            _Pragma("unroll") for (int w = 0; w < (NACT); ++w) win[0][w] += e;      \
        }                                                                           \
    }

    // scratch of this wave: column c, chain q at wsw[(c * NG + q) * CPW]
    double *wsw = a.ws + ((size_t)b * ncols * NG + (size_t)g * NCH) * CPW + cl;
    // The filter loop is the throughput-critical stream of the pipeline: a wave alone on its SIMD issues a float64
    // operation every 5.0 cycles, which leaves the reservoir waves sharing the SIMD one issue slot in five -- about
    // what they need.  At the default priority the reservoir kernel's raised-priority phases (lif_dense.h) take
    // slots from it instead, so it runs at priority 0 (priorities 0-3: profiles/r03_priorities_and_stream_counts.txt).
    // The untaken branches below stay: without them the compiler allocates the filter loop differently (fewer vector
    // registers, e.g. 238 -> 168 in one layout) and the pipeline ran 4 % slower at cfg4, 3 % at cfg2.
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1);
    else if (a.prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (a.prio == 3) __builtin_amdgcn_s_setprio(3);
    if (run) {
        const int pos = nwin - (NW - 1) * hop;
        const int n_end = (nc - 1) * hop + nwin;
        const double dn = (double)nwin;
        if (PAIR) {
            // the head's sample 0; the tail ran on a zero input, and its state restarts at +0 (all it held were
            // signed zeros)
            (void)pfilt((double)x[0]);
            if (owner) z01[0] = z11[0] = z02[0] = z12[0] = 0.0;
        }
        int n = 0;
        for (int h = 0; n < n_end; ++h) {
            const int base = h * hop;
            const int mid = min(base + pos, n_end);
            if (PAIR) LSM_RUNP(mid, NW) else LSM_RUNF(mid, NW)
            const int c = h - (NW - 1);
            if (n == base + pos && c >= 0 && c < nc) {
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    const double y = sqrt(win[q][NW - 1] / dn);
                    const double v = 20 * log10(y + 1e-9);
                    if (owner) wsw[((size_t)c * NG + q) * CPW] = v;
                    if (live[q] && owner) {
                        mx[q] = v > mx[q] ? v : mx[q];
                        mn[q] = v < mn[q] ? v : mn[q];
                        nan_seen |= v != v;
                    }
                }
            }
            const int stop = min(base + hop, n_end);
            if (PAIR) LSM_RUNP(stop, NW - 1) else LSM_RUNF(stop, NW - 1)
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
#pragma unroll
                for (int w = NW - 1; w > 0; --w) win[q][w] = win[q][w - 1];
                win[q][0] = 0.0;
            }
        }
    }
#undef LSM_RUNF
#undef LSM_RUNP

    __builtin_amdgcn_s_setprio(0);
    // ---- the clip's max / min -----------------------------------------------------------------
    double hi = mx[0], lo = mn[0];
#pragma unroll
    for (int q = 1; q < NCH; ++q) {
        hi = mx[q] > hi ? mx[q] : hi;
        lo = mn[q] < lo ? mn[q] : lo;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double oh = __shfl_xor(hi, off), ol = __shfl_xor(lo, off);
        hi = oh > hi ? oh : hi;
        lo = ol < lo ? ol : lo;
    }
    // spec_db.max() / .min() / np.maximum (create_dataset.py:59-63) propagate NaN: one NaN among the clip's dB values makes
    // max, floor and min NaN -- every normalised value NaN, the raster all zeros (tests/golden/postfilter_nonfinite.npz)
    if (__builtin_amdgcn_ballot_w64(nan_seen) != 0ull) hi = lo = (double)NAN;
    if (groups > 1) {                                   // uniform over the launch
        if (lane == 0) { xch[2 * wave] = hi; xch[2 * wave + 1] = lo; }
        __syncthreads();
        const int w0 = wave - g;                        // first wave of this clip in the workgroup
        hi = xch[2 * w0]; lo = xch[2 * w0 + 1];
        bool nan_any = hi != hi;
        for (int i = 1; i < groups; ++i) {
            const double oh = xch[2 * (w0 + i)], ol = xch[2 * (w0 + i) + 1];
            hi = oh > hi ? oh : hi;
            lo = ol < lo ? ol : lo;
            nan_any = nan_any || oh != oh;
        }
        if (nan_any) hi = lo = (double)NAN;
    }
    // create_dataset.py:60 floors at max-80 before the min is taken: min' = max(min, max-80)
    const double fl = hi - 80.0;
    lo = lo > fl ? lo : fl;                             // (NaN: fl)
    const bool flat = (hi - lo) < 1e-8;
    const double den = (hi - lo) + 1e-8;
    const int Tb = RAGGED ? tb_clip : a.time_bins, n_thr = a.n_thr;
    const int row_bits = Tb * n_thr;
    const double zf = (double)(nc - 1) / (double)(Tb - 1);
    // the bin whose coordinate lies outside the input and is +0.0 (spikes_body.h, SPEC.md 1.2): the last one or none (-1)
    const int jz = (nc != Tb && (double)(Tb - 1) * zf > (double)(nc - 1)) ? Tb - 1 : -1;
    // (x - lo) / den for 2 x 100 values per channel: den is wave-uniform, so its correctly rounded reciprocal is
    // computed once and every quotient is q = x*r, q' = fma(fma(-q, den, x), r, q) -- Markstein's sequence, the
    // correctly rounded quotient (= the IEEE division spec_to_spikes_kernel performs) unless den's significand is
    // all ones or den leaves the normal range (broken audio: inf/NaN); those clips take the true division.  The
    // numerators need no check of their own: every x is clamped into [lo, hi] (NaN and -inf become the floor), so
    // 0 <= x - lo <= hi - lo < den, a difference of two dB values: zero or far above the denormal range.
    const double rden = 1.0 / den;
    const unsigned long long den_bits = (unsigned long long)__double_as_longlong(den);
    const bool fastdiv = den > 1e-200 && den < 1e200 &&
                         (den_bits & 0x000FFFFFFFFFFFFFull) != 0x000FFFFFFFFFFFFFull;
    // Per group of JPW bins (no dependency between the bins of a group, the loads of the whole group in flight together):
    // per bin j and threshold t the two comparisons the latch needs, S = val > on[t] in bit t and R = val < off[t] in bit
    // FBH + t of the bin's field; then -- round 4: in the same iteration, from registers -- the set/reset latches of all
    // thresholds at once, A = (S & ~A) | (A & ~R), and the raster bits appended to a 64-bit accumulator that is stored to
    // the lane's LDS row a word at a time.  The first version staged the FIELDS of all bins in LDS (pass A) and ran the
    // latch as a second pass over them (pass B): 100 bytes of stage per channel instead of 50, i.e. 51 KB instead of
    // 27 KB per 4-wave workgroup -- which mattered once a ring-kernel clip pair (2 x 64 KB) had to fit beside it on a CU.
    // The only state carried from group to group is the latch (4-8 bits per chain) and the bit accumulator.
    const int FBH = n_thr <= 4 ? 4 : 8;                 // bits per half field
    const int JPW = 16 / FBH;                           // bins per 32-bit word (4 or 2)
    const int NG4 = (Tb + JPW - 1) / JPW;               // groups of JPW bins
    const int RW = ((RAGGED ? a.time_bins * n_thr : row_bits) + 31) >> 5;   // words per staged raster row (the launch's stride)
    uint32_t *stage = stage_all + (size_t)wave * (NCH * CPW) * RW;
    const size_t cs = (size_t)NG * CPW;                 // doubles between two columns of the scratch
    // MASK: this lane's row bits (a channel past the last filter has none: its word may not exist) and the clip's time words
    bool chm[NCH];
    const uint32_t *tmc = nullptr;
    if constexpr (MASK) {
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            const int chl = (g * NCH + q) * CPW + cl;
            chm[q] = m.freq != nullptr && live[q] &&
                     ((m.freq[(size_t)b * ((F + 31) >> 5) + (chl >> 5)] >> (chl & 31)) & 1u) != 0u;
        }
        // wave-uniform; the mask rows keep the launch's stride (RAGGED: a group's word index stays below ceil(Tb / 32), and
        // the bits at or behind Tb belong to bins that the latch loop skips)
        tmc = m.time ? m.time + (size_t)b * (((RAGGED ? a.time_bins : Tb) + 31) >> 5) : nullptr;
    }
    // straight-line variants (fast division or not, <= 4 thresholds or not, resize or not): one uniform choice
    // per wave instead of uniform branches inside the loop, which would keep the compiler from batching the loads
    auto pass_a = [&](auto fast_c, auto nt_c, auto zoom_c) __attribute__((always_inline)) {
        constexpr bool FD = decltype(fast_c)::value;
        constexpr int NT = decltype(nt_c)::value;       // thresholds compared (tables are padded with +inf / -inf)
        constexpr bool ZOOM = decltype(zoom_c)::value;
        constexpr int H = NT <= 4 ? 4 : 8, G = 16 / H;  // = FBH, JPW
        auto norm1 = [&](double v) __attribute__((always_inline)) -> double {
            v = v > fl ? v : fl;
            double q;
            lsm_gt::quot<FD>(q, v - lo, den, rden);
            return q;
        };
        uint32_t act[NCH];
        unsigned long long acc[NCH];
#pragma unroll
        for (int q = 0; q < NCH; ++q) { act[q] = 0u; acc[q] = 0ull; }
        int fill = 0, wout = 0;                         // the same for every chain of the lane
        const uint32_t tmask_a = (1u << n_thr) - 1u;
        // one group of G bins; LAST: the group that holds the last bin, the only one the zero rule (jz) can touch -- it is
        // peeled off the loop, whose groups then carry no test for it
        auto group = [&](const int jw, auto last_c) __attribute__((always_inline)) {
            constexpr bool LAST = decltype(last_c)::value;
            double x0[G][NCH], x1[G][NCH], w0[G], w1[G];
            bool two[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int j = min(jw * G + u, Tb - 1);
                // scipy.ndimage.zoom(order=1): double coordinate and weights, w1 = 1 - w0
                const double cc = (double)j * zf;
                const double fc = floor(cc);
                const int f = ZOOM ? (int)fc : j;
                w0[u] = 1.0 - (cc - fc);
                w1[u] = 1.0 - w0[u];
                two[u] = f + 1 <= nc - 1;
                const int f1 = two[u] ? f + 1 : f;
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    const double *col = wsw + (size_t)q * CPW;
                    x0[u][q] = col[(size_t)f * cs];
                    if (ZOOM) x1[u][q] = col[(size_t)f1 * cs];
                }
            }
            uint32_t fw[NCH];
#pragma unroll
            for (int q = 0; q < NCH; ++q) fw[q] = 0u;
            // MASK: the group's G bins start at a multiple of G, which divides 32: their time bits lie in one word
            uint32_t tw = 0u;
            if constexpr (MASK) tw = tmc ? tmc[(jw * G) >> 5] >> ((jw * G) & 31) : 0u;
#pragma unroll
            for (int u = 0; u < G; ++u) {
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    const double n0 = norm1(x0[u][q]);
                    double val = n0;
                    if (ZOOM) {
                        const double n1 = norm1(x1[u][q]);
                        const double acc = n0 * w0[u];
                        // the last column has no right neighbour (two == false: cc >= ncols-1).  Either cc == ncols-1, then
                        // its weight w1 is 0 and, on the fast path, n1 is finite and acc >= +0, so acc + n1*0 == acc bit
                        // for bit: no branch needed; or cc > ncols-1, then the bin is jz and the value is replaced below
                        val = (FD || two[u]) ? acc + n1 * w1[u] : acc;
                    }
                    val = (flat || (LAST && ZOOM && jw * G + u == jz)) ? 0.0 : val;     // (a scalar condition: one select)
                    if constexpr (MASK) val = (((tw >> u) & 1u) != 0u || chm[q]) ? 0.0 : val;
                    uint32_t field = 0u;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        field |= (val > a.on[t] ? 1u : 0u) << t;
                        field |= (val < a.off[t] ? 1u : 0u) << (H + t);
                    }
                    fw[q] |= field << (u * 2 * H);
                }
            }
            // the latches of this group's bins, in bin order (bins past the last one repeat it and are skipped)
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (jw * G + u < Tb) {                  // wave-uniform
#pragma unroll
                    for (int q = 0; q < NCH; ++q) {
                        const uint32_t field = fw[q] >> (u * 2 * H);
                        const uint32_t S = field & tmask_a, R = (field >> H) & tmask_a;
                        act[q] = (S & ~act[q]) | (act[q] & ~R);     // create_dataset.py:90-95 (both from the old latch)
                        acc[q] |= (unsigned long long)act[q] << fill;
                    }
                    fill += n_thr;
                    if (fill >= 32) {
#pragma unroll
                        for (int q = 0; q < NCH; ++q) {
                            if (owner) stage[(q * CPW + cl) * RW + wout] = (uint32_t)acc[q];
                            acc[q] >>= 32;
                        }
                        ++wout;
                        fill -= 32;
                    }
                }
            }
        };
#pragma unroll 1
        for (int jw = 0; jw < NG4 - 1; ++jw) group(jw, std::false_type{});
        group(NG4 - 1, std::true_type{});
        if (fill > 0) {
#pragma unroll
            for (int q = 0; q < NCH; ++q) if (owner) stage[(q * CPW + cl) * RW + wout] = (uint32_t)acc[q];
        }
    };
    if (!RAGGED || Tb > 0) {                            // (a clip of 0 bins has no bin to encode; wave-uniform, no barrier inside)
        using T = std::true_type;
        using F = std::false_type;
        using N4 = std::integral_constant<int, 4>;
        using N8 = std::integral_constant<int, MAX_THR>;
        const bool zoom = nc != Tb;
        if (n_thr <= 4) {
            if (fastdiv) { if (zoom) pass_a(T{}, N4{}, T{}); else pass_a(T{}, N4{}, F{}); }
            else         { if (zoom) pass_a(F{}, N4{}, T{}); else pass_a(F{}, N4{}, F{}); }
        } else {
            if (fastdiv) { if (zoom) pass_a(T{}, N8{}, T{}); else pass_a(T{}, N8{}, F{}); }
            else         { if (zoom) pass_a(F{}, N8{}, T{}); else pass_a(F{}, N8{}, F{}); }
        }
    }
    __syncthreads();                                    // the wave's own staged rows (and a uniform barrier count)
#include LSM_FUSED_TAIL_INC
}
