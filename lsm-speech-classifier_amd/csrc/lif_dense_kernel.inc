// lif_dense_kernel.inc -- the body of lif_dense_kernel (lif_dense.h), included between the braces of the kernel it belongs to:
// lif_dense_kernel<SL, WPC, INMODE, REFM, ST>(const DenseArgs a) in lif_dense.h, and the fused step kernel of step_fused.hip,
// where it follows the front end of the same clip in the same workgroup (one text, several kernels: see
// gammatone_spikes_kernel.inc on why the text is shared and not a device function).  The includer says
//   LSM_DENSE_LDS_DECL, LSM_DENSE_LDS   the declaration that makes the kernel's LDS image visible and the address it starts
//                        at (lif_dense.h: the dynamic LDS itself, `smem`);
//   LSM_DENSE_INPUT_BITS_INC   the file that fills the input bit rows bits[t * CW + q] once `icnt`, `wcnt` and `feat` are
//                        zeroed: lif_dense_pack_raster.inc zeroes `bits` and packs the clip's uint8 raster into it with LDS
//                        atomics; step_fused_bits.inc writes every word of every row from the front end's staged bits;
//   LSM_DENSE_CLIP_STEPS, LSM_DENSE_FEATURE_STEPS   the steps the workgroup's clip runs (`Tb`) and the T of its features
//                        (`Tf`), as expressions: lif_dense.h's are the launch's T or, in the ST forms, the state block's count
//                        and t0 + Tb; the fused step's tail gives a ragged clip its own count for both (SPEC.md §4c with
//                        t0 = 0) without a state block.  T stays the row stride and the size of the LDS image.
//   LSM_DENSE_ST_OFFSET  ST forms: the byte offset of the launch's StateArgs (`a.st`) in the kernel-argument segment, which
//                        the zero-step exit reads it from (state_pass_through, clip_step_count): offsetof(DenseArgs, st) where
//                        the argument struct is the kernel's only parameter, behind FusedArgs in the fused step's state forms.
    constexpr bool INREG = INMODE == 1;
    constexpr bool INMASK = INMODE >= 2;
    constexpr bool INCOL = INMODE == 3;
    constexpr int NPW = SL * 64;
    constexpr int NPAD = NPW * WPC;
    constexpr int NT = WPC * 64;
    constexpr int R = 64 / WPC;            // fixed-region list entries per producer wave
    constexpr int G = SL == 1 ? 16 : 32 / SL;   // rows in flight per group (<= 32 registers of weights)
    constexpr bool FEATREG = SL <= 4;           // feature accumulators in registers (4 per neuron) instead of LDS

    LSM_DENSE_LDS_DECL
    uint32_t *icnt = reinterpret_cast<uint32_t *>(LSM_DENSE_LDS);                     // NPAD
    uint16_t *wlist = reinterpret_cast<uint16_t *>(icnt + NPAD);                      // 2*NPAD
    uint32_t *wcnt = reinterpret_cast<uint32_t *>(wlist + 2 * NPAD);                  // 2*16 counts
    uint16_t *flist = reinterpret_cast<uint16_t *>(wcnt + 64);                        // 2*64 fixed-region list
    uint4 *feat = reinterpret_cast<uint4 *>(wcnt + 128);                              // n_out
    uint32_t *bits = reinterpret_cast<uint32_t *>(feat + a.n_out);                    // T*CW

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;      // wave-uniform
    const int N = a.N, T = a.T, CW = a.CW;
    // ST: the steps this clip runs (SPEC.md §4c), workgroup-uniform; T stays the row stride of the raster, the spike matrix
    // and the trace, and the size of the LDS image.  A clip of no steps hands its state on and is left as it is.
    constexpr bool SCALE_LATE = INMODE == 1;        // which form of the step count (lif_common.h on the two forms)
    int Tb = LSM_DENSE_CLIP_STEPS;
    if constexpr (ST) {
        if (Tb == 0) {
            state_pass_through<NT>(b, tid, LSM_DENSE_ST_OFFSET);
            return;
        }
        if constexpr (SCALE_LATE) Tb = stream_step_scale(a.st, Tb, T);
    }

    // ---- prologue: zero LDS state, bit-pack the clip's raster time-major ----
    // (zero_features_and_bits, pack_raster_bits and write_features of lif_common.h stay written out here: each call moves the
    //  registers of some form -- <4, 16, 2, REFM> 115 VGPRs for 114, <16, *, 0> two SGPR spills fewer)
    for (int i = tid; i < NPAD; i += NT) icnt[i] = 0u;
    if (tid < 64) wcnt[tid] = 0u;
    for (int i = tid; i < a.n_out; i += NT) feat[i] = make_uint4(0, 0, 0, 0);
#include LSM_DENSE_INPUT_BITS_INC

    float v[SL], lam[SL];
    int ref[REFM ? 1 : SL], os[SL];
    unsigned long long h1[REFM ? SL : 1], h2[REFM ? SL : 1];     // REFM: lanes whose countdown stands at 1 / at 2
#pragma unroll
    for (int r = 0; r < SL; ++r) {
        const int i = (w * SL + r) * 64 + lane;
        v[r] = 0.0f;
        if (REFM) { h1[r] = 0ull; h2[r] = 0ull; }
        else ref[r] = 0;
        lam[r] = a.leak[i];
        os[r] = a.oslot[i];
    }

    uint32_t im[SL][4];                 // INMASK: channels 0..127 feeding my neuron r
    if (INMASK) {
#pragma unroll
        for (int r = 0; r < SL; ++r) {
            const uint4 m = reinterpret_cast<const uint4 *>(a.inmask)[(w * SL + r) * 64 + lane];
            im[r][0] = m.x; im[r][1] = m.y; im[r][2] = m.z; im[r][3] = m.w;
        }
    }
    uint32_t in_word[IN_REG_SLOTS], in_mask[IN_REG_SLOTS], in_tgt[IN_REG_SLOTS];
    if (INREG) {
#pragma unroll
        for (int q = 0; q < IN_REG_SLOTS; ++q) {
            const int e = q * 64 + lane;
            const uint32_t x = e < a.EinW ? a.in_ent[(size_t)w * a.EinW + e] : 0xFFFFFFFFu;
            const bool ok = x != 0xFFFFFFFFu;
            const uint32_t c = x >> 16;
            in_word[q] = ok ? (c >> 5) : 0u;
            in_mask[q] = ok ? (1u << (c & 31)) : 0u;
            in_tgt[q] = ok ? (x & 0xFFFFu) : (uint32_t)(w * NPW + lane);   // padding: own slot, adds 0
        }
    }
    const float theta = a.theta, w_in = a.w_in;
    const uint32_t *my_ent = a.in_ent + (size_t)w * a.EinW;
    const bool trace = a.spike_matrix != nullptr || a.v_trace != nullptr;
    // weight of presynaptic j onto my target r: byte offset j*ld*4 (scalar, 32 bits are enough:
    // N*ld*4 <= 2^28 for N <= 8192) + my lane's byte offset (vector) + r*256 (immediate)
    const char *wt_bytes = reinterpret_cast<const char *>(a.wt);
    const uint32_t ld_bytes = (uint32_t)a.ld * 4u;
    const uint32_t lane_off = (uint32_t)(w * NPW + lane) * 4u;
    uint4 fr[FEATREG ? SL : 1];        // FEATREG: {n | bursts << 16, first | last << 16, sum t, sum isi^2} per neuron
#pragma unroll
    for (int r = 0; r < (FEATREG ? SL : 1); ++r) fr[r] = make_uint4(0, 0, 0, 0);
    uint32_t hf = 0u;                  // bit r: my neuron r fired at least once (stats)
    uint32_t tot_spk = 0u;             // spikes of my wave (stats)
    SegmentCursor sc = {nullptr, 0u, 0u};       // ST: the open segment (SPEC.md §4b)
    if constexpr (ST) sc = segment_cursor(a.st, b, T, a.n_out);
    if constexpr (ST) {
        if (a.st.in) {
            // the state after step t0-1: potentials, countdowns, and the spike lists of that step as the update leaves them
            const unsigned char *sin = a.st.in + (size_t)b * a.st.stride;
            const int NP = state_np(N);
            uint16_t *list_last = wlist + NPAD + w * NPW;
            int nspk = 0;
#pragma unroll
            for (int r = 0; r < SL; ++r) {
                const int i = (w * SL + r) * 64 + lane;
                bool last = false, ever = false;
                uint32_t rf = 0u;
                if (i < N) state_load_neuron(sin, NP, i, &v[r], &rf, &last, &ever);
                if (REFM) { h2[r] = __ballot(rf == 2u); h1[r] = __ballot(rf == 1u); }
                else ref[r] = (int)rf;
                hf |= (ever ? 1u : 0u) << r;
                const unsigned long long bal = __ballot(last);
                if (last) {
                    const int rank = nspk + lane_rank(bal);
                    list_last[rank] = (uint16_t)i;
                    if (rank < R) flist[64 + w * R + rank] = (uint16_t)i;
                }
                nspk += __popcll(bal);
            }
            if (lane == 0) wcnt[16 + w] = (uint32_t)nspk;
            tot_spk = w == 0 ? state_load_total(sin) : 0u;
        }
    }
    __syncthreads();

    // input drive of step `ts`: count the active channels feeding each target (integer atomics)
    auto input_drive = [&](int ts) {
        if (INMASK) return;
        const uint32_t *row = bits + ts * CW;
        if (INREG) {
#pragma unroll
            for (int q = 0; q < IN_REG_SLOTS; q += 2) {
                if (q * 64 < a.EinW) {          // two slots at a time, only as many as the map needs
                    const uint32_t w0 = row[in_word[q]], w1 = row[in_word[q + 1]];
                    atomicAdd(icnt + in_tgt[q], (w0 & in_mask[q]) ? 1u : 0u);
                    if ((q + 1) * 64 < a.EinW) atomicAdd(icnt + in_tgt[q + 1], (w1 & in_mask[q + 1]) ? 1u : 0u);
                }
            }
        } else {
            for (int e = lane; e < a.EinW; e += 64) {
                const uint32_t x = my_ent[e];
                if (x != 0xFFFFFFFFu) {
                    const uint32_t c = x >> 16;
                    atomicAdd(icnt + (x & 0xFFFFu), (row[c >> 5] >> (c & 31)) & 1u);
                }
            }
        }
    };

    for (int t = 0; t < Tb; ++t) {
        // The step list read and the row fetch are the latency-critical part of a step: they issue at
        // raised priority so that waves of other kernels sharing the SIMD (the float64 filterbank in the
        // pipeline) do not delay the loads; the update below runs at normal priority in their stall slots.
        // Measured inside the pipeline: launch duration 1.31 -> 1.11 ms at unchanged throughput (raising
        // the priority for the whole step gives 0.67 ms but costs 4 % of the pipeline's throughput).
        __builtin_amdgcn_s_setprio(1);
        const int cur = t & 1, prv = cur ^ 1;
        const uint16_t *list_prev = wlist + prv * NPAD;
        uint16_t *list_cur = wlist + cur * NPAD + w * NPW;

        float cin[SL];
#pragma unroll
        for (int r = 0; r < SL; ++r) cin[r] = 0.0f;
        uint32_t rowbits[4] = {0u, 0u, 0u, 0u};          // INMASK: this step's input bit row (wave-uniform)
        if (INMASK) {
            if (CW == 4) {
                const uint4 q4 = *reinterpret_cast<const uint4 *>(bits + t * 4);
                rowbits[0] = q4.x; rowbits[1] = q4.y; rowbits[2] = q4.z; rowbits[3] = q4.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) rowbits[q] = q < CW ? bits[t * CW + q] : 0u;
            }
        }

        // `todo`: filled entries of the step list; lane l holds entry l's neuron in `jl`.  Up to G rows
        // are in flight; nested "one more?" tests make a group cost one taken branch.
        bool drove = false;
        auto add_rows = [&](unsigned long long todo, uint32_t jl) {
            // entry -> byte offset of its row, once per 64 entries (N*ld*4 <= 2^28 for N <= 8192)
            const uint32_t jo = jl * ld_bytes;
            while (todo != 0ull) {
                const int n8 = min((int)__builtin_popcountll(todo), G);
                float wv[16][SL];                   // only the first G rows are ever live
#define LSM_LD(k)                                                                   \
    {                                                                               \
        const int sk = __builtin_ctzll(todo);                                       \
        const uint32_t j = __builtin_amdgcn_readlane(jo, sk);                       \
        asm volatile("s_bitset0_b64 %0, %1" : "+s"(todo) : "s"(sk));               \
        _Pragma("unroll") for (int r = 0; r < SL; ++r)                              \
            wv[k][r] = *reinterpret_cast<const float *>(wt_bytes + j + lane_off + r * 256); \
    }
                // the load chain tests the remaining-entries mask itself (one scalar 64-bit compare per row)
                LSM_LD(0)
                if (G > 1 && todo) { LSM_LD(1)
                if (G > 2 && todo) { LSM_LD(2)
                if (G > 3 && todo) { LSM_LD(3)
                if (G > 4 && todo) { LSM_LD(4)
                if (G > 5 && todo) { LSM_LD(5)
                if (G > 6 && todo) { LSM_LD(6)
                if (G > 7 && todo) { LSM_LD(7)
                if (G > 8 && todo) { LSM_LD(8)
                if (G > 9 && todo) { LSM_LD(9)
                if (G > 10 && todo) { LSM_LD(10)
                if (G > 11 && todo) { LSM_LD(11)
                if (G > 12 && todo) { LSM_LD(12)
                if (G > 13 && todo) { LSM_LD(13)
                if (G > 14 && todo) { LSM_LD(14)
                if (G > 15 && todo) { LSM_LD(15) } } } } } } } } } } } } } } }
#undef LSM_LD
                if (!drove) {                     // the input counts fill the load latency
                    input_drive(t);
                    drove = true;
                }
#define LSM_ADD(k)                                                                  \
    {                                                                               \
        _Pragma("unroll") for (int r = 0; r < SL; ++r) cin[r] = cin[r] + wv[k][r];  \
    }
                LSM_ADD(0)
                if (n8 > 1) { LSM_ADD(1)
                if (n8 > 2) { LSM_ADD(2)
                if (n8 > 3) { LSM_ADD(3)
                if (n8 > 4) { LSM_ADD(4)
                if (n8 > 5) { LSM_ADD(5)
                if (n8 > 6) { LSM_ADD(6)
                if (n8 > 7) { LSM_ADD(7)
                if (n8 > 8) { LSM_ADD(8)
                if (n8 > 9) { LSM_ADD(9)
                if (n8 > 10) { LSM_ADD(10)
                if (n8 > 11) { LSM_ADD(11)
                if (n8 > 12) { LSM_ADD(12)
                if (n8 > 13) { LSM_ADD(13)
                if (n8 > 14) { LSM_ADD(14)
                if (n8 > 15) { LSM_ADD(15) } } } } } } } } } } } } } } }
#undef LSM_ADD
            }
        };

        // ---- spiking neurons of step t-1 ----
        const uint32_t pcnt = wcnt[prv * 16 + lane / R];            // spikes of producer wave lane/R
        const uint32_t jfix = flist[prv * 64 + lane];               // its (lane%R)-th spiking neuron
        // a producer with more than R spikes does not fit its fixed region: the counts themselves say so
        if (__ballot(pcnt > (uint32_t)R) == 0ull) {
            add_rows(__ballot((uint32_t)(lane % R) < pcnt), jfix);
        } else {
            // general path: merge the per-wave lists (scalar prefix over the counts, compare chain)
            const uint32_t cv = wcnt[prv * 16 + (lane & 15)];
            uint32_t pre[WPC + 1];
            pre[0] = 0u;
#pragma unroll
            for (int q = 0; q < WPC; ++q) pre[q + 1] = pre[q] + __builtin_amdgcn_readlane(cv, q);
            const uint32_t total = pre[WPC];
            for (uint32_t l0 = 0; l0 < total; l0 += 64) {
                const uint32_t l = l0 + lane;
                uint32_t wsel = 0u, pbase = 0u;
#pragma unroll
                for (int q = 1; q < WPC; ++q) {
                    const bool ge = l >= pre[q];
                    wsel += ge ? 1u : 0u;
                    pbase = ge ? pre[q] : pbase;
                }
                uint32_t jl = 0u;
                if (l < total) jl = list_prev[wsel * NPW + (l - pbase)];
                add_rows(__ballot(l < total), jl);
            }
        }
        if (!drove) input_drive(t);
        if (!INMASK) wave_lds_fence();

        __builtin_amdgcn_s_setprio(0);
        // ---- neuron update ----
        unsigned long long bal[SL];
        unsigned long long any_fire = 0ull;
#pragma unroll
        for (int r = 0; r < SL; ++r) {
            const int i = (w * SL + r) * 64 + lane;
            uint32_t nin;
            if (INCOL) {
                // disjoint by construction of the bit positions: the union's popcount is the sum of the four.
                // (v_and_or_b32 spelled out: the compiler forms four v_and and two v_or/v_or3 from the C expression)
                uint32_t u = im[r][0] & rowbits[0];
#pragma unroll
                for (int q = 1; q < 4; ++q)
                    asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(u) : "v"(im[r][q]), "s"(rowbits[q]));
                nin = __popc(u);
            } else if (INMASK) {
                nin = __popc(im[r][0] & rowbits[0]) + __popc(im[r][1] & rowbits[1]) +
                      __popc(im[r][2] & rowbits[2]) + __popc(im[r][3] & rowbits[3]);
            } else {
                nin = icnt[i];
                icnt[i] = 0u;
            }
            cin[r] = cin[r] + w_in * (float)nin;         // SPEC.md §3: input term after the recurrent sum
            const float m = lam[r] * v[r];
            const float d = v[r] - m;
            const float vn = d + cin[r];
            if (REFM) {
                const unsigned long long held = h1[r] | h2[r];
                const unsigned long long ge = __builtin_amdgcn_fcmpf(vn, theta, 3 /* ordered >= */);
                const unsigned long long fire = ge & ~held;
                v[r] = __builtin_amdgcn_inverse_ballot_w64(ge | held) ? 0.0f : vn;
                h1[r] = h2[r];                  // 2 -> 1 (and 1 -> 0: the old h1 is dropped)
                h2[r] = fire;                   // a firing neuron (never a held one) starts at the period, 2
                bal[r] = fire;
            } else {
                const bool held = ref[r] > 0;
                const bool fire = !held && (vn >= theta);
                v[r] = (held || fire) ? 0.0f : vn;
                ref[r] = held ? ref[r] - 1 : (fire ? a.refractory : 0);
                bal[r] = __ballot(fire);
            }
            any_fire |= bal[r];
        }
        int nspk = 0;
        if (any_fire != 0ull) {                  // one branch per wave and step
#pragma unroll
            for (int r = 0; r < SL; ++r) {
                // (the mask itself becomes the execution mask: no per-lane bit test)
                const bool fire = REFM ? __builtin_amdgcn_inverse_ballot_w64(bal[r]) : (bool)((bal[r] >> lane) & 1ull);
                if (fire) {
                    const int rank = nspk + lane_rank(bal[r]);
                    const uint16_t me = (uint16_t)((w * SL + r) * 64 + lane);
                    list_cur[rank] = me;
                    if (rank < R) flist[cur * 64 + w * R + rank] = me;
                    hf |= 1u << r;
                    if (FEATREG || os[r] >= 0) {
                        // FEATREG: the accumulators of EVERY neuron of the lane sit in registers (no LDS round
                        // trip in the fire path, which all other waves wait for at the barrier); they are parked
                        // in the LDS array once, after the last step
                        uint4 f = FEATREG ? fr[r] : feat[os[r]];
                        uint32_t n = f.x & 0xFFFFu, bursts = f.x >> 16;
                        uint32_t first = f.y & 0xFFFFu, last = f.y >> 16;
                        const uint32_t isi = (uint32_t)t - last;
                        first = n == 0 ? (uint32_t)t : first;
                        f.w += n == 0 ? 0u : isi * isi;
                        bursts += (n != 0 && (int)isi <= a.burst_isi_max) ? 1u : 0u;
                        last = (uint32_t)t;
                        n += 1;
                        f.z += (uint32_t)t;
                        f.x = n | (bursts << 16);
                        f.y = first | (last << 16);
                        if (FEATREG) fr[r] = f;
                        else feat[os[r]] = f;
                    }
                }
                nspk += __popcll(bal[r]);
            }
        }
        tot_spk += (uint32_t)nspk;
        if (lane == 0) wcnt[cur * 16 + w] = (uint32_t)nspk;   // > R: next step's consumers merge the lists
        if constexpr (ST) {
            if (segment_ends(sc, t)) {           // the owners close their records (FEATREG: straight from the registers)
                if constexpr (FEATREG) {
#pragma unroll
                    for (int r = 0; r < SL; ++r) {
                        if (os[r] >= 0) segment_close(sc, os[r], fr[r]);
                        fr[r] = make_uint4(0, 0, 0, 0);
                    }
                } else {
#pragma unroll 1
                    for (int r = 0; r < SL; ++r) segment_close_lds(sc, feat, a.oslot[(w * SL + r) * 64 + lane]);
                }
                segment_next(&sc, a.st.seg, a.n_out);
            }
        }
        if (trace) {
#pragma unroll
            for (int r = 0; r < SL; ++r) {
                const int i = (w * SL + r) * 64 + lane;
                if (i < N) {
                    if (a.spike_matrix)
                        a.spike_matrix[((size_t)b * T + t) * N + i] = (uint8_t)((bal[r] >> lane) & 1ull);
                    if (a.v_trace) a.v_trace[((size_t)b * T + t) * N + i] = v[r];
                }
            }
        }
        __syncthreads();
    }

    if (FEATREG) {
#pragma unroll
        for (int r = 0; r < SL; ++r)
            if (os[r] >= 0) feat[os[r]] = fr[r];
        __syncthreads();
    }
    // ---- epilogue: health statistics (/root/reference/extract_lsm_features.py:119-133 derives them from the
    //      (T, N) spike matrix; here they come from one flag per neuron and one count per wave), then
    //      SPEC.md §4 features from the integer accumulators (float64, then float32) ----
    if constexpr (ST) {
        // the state after the last step (the count array is idle: scratch), and the feature records of the whole run
        const unsigned char *sin = a.st.in ? a.st.in + (size_t)b * a.st.stride : nullptr;
        unsigned char *sout = a.st.out ? a.st.out + (size_t)b * a.st.stride : nullptr;
        uint32_t *scratch = icnt;
        const int NP = state_np(N);
        state_begin<NT>(scratch, NP, tid);
#pragma unroll
        for (int r = 0; r < SL; ++r) {
            const uint32_t rf = REFM ? (((h2[r] >> lane) & 1ull) ? 2u : (uint32_t)((h1[r] >> lane) & 1ull)) : (uint32_t)ref[REFM ? 0 : r];
            state_store_neuron(sout, scratch, NP, N, (w * SL + r) * 64 + lane, v[r], rf, (hf >> r) & 1u);
        }
        const int lastbuf = (Tb - 1) & 1;
        const uint16_t *list_last = wlist + lastbuf * NPAD + w * NPW;
        const int nlast = (int)wcnt[lastbuf * 16 + w];
        for (int l = lane; l < nlast; l += 64) state_mark_last(scratch, list_last[l]);
        if (lane == 0) state_add_total(scratch, NP, tot_spk);
        // (a stream launch, SPEC.md §4d, keeps no cumulative record: no fold, and state_finish does not merge)
        if (a.st.seg > 0 && a.st.t0 != STREAM_T0) segment_fold<NT>(a.st, b, Tb, feat, a.n_out, a.burst_isi_max, tid);
        state_finish<NT>(sin, sout, scratch, feat, NP, a.n_out, (uint32_t)a.st.t0, a.burst_isi_max, tid);
    }
    const int Tf = LSM_DENSE_FEATURE_STEPS;         // lif_dense.h: the features are those of [0, t0 + Tb)
    if (a.stats) write_stats(a.stats, b, &wcnt[32], &wcnt[33], hf, tot_spk, lane, tid);
    const int nf = a.n_keys * a.n_out;
    for (int idx = tid; idx < nf; idx += NT) {
        const int kq = idx / a.n_out;
        const int o = idx - kq * a.n_out;
        const uint4 f = feat[o];
        const int n = (int)(f.x & 0xFFFFu), bursts = (int)(f.x >> 16);
        const int first = (int)(f.y & 0xFFFFu), last = (int)(f.y >> 16);
        double val = 0.0;
        switch (a.key_ids[kq]) {
        case 0: val = (double)n; break;
        case 1: { const double p = (double)n / (double)Tf; val = p * (1.0 - p); } break;
        case 2: val = n >= 1 ? (double)f.z / (double)n : 0.0; break;
        case 3: val = n >= 1 ? (double)first : 0.0; break;
        case 4: val = n >= 1 ? (double)last : 0.0; break;
        case 5: val = n >= 2 ? (double)(last - first) / (double)(n - 1) : 0.0; break;
        case 6:
            if (n >= 2) {
                const double m = (double)(last - first) / (double)(n - 1);
                val = (double)f.w / (double)(n - 1) - m * m;
            }
            break;
        default: val = (double)bursts; break;
        }
        a.features[(size_t)b * nf + idx] = (float)val;
    }
