// step_fused_bits.inc -- the fused step kernel's input bit rows (lif_dense_kernel.inc, LSM_DENSE_INPUT_BITS_INC), straight
// from the front end's staged raster bits in LDS (step_fused_tail.inc declares step_stage, step_rw, step_red).
// The stage holds channel c's T raster bits as the words step_stage[(c / redundancy) * RW + k]; the time loop reads step t's
// input as the 128-bit row bits[t * 4 ..], channel c at bit a.inperm[c].  Lane l of a wave with position half `ph` takes the
// channel whose bit position is ph * 64 + l (`inv`, the inverse of inperm, 0xFF where no channel sits) and reads that
// channel's staged word k: the 32 ballots of the word's bits are the two words of half `ph` of the rows of steps 32 k ..
// 32 k + 31.  Waves 0 / 1 take the even staged words, waves 2 / 3 the odd ones.  Every word of every row is written exactly
// once, so `bits` is not zeroed first, and nothing here is an atomic.
// RAGGED: the clip owns its first Tb steps only -- the staged words past ceil(Tb / 32) were never written and the time loop
// reads no row past Tb -- so the hand-off stops there; the stage's and the rows' strides stay the launch's.
    uint8_t *inv = reinterpret_cast<uint8_t *>(bits + T * CW);          // 128 bit positions -> channel
    if (tid < 128) inv[tid] = 0xFFu;
    __syncthreads();                                                    // (also: icnt, wcnt and feat are zeroed)
    if (tid < a.C && a.inperm[tid] < 128) inv[a.inperm[tid]] = (uint8_t)tid;
    __syncthreads();
    {
        const int ph = w & 1;
        const uint32_t ch = inv[ph * 64 + lane];
        const uint32_t *srow = step_stage + (ch == 0xFFu ? 0u : ch / (uint32_t)step_red) * step_rw;
        const int own_steps = RAGGED ? Tb : T;                          // the steps handed off, and the staged words that
        const int own_rw = RAGGED ? (Tb + 31) >> 5 : step_rw;           // hold them
        for (int k = w >> 1; k < own_rw; k += 2) {
            const uint32_t word = ch == 0xFFu ? 0u : srow[k];
            const int nb = min(32, own_steps - 32 * k);
            for (int i = 0; i < nb; ++i) {
                const unsigned long long bal = __ballot(((word >> i) & 1u) != 0u);
                if (lane == 0)
                    *reinterpret_cast<uint2 *>(bits + (32 * k + i) * 4 + 2 * ph) = make_uint2((uint32_t)bal, (uint32_t)(bal >> 32));
            }
        }
    }
