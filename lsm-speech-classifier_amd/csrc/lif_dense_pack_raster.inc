// lif_dense_pack_raster.inc -- lif_dense_kernel's input bit rows from the clip's uint8 raster (lif_dense_kernel.inc,
// LSM_DENSE_INPUT_BITS_INC): `bits` zeroed, a barrier, then every non-zero raster byte sets its bit with an LDS atomic.
    for (int i = tid; i < Tb * CW; i += NT) bits[i] = 0u;
    __syncthreads();
    {
        const uint8_t *clip = a.raster + (size_t)b * a.C * T;
        if ((T & 3) == 0) {
            const uint32_t *clip4 = reinterpret_cast<const uint32_t *>(clip);
            const int nd = a.C * T / 4;
            for (int q = tid; q < nd; q += NT) {
                const uint32_t v = clip4[q];
                if (v == 0) continue;
                const int c = (q * 4) / T;
                const int t0 = (q * 4) - c * T;
                if (ST && t0 >= Tb) continue;                       // ST: only the steps t < Tb are packed
                const int pc = INCOL ? (int)a.inperm[c] : c;        // the channel's place in the bit row
                const uint32_t bit = 1u << (pc & 31);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (((v >> (8 * k)) & 0xFFu) && (!ST || t0 + k < Tb)) atomicOr(&bits[(t0 + k) * CW + (pc >> 5)], bit);
            }
        } else {
            const int nb = a.C * T;
            for (int q = tid; q < nb; q += NT)
                if (clip[q]) {
                    const int c = q / T;
                    if (ST && q - c * T >= Tb) continue;
                    const int pc = INCOL ? (int)a.inperm[c] : c;
                    atomicOr(&bits[(q - c * T) * CW + (pc >> 5)], 1u << (pc & 31));
                }
        }
    }
