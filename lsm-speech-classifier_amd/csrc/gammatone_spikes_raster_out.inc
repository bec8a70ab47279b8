// gammatone_spikes_raster_out.inc -- the end of the fused gammatone kernel (gammatone_spikes_kernel.inc, LSM_FUSED_TAIL_INC)
// in its three raster-writing forms: the wave's staged bit rows leave as the uint8 raster, in coalesced 4-byte stores.
    if (valid) {
        // create_pure_redundancy: output row c reads filter row c / redundancy
        const int R = a.redundancy;
        const int fbase = g * NCH * CPW;
        const int rows_out = min(NCH * CPW, F - fbase) * R;
        // RAGGED: a row keeps the launch's length; the clip owns its first row_bits bytes, the rest is written as 0 (the stage
        // holds nothing of the clip past them)
        const int row_bytes = RAGGED ? a.time_bins * n_thr : row_bits;
        uint8_t *dst = a.raster + ((size_t)b * F + fbase) * R * row_bytes;
        if ((row_bytes & 3) == 0) {
            const int rw = row_bytes >> 2;
            uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
            for (int i = lane; i < rows_out * rw; i += 64) {
                const int c = i / rw;
                const int p = (i - c * rw) * 4;
                uint32_t nib = (stage[(c / R) * RW + (p >> 5)] >> (p & 31)) & 0xFu;
                if constexpr (RAGGED) nib &= (1u << min(max(row_bits - p, 0), 4)) - 1u;
                d4[i] = (nib * 0x00204081u) & 0x01010101u;
            }
        } else {
            for (int i = lane; i < rows_out * row_bytes; i += 64) {
                const int c = i / row_bytes;
                const int p = i - c * row_bytes;
                uint32_t bit = (stage[(c / R) * RW + (p >> 5)] >> (p & 31)) & 1u;
                if constexpr (RAGGED) bit = p < row_bits ? bit : 0u;
                dst[i] = (uint8_t)bit;
            }
        }
    }
