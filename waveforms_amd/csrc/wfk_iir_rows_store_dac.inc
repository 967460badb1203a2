// wfk_iir_rows_store_dac.inc -- the store section of the per-row IIR tile body that writes int16 DAC codes, the
// expansion of IRW_STORE_INC in iir_rows_dac (wfk_iir_rows_dac.hip): after sweep 2 the tile holds y in LDS, already
// rounded to T; here it goes through the statements of dac_block (wfk_dac_rows.hip) in their order and leaves as codes.
// A tile is 512 slots of 8 codes (16 bytes).  Lane l takes slots 2 l and 2 l + 1: its OWN run of 16 samples, at
// l * IRW_PITCH elements -- the pattern of the sweeps, 32 lanes of a read on 32 distinct banks.  (The map that would
// coalesce best, slot l and slot l + 256, reads elements 17 (l >> 1) + 8 (l & 1) + e: in fp64 lanes 1 and 16, 3 and 18,
// ... of every 32 meet on a bank.)  A lane's two slots are 32 consecutive bytes; a wave's two stores fill whole lines.
// In scope beyond the body's names: y (int16_t*), dgain, doff, lo, hi, shift, counts, vec16 (the row's slot addresses
// are 16-byte aligned: one test per workgroup), n_below / n_above / n_nan (this wave's counts so far, scalar).
    __syncthreads();
    {
#pragma clang fp contract(off)   // a rounded product and a rounded sum, as dac_block
#pragma unroll
      for (int h = 0; h < IRW_RUN / 8; ++h) {
        // From here to the stores every lane of the wave runs every statement: the counts are ballots.
        int w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const double v = (double)tile[irw_at(tid * IRW_RUN + 8 * h + e)] * dgain + doff;
          const double q = rint(v);
          const bool nan = v != v, below = q < lo, above = q > hi;
          const double c = nan ? 0.0 : below ? lo : above ? hi : q;
          w[e] = (int)c * (1 << shift);
          if (counts) {                                                 // (workgroup-uniform: a scalar branch)
            const bool live = 8 * h + e < cnt;
            n_below += (unsigned)__popcll(__ballot(live && below));
            n_above += (unsigned)__popcll(__ballot(live && above));
            n_nan += (unsigned)__popcll(__ballot(live && nan));
            // (as in dac_block: the sums exist here, in scalar registers, not as lane masks kept to the end)
            asm volatile("" : "+s"(n_below), "+s"(n_above), "+s"(n_nan));
          }
        }
        const int have = cnt - 8 * h;                                   // codes of this slot inside the row
        int16_t* const dst = y + base + tid * IRW_RUN + 8 * h;
        if (vec16 && have >= 8) {
          uint4 q;
          q.x = (uint32_t)(w[0] & 0xffff) | ((uint32_t)w[1] << 16);
          q.y = (uint32_t)(w[2] & 0xffff) | ((uint32_t)w[3] << 16);
          q.z = (uint32_t)(w[4] & 0xffff) | ((uint32_t)w[5] << 16);
          q.w = (uint32_t)(w[6] & 0xffff) | ((uint32_t)w[7] << 16);
          *reinterpret_cast<uint4*>(dst) = q;
        } else {                           // a partial slot is written code by code, never read-modify-written
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < have) dst[e] = (int16_t)w[e];
        }
      }
    }
    __syncthreads();
