// wfk_iir_rows_body.inc -- the tile body of the per-row IIR kernels, written once and included as TEXT inside the tile loop
// of iir_rows_tile (wfk_iir_rows.hip) and of iir_rows_sampled / iir_rows_short (wfk_iir_rows_sampled.hip): everything
// after the fill of the tile -- sweep from zero state, double-double wave scan, carry chain, replay from LDS, and the
// store section the kernel names in IRW_STORE_INC: whole-line stores of T (wfk_iir_rows_store.inc: these three kernels) or
// int16 DAC codes (wfk_iir_rows_store_dac.inc: iir_rows_dac and the _dac builds of the other two) (DESIGN.md §3.8.1,
// steps 2-4; §3.23).  Text, not a function: behind a call boundary (a __forceinline__ function, even
// an always-inline lambda inside the kernel) the compiler schedules iir_rows_tile differently and takes 16 more VGPRs in
// every instantiation, which costs the state-dimension-4 shapes a wave per SIMD (DESIGN.md §3.8.2 has the figures);
// included, iir_rows_tile keeps its instruction words (tools/kernel_cmp.py).
// In scope where it is included (wfk_iir_rows_dev.h lists them): T, NSEC, ORD, D; tile, s_tot, s_carry; tid, lane, wv, my;
// B, A, pw, W, L (T^lane as (hi, lo) pairs), pre; zf, row, y; t, base = t * IRW_TILE, left = n - base.  The tile holds the
// samples (zeros past the end of the row) and a barrier has made them visible; the text ends with a barrier, after which
// the tile array is free again.
    const int64_t mine = left - (int64_t)tid * IRW_RUN;                 // samples of the row from this lane's run on
    const int cnt = (int)(mine < 0 ? 0 : (mine > IRW_RUN ? IRW_RUN : mine));

    // ---- sweep 1: zero state -> local end state; inclusive scan over the wave
    double z[D];
#pragma unroll
    for (int i = 0; i < D; ++i) z[i] = 0.0;
    if (cnt == IRW_RUN) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) (void)iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z);
    } else {
      for (int i = 0; i < cnt; ++i) (void)iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z);
    }
    // (a lane past the end of the row keeps a zero state; the scan still multiplies by T per lane, which only
    //  matters AFTER the last sample -- nothing there is used)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int d = 1 << k;
      double u[D], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) u[i] = __shfl_up(z[i], d);
      dd_matvec_add<D>(r, z, pw + k * MM, u);
#pragma unroll
      for (int i = 0; i < D; ++i) z[i] = lane >= d ? r[i] : z[i];
    }
    double vprev[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double up = __shfl_up(z[i], 1);
      vprev[i] = lane == 0 ? 0.0 : up;
    }
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i < D; ++i) s_tot[wv][i] = z[i];
    }
    __syncthreads();

    // ---- state at this wave's start: the carry pushed through the waves before it
    double S[D];
#pragma unroll
    for (int i = 0; i < D; ++i) S[i] = s_carry[t & 1][i];
    for (int w = 0; w < wv; ++w) {
      double tot[D], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) tot[i] = s_tot[w][i];
      dd_matvec_add<D>(r, tot, W, S);
#pragma unroll
      for (int i = 0; i < D; ++i) S[i] = r[i];
    }
    if (wv == IRW_WAVES - 1) {     // the next tile's carry (double-buffered: the other waves still read this tile's)
      double r[D];
      dd_matvec_add<D>(r, z, W, S);                                    // lane 63: z = this wave's total
      if (lane == 63) {
#pragma unroll
        for (int i = 0; i < D; ++i) s_carry[(t + 1) & 1][i] = r[i];
      }
    }

    // ---- sweep 2 from the true start state v_(l-1) + T^l S_w, y over x in LDS
    dd_matvec_add<D>(z, vprev, L, S);
    if (cnt == IRW_RUN) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) my[i] = (T)(iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z) + pre);
    } else {
      for (int i = 0; i < cnt; ++i) my[i] = (T)(iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z) + pre);
    }
    if (zf && cnt > 0 && mine <= IRW_RUN) {                             // the lane that holds the row's last sample
#pragma unroll
      for (int i = 0; i < D; ++i) zf[row * D + i] = z[i];
    }
    // ---- the store section (from the barrier after sweep 2 to the barrier that frees the tile): IRW_STORE_INC, the text
    // each kernel names -- wfk_iir_rows_store.inc writes the tile as T, wfk_iir_rows_store_dac.inc as int16 DAC codes
#include IRW_STORE_INC
