// wfk_iir_rows_sampled_kernels.inc -- the two kernels of the sampler inside the per-row IIR stage (DESIGN.md §3.8.2),
// included as TEXT by wfk_iir_rows_sampled.hip, once per way a tile leaves LDS:
//   as T     iir_rows_sampled / iir_rows_short           IRS_K(name) = name, IRS_OUT_PARAMS = the T rows, the body stores
//                                                        through wfk_iir_rows_store.inc
//   as codes iir_rows_sampled_dac / iir_rows_short_dac   IRW_DAC defined, IRS_K(name) = name_dac, IRS_OUT_PARAMS = the int16
//                                                        rows and IRW_DAC_PARAMS, IRW_OUT_T = int16_t, the body stores
//                                                        through wfk_iir_rows_store_dac.inc (DESIGN.md §3.23)
//   as codes, the row's curve in front of the tile       IRW_DAC and IRW_CURVE defined, IRS_K(name) = name_curve_dac,
//            iir_rows_sampled_curve_dac /                IRS_OUT_PARAMS with IRW_CURVE_PARAMS behind IRW_DAC_PARAMS
//            iir_rows_short_curve_dac                    (DESIGN.md §3.24): every sample the fill produces goes through
//                                                        through_curve (wfk_iir_rows_curve_row.inc) before the sweeps
// The fills are the same text every way; what IRW_CURVE adds expands to nothing without it.
// ---- the lean fill: stride-256 chains (the sampling phase of fir_sampled, CL = 16, no carried op state) -----------
template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) IRS_K(iir_rows_sampled)(const IrsLeanArgs a, IRS_OUT_PARAMS
                                                                       const double* __restrict__ tab,
                                                                       const double* __restrict__ zi,
                                                                       double* __restrict__ zf,
                                                                       const double* __restrict__ initial, int64_t n) {
  constexpr int CL = IRW_RUN;
#include "wfk_iir_rows_head.inc"
#ifdef IRW_DAC
#include "wfk_iir_rows_dac_row.inc"
#endif
#ifdef IRW_CURVE
#include "wfk_iir_rows_curve_row.inc"
#endif
  __shared__ __attribute__((aligned(16))) double s_par[IRS_PAR + 2 * (CL + 1)];
  double2* const unit_tab = reinterpret_cast<double2*>(s_par + IRS_PAR);
  const DevChannel C = a.channels[row];
  if (tid <= CL) unit_tab[tid] = make_double2(1.0, 0.0);       // phasor table of ops without a carrier
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t s1 = t * IRW_TILE, range_end = s1 + IRW_TILE; // per-thread sample index: s1 + tid + 256 k
    T acc[CL];
    CH_EACH(CL, k) acc[k] = (T)0; CH_END
    double x;
    {
      // t[j] = fl(fl(j*step) + t0) (NumPy's linspace / arange element formula), as fir_sampled's chain_time.  As there,
      // the time is taken for the chain's FIRST sample only: an endpoint grid's overridden last sample gets `last` where
      // it starts a chain (k = 0); further down a chain its time is the stride-256 continuation, one ulp of t away
#pragma clang fp contract(off)
      const int64_t j = s1 + tid;
      const double m = (double)(j + a.i0) * a.step;
      x = m + a.t0;
      if (a.has_last && j == n - 1) x = a.last;
    }
    if (C.tshift != 0.0) x = x - C.tshift;
    int q = cuni(a.tile_first[row * ntile + t]);
    for (; q < C.piece_end; q = cuni(q + 1)) {
      const DevPiece P = a.pieces[q];
      if (P.start >= range_end) break;
      if (P.n_blk == 0 || P.stop <= s1) continue;               // zero piece / entirely before the tile
      __syncthreads();                                           // every wave is done with the previous block
      for (int i = tid; i < P.first_len; i += IRW_THREADS) s_par[i] = a.params[P.par_off + i];
      __syncthreads();
      const int nops = cuni((int)s_par[1]);
      const bool full = P.start <= s1 && P.stop >= range_end;   // wave-uniform: the whole tile is inside
      int klo = 0, khi = CL;
      if (!full) {
        // samples k of this thread inside the piece: P.start <= s1 + tid + 256 k < P.stop (scalar parts clamped to
        // what matters for k in [0, CL): the per-thread part is 32-bit)
        const int64_t lim = 256 * (int64_t)(CL + 2);
        const int64_t los = P.start - s1, his = P.stop - s1;
        const int lo = (int)(los < -lim ? -lim : (los > lim ? lim : los)) - tid;
        const int hi = (int)(his < -lim ? -lim : (his > lim ? lim : his)) - tid;
        klo = lo <= 0 ? 0 : (lo + 255) >> 8;
        khi = hi <= 0 ? 0 : (hi + 255) >> 8;
        klo = klo > CL ? CL : klo;
        khi = khi > CL ? CL : khi;
      }
      for (int op = 0; op < nops; ++op) {
        const double* rec = s_par + WFK_BLK_HDR + op * WFK_FCE_REC;
        const int fl = cuni(WFK_FCE_WORD(rec));
        const int env = (fl >> 4) & 3, carrier = (fl >> 2) & 1;
        ChSeeds nx;
        const ChSeeds sd = chain_make_seeds(rec, x, fl);         // exact
        if (env == 3) {
          chain_envmul<T, CL, -1>(rec, sd, acc, klo, khi, nx);
        } else {
          const double2* ptab = carrier ? reinterpret_cast<const double2*>(s_par + WFK_FCE_TABOFF(fl)) : unit_tab;
          const double qq = env ? rec[WFK_FCE_Q] : 1.0;
          const double u0 = x - rec[WFK_FCE_SLIN];
          if (full && (fl & 3) <= 1) chain_loop<T, CL, -1, false, true>(ptab, rec, sd, u0, qq, acc, 0, CL, nx);
          else if (full) chain_loop<T, CL, -1, false, false>(ptab, rec, sd, u0, qq, acc, 0, CL, nx);
          else chain_loop<T, CL, -1, true, false>(ptab, rec, sd, u0, qq, acc, klo, khi, nx);
        }
      }
    }
    // channel offset inside [0, n), zeros behind the row; into the tile by the scatter of iir_rows_tile's loads
    // (the previous tile's body ended with a barrier: the array is free)
    const T off = (T)C.offset;
    const int64_t left = n - s1;
    CH_EACH(CL, k)
      const int j = k * IRW_THREADS + tid;
#ifdef IRW_CURVE
      tile[irw_at(j)] = through_curve(acc[k] + off, j < left);   // in the register: neighbouring lanes, neighbouring samples
#else
      tile[irw_at(j)] = j < left ? acc[k] + off : (T)0;
#endif
    CH_END
    __syncthreads();
    {
      const int64_t base = s1;
      double L[MM];                                              // T^lane, read here: after the fill
#pragma unroll
      for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
#include "wfk_iir_rows_body.inc"
    }
  }
#ifdef IRW_DAC
#include "wfk_iir_rows_dac_end.inc"
#endif
#ifdef IRW_CURVE
#include "wfk_iir_rows_curve_end.inc"
#endif
}

// ---- the short fill: runs of one piece (the entry evaluation of fir_short) -----------------------------------------
template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) IRS_K(iir_rows_short)(const IrsShortArgs a, IRS_OUT_PARAMS
                                                                     const double* __restrict__ tab,
                                                                     const double* __restrict__ zi,
                                                                     double* __restrict__ zf,
                                                                     const double* __restrict__ initial, int64_t n) {
  constexpr int R = WFK_SH_R;
  static_assert(R == IRW_RUN, "an entry is at most one run of the tile");
#include "wfk_iir_rows_head.inc"
#ifdef IRW_DAC
#include "wfk_iir_rows_dac_row.inc"
#endif
#ifdef IRW_CURVE
#include "wfk_iir_rows_curve_row.inc"
#endif
  const DevChannel C = a.channels[row];
  const double coff = C.offset;
  const ShortWin* const wp = a.wins + row * 2 * a.npairs;
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t h0 = t * IRW_TILE, left = n - h0;
    const int64_t rec0 = cuni64(wp[t].rec0), e0 = cuni64(wp[t].e0);   // (block-uniform: SGPRs)
    const int cnt = cuni(wp[t].cnt);
    // zeros behind the row, the channel offset inside (skipped zero pieces, gaps between entries); the previous tile's
    // body ended with a barrier: the array is free.  Always the padded layout: it is the tile's
    CH_EACH(IRW_RUN, k)
      const int j = k * IRW_THREADS + tid;
      tile[irw_at(j)] = j < left ? (T)coff : (T)0;
    CH_END
    __syncthreads();
    for (int eb = 0; eb < cnt; eb += IRW_THREADS) {             // block-uniform trip count
      const int idx = eb + tid;
      bool live = idx < cnt;
      const uint32_t word = live ? a.entries[e0 + idx] : 0u;
      const int len = live ? (int)(word >> 28) + 1 : 0;
      const int o = (int)((word >> 16) & 0xfff);
      const double* op = a.recs + 2 * (rec0 + (int64_t)(word & 0xffff));
      shdev::OpRec rec = shdev::load_op(op);
      const double kf = (double)((int)(uint32_t)(h0 + o) - shdev::op_ref(rec));   // samples from the record's reference sample
      double acc[R], acci[1];
      CH_EACH(R, k) acc[k] = 0.0; CH_END
      acci[0] = 0.0;
      auto eval = [&](const shdev::OpRec& rc, const double* opp, bool lv) -> bool {   // -> another op follows
        const int w = shdev::op_word(rc);
        const bool closing = ((w >> 4) & 3) == 3;               // erf edge multiplier
        const bool mine = lv && !closing && !(w & 8);           // (real channels only: no op of an imaginary part)
        const bool cubic = __any(mine && (w & 3) > 1);
        if (mine) {
          if (cubic) shdev::short_op<R, true, false>(rc, opp, w, kf, a.step, acc, acci);
          else shdev::short_op<R, false, false>(rc, opp, w, kf, a.step, acc, acci);
        }
        if (__any(lv && closing)) {
          if (lv && closing) shdev::short_erfmul<R, false>(rc, kf, acc, acci);
        }
        return lv && !(w & WFK_SH_LAST);
      };
      live = eval(rec, op, live);
      while (__any(live)) {
        op += (shdev::op_word(rec) & 3) > 1 ? WFK_SH_OP3 : WFK_SH_OP1;
        if (live) rec = shdev::load_op(op);
        live = eval(rec, op, live);
      }
      if (C.do_clip) {
        CH_EACH(R, k) acc[k] = shdev::clip_np(acc[k], C.clip_lo, C.clip_hi); CH_END
      }
      // element o + k of the tile sits at (o + k) + ((o + k) >> 4) = irw_at(o) + k + [k >= 16 - (o & 15)]
      T* const b0 = tile + o + (o >> 4);
      const int tk = 16 - (o & 15);
      CH_EACH(R, k)
        if (k < len) *((k >= tk ? b0 + 1 : b0) + k) = (T)(acc[k] + coff);
      CH_END
    }
    __syncthreads();
#ifdef IRW_CURVE
    // entries overwrite the offset the tile was filled with, so a sample is final only here: each lane takes its own run
    // through the curve (the run the sweeps read next: no barrier between); the zeros behind the row stay zeros
    CH_EACH(IRW_RUN, k)
      my[k] = through_curve(my[k], tid * IRW_RUN + k < left);
    CH_END
#endif
    {
      const int64_t base = h0;
      double L[MM];                                              // T^lane, read here: after the fill
#pragma unroll
      for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
#include "wfk_iir_rows_body.inc"
    }
  }
#ifdef IRW_DAC
#include "wfk_iir_rows_dac_end.inc"
#endif
#ifdef IRW_CURVE
#include "wfk_iir_rows_curve_end.inc"
#endif
}
