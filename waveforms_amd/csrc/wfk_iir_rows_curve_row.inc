// wfk_iir_rows_curve_row.inc -- what a per-row IIR kernel with the row's calibration curve in front of its tile adds to
// the row head, included as TEXT behind wfk_iir_rows_head.inc and wfk_iir_rows_dac_row.inc by iir_rows_curve_dac
// (wfk_iir_rows_curve_dac.hip) and iir_rows_sampled_curve_dac / iir_rows_short_curve_dac
// (wfk_iir_rows_sampled_kernels.inc): the row's CurveRow by scalar loads, its knots and buckets copied into dynamic LDS
// ONCE for the whole row, this wave's three `beyond` counts, and through_curve -- curve_block's statements
// (wfk_curve_rows.hip) in their order, contraction off, the "outside samples search for x0" trick included -- which a
// sample passes on its way into the tile.  Every lane of a wave calls through_curve the same number of times (the counts
// are ballots).  In scope: IRW_CURVE_PARAMS.  wfk_iir_rows_curve_end.inc stores the row's counts.
  extern __shared__ __attribute__((aligned(16))) char c_lds[];          // xp, fp, slope: lds_knots doubles each; buckets
  __shared__ unsigned long long s_bey[IRW_WAVES][3];
  const CurveRow crow = crows[row];                                     // workgroup-uniform: scalar loads
  {
    double* const sx = reinterpret_cast<double*>(c_lds);
    double* const sf = sx + lds_knots;
    double* const ss = sf + lds_knots;
    uint32_t* const sb = reinterpret_cast<uint32_t*>(ss + lds_knots);
    const double* __restrict__ g = cknots + crow.off;
    for (int i = tid; i < crow.K; i += IRW_THREADS) {
      sx[i] = g[i];
      sf[i] = g[crow.K + i];
      ss[i] = g[2 * crow.K + i];
    }
    const uint32_t* __restrict__ gb = cbuckets + crow.boff;
    for (int i = tid; i < crow.nb; i += IRW_THREADS) sb[i] = gb[i];
  }
  __syncthreads();
  const Knots cknot{reinterpret_cast<const double*>(c_lds), reinterpret_cast<const double*>(c_lds) + lds_knots,
                    reinterpret_cast<const double*>(c_lds) + 2 * lds_knots,
                    reinterpret_cast<const uint32_t*>(reinterpret_cast<const double*>(c_lds) + 3 * lds_knots)};
  unsigned long long b_below = 0, b_above = 0, b_nan = 0;               // this wave's counts over the row, scalar
  // xs: a sample; live: it lies inside [0, n) (only those are counted; the tile's padding stays zero)
  const auto through_curve = [&](T xs, bool live) -> T {
#pragma clang fp contract(off)   // a rounded difference, a rounded product and a rounded sum, as curve_block
    const double xe = (double)xs;
    const bool nan = xe != xe, below = xe < crow.x0, above = xe > crow.xl;
    // a sample outside the knots searches for x0: every lane of a wave stays in one loop
    const double inside = curve_at(cknot, crow, (nan || below || above) ? crow.x0 : xe);
    const T v = (T)(nan ? xe : below ? crow.left : above ? crow.right : inside);
    if (beyond) {                                                       // (workgroup-uniform: a scalar branch)
      b_below += (unsigned)__popcll(__ballot(live && below));
      b_above += (unsigned)__popcll(__ballot(live && above));
      b_nan += (unsigned)__popcll(__ballot(live && nan));
      asm volatile("" : "+s"(b_below), "+s"(b_above), "+s"(b_nan));    // sums in scalar registers, as the converter's
    }
    return live ? v : (T)0;
  };
