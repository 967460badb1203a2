// wfk_iir_rows_curve_end.inc -- the end of a row in a per-row IIR kernel with the curve in front, included as TEXT behind
// wfk_iir_rows_dac_end.inc: the waves' `beyond` counts (wfk_iir_rows_curve_row.inc) meet in LDS once and the row's
// [below, above, nan] are STORED -- no atomic, no zeroing in front.  beyond == nullptr: nothing was counted.
  if (beyond) {
    if (lane == 0) { s_bey[wv][0] = b_below; s_bey[wv][1] = b_above; s_bey[wv][2] = b_nan; }
    __syncthreads();
    if (tid < 3) {
      unsigned long long sum = 0;
#pragma unroll
      for (int w = 0; w < IRW_WAVES; ++w) sum += s_bey[w][tid];
      beyond[row * 3 + tid] = sum;
    }
  }
