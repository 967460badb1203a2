// wfk_iir_rows_dac_end.inc -- the end of a row in a per-row IIR kernel that ends in DAC codes, included as TEXT behind the
// tile loop: the workgroup owns the row, so the waves' counts (wfk_iir_rows_dac_row.inc) meet in LDS once and the row's
// [below, above, nan] are STORED -- no atomic, no zeroing in front.  counts == nullptr: nothing was counted.
  if (counts) {
    if (lane == 0) { s_cnt[wv][0] = n_below; s_cnt[wv][1] = n_above; s_cnt[wv][2] = n_nan; }
    __syncthreads();
    if (tid < 3) {
      unsigned long long sum = 0;
#pragma unroll
      for (int w = 0; w < IRW_WAVES; ++w) sum += s_cnt[w][tid];
      counts[row * 3 + tid] = sum;
    }
  }
