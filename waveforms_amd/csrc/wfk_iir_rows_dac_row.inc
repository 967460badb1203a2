// wfk_iir_rows_dac_row.inc -- what a per-row IIR kernel that ends in DAC codes adds to the row head, included as TEXT
// behind wfk_iir_rows_head.inc by iir_rows_dac (wfk_iir_rows_dac.hip) and iir_rows_sampled_dac / iir_rows_short_dac
// (wfk_iir_rows_sampled_kernels.inc): the row's gain and offset, whether its slot addresses are aligned, and this wave's
// three counts -- the names wfk_iir_rows_store_dac.inc and wfk_iir_rows_dac_end.inc expect.  In scope: IRW_DAC_PARAMS.
  __shared__ unsigned long long s_cnt[IRW_WAVES][3];
  const double dgain = gd[2 * row], doff = gd[2 * row + 1];          // workgroup-uniform: scalar loads
  // a slot of tile t starts 2 * (t * 4096 + 8 s) bytes into the row: aligned in every tile or in none
  const bool vec16 = ((uintptr_t)y & 15) == 0;
  unsigned long long n_below = 0, n_above = 0, n_nan = 0;            // this wave's counts over the row, scalar
