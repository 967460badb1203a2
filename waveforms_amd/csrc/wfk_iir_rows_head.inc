// wfk_iir_rows_head.inc -- the row head of the per-row IIR kernels, included as TEXT at the top of iir_rows_tile
// (wfk_iir_rows.hip) and of iir_rows_sampled / iir_rows_short (wfk_iir_rows_sampled.hip): the LDS arrays, the thread's
// place, the row's table (layout: irw_row_doubles, wfk_iir_rows_dev.h) with its coefficients in registers, its level,
// its carry seeded from zi, its output and tile count -- the names wfk_iir_rows_body.inc expects.
// In scope where it is included: T, NSEC, ORD; the kernel arguments out, out_stride, tab, zi, initial, n.
// IRW_LOADS_INPUT (defined by wfk_iir_rows.hip): the kernel loads its tiles from `in` -- it holds L = T^lane for the whole
// row and has the row's input x; the evaluating kernels read L after their fill.  (The statements keep the order
// iir_rows_tile had them in: moved, they change its schedule and registers -- tools/kernel_cmp.py.)
// IRW_OUT_T: the element of `out` -- T, unless the kernel has said otherwise (wfk_iir_rows_dac.hip: int16_t codes).
#ifndef IRW_OUT_T
#define IRW_OUT_T T
#endif
  constexpr int D = NSEC * ORD, NC = NSEC * (ORD + 1), MM = D * D * 2;
  __shared__ T tile[IRW_THREADS * IRW_PITCH];
  __shared__ double s_tot[IRW_WAVES][D];
  __shared__ double s_carry[2][D];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row = blockIdx.x;
  const double* rt = tab + row * (int64_t)irw_row_doubles(NSEC, ORD);   // workgroup-uniform: scalar loads
  double cb[NC], ca[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) { cb[i] = rt[i]; ca[i] = rt[NC + i]; }
  const auto B = [&](int s, int i) { return cb[s * (ORD + 1) + i]; };
  const auto A = [&](int s, int i) { return ca[s * (ORD + 1) + i]; };
  const double* pw = rt + 2 * NC;
  const double* W = pw + (IRW_NPW - 1) * MM;                            // T^64
#ifdef IRW_LOADS_INPUT
  double L[MM];                                                         // T^lane, kept for the whole row
#pragma unroll
  for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
#endif
  const double pre = initial ? initial[row] : 0.0;
  if (tid < D) s_carry[0][tid] = zi ? zi[row * D + tid] : 0.0;
#ifdef IRW_LOADS_INPUT
  const T* x = in + row * in_stride;
#endif
  IRW_OUT_T* y = out + row * out_stride;
  const int64_t ntile = (n + IRW_TILE - 1) / IRW_TILE;
  T* const my = tile + tid * IRW_PITCH;
