/* Plain-C consumer of the DAC stage declarations of include/wfk.h, on the device: the argument checks, then four rows
 * of 1000 doubles (an I/Q pair inside the rails, a pair driven past both rails with an inf and a NaN in it) through
 * wfk_dac_rows_apply with strided rows, 14 bits left-justified, pairs interleaved, compared code by code and count
 * by count with its own loop.  Prints "quantised on the device, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 1000
#define ROWS 4
#define K 2
#define BITS 14
#define SHIFT 2
#define IN_STRIDE 1003
#define OUT_STRIDE (K * N + 11)

int main(void) {
  static double x[ROWS * IN_STRIDE];
  static int16_t y[(ROWS / K) * OUT_STRIDE];
  static int64_t counts[ROWS * 3], want_counts[ROWS * 3];
  const double gain[ROWS] = {8191.0, -8191.0, 9731.37, 4000.5};
  const double offset[ROWS] = {0.0, 12.5, -300.0, 7.0};
  const double bad_nan[ROWS] = {8191.0, NAN, 1.0, 1.0}, bad_inf[ROWS] = {0.0, 0.0, INFINITY, 0.0};
  const double lo = -8192.0, hi = 8191.0;
  wfk_dac_rows_plan* plan = NULL;
  void *xd = NULL, *yd = NULL, *cd = NULL;
  int r, i;

  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, bad_nan, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 1")) return 2;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, bad_inf, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "row 2")) return 4;
  if (wfk_dac_rows_plan_create(-1, ROWS, WFK_OUT_F64, gain, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 5;
  if (wfk_dac_rows_plan_create(N, 0, WFK_OUT_F64, gain, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 6;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_C128, gain, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 7;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, 1, 0, K, &plan) != WFK_EINVAL) return 8;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, 17, 0, K, &plan) != WFK_EINVAL) return 9;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, BITS, 3, K, &plan) != WFK_EINVAL) return 10;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, BITS, SHIFT, 3, &plan) != WFK_EINVAL) return 11;
  if (wfk_dac_rows_plan_create(N, 3, WFK_OUT_F64, gain, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 12;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, NULL, offset, BITS, SHIFT, K, &plan) != WFK_EINVAL) return 13;
  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, BITS, SHIFT, K, NULL) != WFK_EINVAL) return 14;
  if (wfk_dac_rows_apply(NULL, NULL, N, NULL, N, NULL, NULL) != WFK_EINVAL) return 15;
  if (wfk_dac_rows_plan_destroy(NULL) != WFK_OK) return 16;

  if (wfk_dac_rows_plan_create(N, ROWS, WFK_OUT_F64, gain, offset, BITS, SHIFT, K, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 17;
  }
  if (strcmp(wfk_dac_rows_kernel_name(plan, 0), "dac_rows<double>") != 0) return 18;
  if (strcmp(wfk_dac_rows_kernel_name(plan, 1), "dac_rows_count<double>") != 0) return 19;
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = 0.9 * sin(0.37 * i) + 1e-3 * (i % 17);
  for (i = 0; i < N; ++i) {                            /* rows 2 and 3 overshoot */
    x[2 * IN_STRIDE + i] *= 1.4;
    x[3 * IN_STRIDE + i] = 3.0 * cos(0.11 * i);
  }
  x[2 * IN_STRIDE + 17] = INFINITY;
  x[2 * IN_STRIDE + 18] = -INFINITY;
  x[3 * IN_STRIDE + 500] = NAN;
  for (i = 0; i < (ROWS / K) * OUT_STRIDE; ++i) y[i] = -5;
  for (i = 0; i < ROWS * 3; ++i) counts[i] = 0x5a5a5a5a5a5aLL;              /* garbage: the apply overwrites it */
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK)
    return 20;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK ||
      wfk_memcpy_h2d(cd, counts, sizeof counts) != WFK_OK)
    return 21;
  /* out of place only; strides; the counts may meet neither side */
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)xd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 22;
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)xd + 4 * (ROWS - 1) * IN_STRIDE, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 23;
  if (wfk_dac_rows_apply(plan, xd, N - 1, (int16_t*)yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 24;
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)yd, K * N - 1, NULL, NULL) != WFK_EINVAL) return 25;
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)xd, NULL) != WFK_EINVAL) return 26;
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)yd, NULL) != WFK_EINVAL) return 27;
  if (wfk_dac_rows_apply(plan, (char*)xd + 4, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 28;
  if (wfk_dac_rows_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)cd, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 29;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 30;
  memset(want_counts, 0, sizeof want_counts);
  for (r = 0; r < ROWS; ++r) {
    for (i = 0; i < N; ++i) {
      volatile double prod = x[r * IN_STRIDE + i] * gain[r];     /* rounded before the sum: no fused multiply-add */
      const double v = prod + offset[r];
      const double q = rint(v);                                  /* half to even in the default rounding mode */
      double c = q;
      if (v != v) { c = 0.0; ++want_counts[r * 3 + 2]; }
      else if (q < lo) { c = lo; ++want_counts[r * 3 + 0]; }
      else if (q > hi) { c = hi; ++want_counts[r * 3 + 1]; }
      {
        const int16_t want = (int16_t)((int)c * (1 << SHIFT));
        const int16_t got = y[(r / K) * OUT_STRIDE + i * K + r % K];
        if (got != want) {
          fprintf(stderr, "row %d sample %d: got %d, want %d\n", r, i, got, want);
          return 31;
        }
      }
    }
  }
  for (r = 0; r < ROWS / K; ++r)
    for (i = K * N; i < OUT_STRIDE; ++i)
      if (y[r * OUT_STRIDE + i] != -5) return 32;                /* past a row: untouched */
  for (i = 0; i < ROWS * 3; ++i)
    if (counts[i] != want_counts[i]) {
      fprintf(stderr, "count %d: got %lld, want %lld\n", i, (long long)counts[i], (long long)want_counts[i]);
      return 33;
    }
  if (want_counts[6] + want_counts[7] < 10 || want_counts[11] != 1 || want_counts[0] + want_counts[1] != 0) return 34;
  wfk_dac_rows_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  wfk_free(cd);
  printf("quantised on the device, parity ok\n");
  return 0;
}
