/* Plain-C consumer of the per-row shift declarations of include/wfk.h, on the device: the argument checks, then three
 * rows of 1000 doubles (a fractional delay, a whole-sample advance, a row pushed out altogether) through
 * wfk_shift_rows_apply with strided rows, compared sample by sample with the closed form.  Prints
 * "shifted on the device, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 1000
#define ROWS 3
#define IN_STRIDE 1003
#define OUT_STRIDE 1011

int main(void) {
  static double x[ROWS * IN_STRIDE], y[ROWS * OUT_STRIDE];
  const int64_t points[ROWS] = {7, -130, 1000};
  const double delta[ROWS] = {0.375, 0.0, 0.5};
  const double bad_hi[ROWS] = {0.375, 1.5, 0.5}, bad_nan[ROWS] = {0.375, 0.0, NAN};
  wfk_shift_rows_plan* plan = NULL;
  void *xd = NULL, *yd = NULL;
  int r, i;

  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, points, bad_hi, &plan) != WFK_EINVAL || plan) return 1;
  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, points, bad_nan, &plan) != WFK_EINVAL) return 2;
  if (wfk_shift_rows_plan_create(-1, ROWS, WFK_OUT_F64, points, delta, &plan) != WFK_EINVAL) return 3;
  if (wfk_shift_rows_plan_create(N, 0, WFK_OUT_F64, points, delta, &plan) != WFK_EINVAL) return 4;
  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_C128, points, delta, &plan) != WFK_EINVAL) return 5;
  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, NULL, delta, &plan) != WFK_EINVAL) return 6;
  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, points, NULL, &plan) != WFK_EINVAL) return 7;
  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, points, delta, NULL) != WFK_EINVAL) return 8;
  if (wfk_shift_rows_apply(NULL, NULL, N, NULL, N, NULL) != WFK_EINVAL) return 9;
  if (wfk_shift_rows_plan_destroy(NULL) != WFK_OK) return 10;

  if (wfk_shift_rows_plan_create(N, ROWS, WFK_OUT_F64, points, delta, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 11;
  }
  if (strcmp(wfk_shift_rows_kernel_name(plan), "shift_rows<double>") != 0) return 12;
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = sin(0.37 * i) + 1e-3 * (i % 17);
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) y[i] = -5.0;
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK) return 13;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK) return 14;
  /* out of place only: the same rows, and rows that overlap, are refused */
  if (wfk_shift_rows_apply(plan, xd, IN_STRIDE, xd, IN_STRIDE, NULL) != WFK_EINVAL) return 15;
  if (wfk_shift_rows_apply(plan, xd, IN_STRIDE, (double*)xd + 500, IN_STRIDE, NULL) != WFK_EINVAL) return 16;
  if (wfk_shift_rows_apply(plan, xd, N - 1, yd, OUT_STRIDE, NULL) != WFK_EINVAL) return 17;
  if (wfk_shift_rows_apply(plan, xd, IN_STRIDE, yd, OUT_STRIDE, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 18;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK) return 19;
  for (r = 0; r < ROWS; ++r) {
    const double* xr = x + r * IN_STRIDE;
    for (i = 0; i < OUT_STRIDE; ++i) {
      const double got = y[r * OUT_STRIDE + i];
      const int64_t j = i - points[r];
      double want = -5.0, tol = 0.0;                 /* past the row: untouched */
      if (i < N) {
        want = 0.0;                                  /* zero fill */
        if (j >= 0 && j < N) {
          const double prev = j >= 1 ? xr[j - 1] : 0.0;
          want = delta[r] > 0 ? (1 - delta[r]) * xr[j] + delta[r] * prev : xr[j];
          tol = delta[r] > 0 ? 4 * 0x1p-53 * ((1 - delta[r]) * fabs(xr[j]) + delta[r] * fabs(prev)) : 0.0;
        }
      }
      if (!(fabs(got - want) <= tol)) {
        fprintf(stderr, "row %d sample %d: got %.17g, want %.17g\n", r, i, got, want);
        return 20;
      }
    }
  }
  wfk_shift_rows_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  printf("shifted on the device, parity ok\n");
  return 0;
}
