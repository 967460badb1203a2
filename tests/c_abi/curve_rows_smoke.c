/* Plain-C consumer of the curve stage declarations of include/wfk.h, on the device: the argument checks, then two rows
 * of 8 doubles -- a 3-knot and a 2-knot curve; samples at knots, between them, beyond both ends, an inf and a NaN --
 * through wfk_curve_rows_apply out of place with strided rows and in place, compared value by value and count by count
 * with its own loop.  Prints "16 values interpolated on the device, parity ok". */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wfk.h"

#define N 8
#define ROWS 2
#define IN_STRIDE 11
#define OUT_STRIDE 9

static double curve(double x, const double* xp, const double* fp, int k, double left, double right, int64_t* counts) {
  int j = 0;
  if (x != x) { ++counts[2]; return x; }
  if (x < xp[0]) { ++counts[0]; return left; }
  if (x > xp[k - 1]) { ++counts[1]; return right; }
  while (j + 1 < k && xp[j + 1] <= x) ++j;
  if (x == xp[j]) return fp[j];
  {
    volatile double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    volatile double prod = slope * (x - xp[j]);                    /* rounded before the sum: no fused multiply-add */
    return prod + fp[j];
  }
}

int main(void) {
  static double x[ROWS * IN_STRIDE], y[ROWS * OUT_STRIDE], z[ROWS * IN_STRIDE];
  static int64_t counts[ROWS * 3], want_counts[ROWS * 3];
  const int64_t knot_ptr[ROWS + 1] = {0, 3, 5}, bad_ptr[ROWS + 1] = {0, 1, 5}, late_ptr[ROWS + 1] = {1, 3, 5};
  const double xp[5] = {-1.0, 0.25, 2.0, 0.0, 10.0}, fp[5] = {0.3, -0.7, 1.9, 5.0, -5.0};
  const double flat[5] = {-1.0, 0.25, 0.25, 0.0, 10.0}, nanf_[5] = {0.3, -0.7, 1.9, NAN, -5.0};
  const double left[ROWS] = {-100.0, 7.5}, right[ROWS] = {100.0, NAN};
  const double row0[N] = {-1.0, 0.25, 2.0, 0.1, 1.7, -1.5, INFINITY, -0.3};
  const double row1[N] = {0.0, 10.0, 3.3, NAN, -0.0, 11.0, -INFINITY, 9.99};
  wfk_curve_rows_plan* plan = NULL;
  void *xd = NULL, *yd = NULL, *cd = NULL;
  int r, i;

  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, bad_ptr, xp, fp, left, right, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 0: fewer than 2 knots")) return 2;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, knot_ptr, flat, fp, left, right, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "row 0: knots are not strictly increasing at 2")) return 4;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, knot_ptr, xp, nanf_, left, right, &plan) != WFK_EINVAL) return 5;
  if (!strstr(wfk_last_error(), "row 1: value 0 is not finite")) return 6;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, late_ptr, xp, fp, left, right, &plan) != WFK_EINVAL) return 7;
  if (wfk_curve_rows_plan_create(-1, ROWS, WFK_OUT_F64, knot_ptr, xp, fp, left, right, &plan) != WFK_EINVAL) return 8;
  if (wfk_curve_rows_plan_create(N, 0, WFK_OUT_F64, knot_ptr, xp, fp, left, right, &plan) != WFK_EINVAL) return 9;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_C128, knot_ptr, xp, fp, left, right, &plan) != WFK_EINVAL) return 10;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, NULL, xp, fp, left, right, &plan) != WFK_EINVAL) return 11;
  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, knot_ptr, xp, fp, left, right, NULL) != WFK_EINVAL) return 12;
  if (wfk_curve_rows_apply(NULL, NULL, N, NULL, N, NULL, NULL) != WFK_EINVAL) return 13;
  if (wfk_curve_rows_plan_destroy(NULL) != WFK_OK || strcmp(wfk_curve_rows_kernel_name(NULL, 0), "") != 0) return 14;
  if (WFK_CURVE_MAX_KNOTS != 1024 || wfk_abi_version() != 2) return 15;

  if (wfk_curve_rows_plan_create(N, ROWS, WFK_OUT_F64, knot_ptr, xp, fp, left, right, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 16;
  }
  if (strcmp(wfk_curve_rows_kernel_name(plan, 0), "curve_rows<double>") != 0) return 17;
  if (strcmp(wfk_curve_rows_kernel_name(plan, 1), "curve_rows_counts<double>") != 0) return 18;
  if (wfk_curve_rows_spans(plan) != 1) return 19;
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = 0.5;
  for (i = 0; i < N; ++i) {
    x[i] = row0[i];
    x[IN_STRIDE + i] = row1[i];
  }
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) y[i] = -5.0;
  for (i = 0; i < ROWS * 3; ++i) counts[i] = 0x5a5a5a5a5a5aLL;              /* garbage: the apply overwrites it */
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK)
    return 20;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK ||
      wfk_memcpy_h2d(cd, counts, sizeof counts) != WFK_OK)
    return 21;
  /* exactly in place or disjoint; strides; the counts may meet neither side */
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, (double*)xd + 1, IN_STRIDE, NULL, NULL) != WFK_EINVAL) return 22;
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, xd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 23;
  if (wfk_curve_rows_apply(plan, xd, N - 1, yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 24;
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, yd, N - 1, NULL, NULL) != WFK_EINVAL) return 25;
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, yd, OUT_STRIDE, (int64_t*)xd, NULL) != WFK_EINVAL) return 26;
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, yd, OUT_STRIDE, (int64_t*)yd, NULL) != WFK_EINVAL) return 27;
  if (wfk_curve_rows_apply(plan, (char*)xd + 4, IN_STRIDE, yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 28;
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, yd, OUT_STRIDE, (int64_t*)cd, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 29;
  }
  if (wfk_curve_rows_apply(plan, xd, IN_STRIDE, xd, IN_STRIDE, NULL, NULL) != WFK_OK) return 30;      /* in place */
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(z, xd, sizeof z) != WFK_OK || wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 31;
  memset(want_counts, 0, sizeof want_counts);
  for (r = 0; r < ROWS; ++r) {
    for (i = 0; i < N; ++i) {
      const double want = curve(x[r * IN_STRIDE + i], xp + knot_ptr[r], fp + knot_ptr[r],
                                (int)(knot_ptr[r + 1] - knot_ptr[r]), left[r], right[r], want_counts + 3 * r);
      const double got = y[r * OUT_STRIDE + i], again = z[r * IN_STRIDE + i];
      if (want != want ? !(got != got && again != again)
                       : (memcmp(&got, &want, sizeof want) != 0 || memcmp(&again, &want, sizeof want) != 0)) {
        fprintf(stderr, "row %d sample %d: got %.17g / %.17g, want %.17g\n", r, i, got, again, want);
        return 32;
      }
    }
    for (i = N; i < OUT_STRIDE; ++i)
      if (y[r * OUT_STRIDE + i] != -5.0) return 33;              /* past a row: untouched */
    for (i = N; i < IN_STRIDE; ++i)
      if (z[r * IN_STRIDE + i] != 0.5) return 34;
  }
  for (i = 0; i < ROWS * 3; ++i)
    if (counts[i] != want_counts[i]) {
      fprintf(stderr, "count %d: got %lld, want %lld\n", i, (long long)counts[i], (long long)want_counts[i]);
      return 35;
    }
  if (want_counts[0] != 1 || want_counts[1] != 1 || want_counts[2] != 0 || want_counts[3] != 1 || want_counts[4] != 1 ||
      want_counts[5] != 1)
    return 36;
  if (y[0] != 0.3 || y[1] != -0.7 || y[2] != 1.9 || y[5] != -100.0 || y[6] != 100.0 || y[OUT_STRIDE + 6] != 7.5) return 37;
  wfk_curve_rows_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  wfk_free(cd);
  printf("16 values interpolated on the device, parity ok\n");
  return 0;
}
