/* Plain-C consumer of the per-row curve -> IIR -> DAC codes declarations of include/wfk.h, on the device: the argument
 * checks, then three rows of 5000 doubles (two tiles: its own curve of 2, 3 or 5 knots, one section of order 2, its own
 * gain, offset and level per row) through wfk_curve_iir_dac_apply with strided rows, 14 bits left-justified, compared
 * with its own scalar loop (the piecewise-linear lookup, direct form II transposed, then the converter's statements);
 * the curve's report `beyond` is exact.  The device filter is held to 1e-9 of the loop's, so a code is compared
 * where the loop's v is at least 1e-4 LSB (the largest gain, 29731, times 1e-9, three times over) from a half-integer -- all but a few samples -- and
 * may differ by one step elsewhere; a count may differ by the number of such samples.  Prints
 * "curve and filter to codes on the device, <n> codes ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 5000
#define ROWS 3
#define ORD 2
#define BITS 14
#define SHIFT 2
#define IN_STRIDE 5003
#define OUT_STRIDE (N + 11)

int main(void) {
  static double x[ROWS * IN_STRIDE];
  static int16_t y[ROWS * OUT_STRIDE];
  static int64_t counts[ROWS * 3], want_counts[ROWS * 3], beyond[ROWS * 3], want_beyond[ROWS * 3];
  double zf[ROWS * ORD];
  const int32_t orders[1] = {ORD};
  /* a[0] != 1 in row 1: the library normalises */
  const double b[ROWS * (ORD + 1)] = {0.3, 0.2, -0.1, 0.5, -0.4, 0.2, 1.0, -0.9, 0.1};
  const double a[ROWS * (ORD + 1)] = {1.0, -1.1, 0.3, 2.0, -1.0, 0.25, 1.0, 0.2, -0.35};
  const double gain[ROWS] = {8191.0, -6000.5, 29731.37};
  const double offset[ROWS] = {0.25, 12.5, -300.75};
  const double level[ROWS] = {0.0, 0.125, -0.25};
  /* the curves, CSR-like: 2, 3 and 5 knots; row 1 descends; right given (row 2: beyond its last knot a sample becomes 0.9) */
  const int64_t kp[ROWS + 1] = {0, 2, 5, 10};
  const double xp[10] = {-0.8, 0.9, -1.0, 0.1, 0.7, -0.9, -0.3, 0.0, 0.25, 0.85};
  const double fp[10] = {-0.6, 0.7, 0.8, 0.05, -0.5, -0.7, -0.1, 0.1, 0.2, 0.75};
  const double right[ROWS] = {0.7, -0.5, 0.9};
  const int64_t bad_kp[ROWS + 1] = {0, 1, 5, 10};
  const double bad_nan[ROWS] = {8191.0, NAN, 1.0};
  const double lo = -8192.0, hi = 8191.0;
  wfk_curve_iir_dac_plan* plan = NULL;
  void *xd = NULL, *yd = NULL, *cd = NULL, *bd = NULL, *zd = NULL, *ld = NULL;
  long compared = 0, loose = 0;
  int r, i, j;

  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, bad_nan, offset, BITS, SHIFT, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 1: gain")) return 2;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, gain, offset, 17, 0, &plan) != WFK_EINVAL) return 3;
  /* the curve's refusal comes before the converter's */
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, bad_kp, xp, fp, NULL, right, bad_nan, offset, 17, 0, &plan) != WFK_EINVAL) return 34;
  if (!strstr(wfk_last_error(), "row 0: fewer than 2 knots")) return 35;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, gain, offset, BITS, 3, &plan) != WFK_EINVAL) return 4;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, NULL, offset, BITS, SHIFT, &plan) != WFK_EINVAL) return 5;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, -1, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, gain, offset, BITS, SHIFT, &plan) != WFK_EINVAL) return 6;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_C128, kp, xp, fp, NULL, right, gain, offset, BITS, SHIFT, &plan) != WFK_EINVAL) return 7;
  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, gain, offset, BITS, SHIFT, NULL) != WFK_EINVAL) return 8;
  if (wfk_curve_iir_dac_apply(NULL, NULL, N, NULL, N, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 9;
  if (wfk_curve_iir_dac_plan_destroy(NULL) != WFK_OK) return 10;

  if (wfk_curve_iir_dac_plan_create(1, orders, b, a, N, ROWS, WFK_OUT_F64, kp, xp, fp, NULL, right, gain, offset, BITS, SHIFT, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 11;
  }
  if (strcmp(wfk_curve_iir_dac_kernel_name(plan), "iir_rows_curve_dac<f64,1,2>") != 0) return 12;
  if (wfk_curve_iir_dac_state_dim(plan) != ORD) return 13;
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = 0.7 * sin(0.37 * i) + 0.35 * cos(0.011 * i) + 1e-3 * (i % 17);
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) y[i] = -5;
  for (i = 0; i < ROWS * 3; ++i) counts[i] = beyond[i] = 0x5a5a5a5a5a5aLL;    /* garbage: the apply overwrites it */
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK ||
      wfk_malloc(&bd, sizeof beyond) != WFK_OK ||
      wfk_malloc(&zd, sizeof zf) != WFK_OK || wfk_malloc(&ld, sizeof level) != WFK_OK)
    return 14;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK ||
      wfk_memcpy_h2d(cd, counts, sizeof counts) != WFK_OK || wfk_memcpy_h2d(bd, beyond, sizeof beyond) != WFK_OK || wfk_memcpy_h2d(ld, level, sizeof level) != WFK_OK)
    return 15;
  /* out of place only; strides; the counts may meet neither side */
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)xd, OUT_STRIDE, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 16;
  if (wfk_curve_iir_dac_apply(plan, xd, N - 1, (int16_t*)yd, OUT_STRIDE, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 17;
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, N - 1, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 18;
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)xd, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 19;
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)yd, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 20;
  /* the second report: apart from both sides and from the first */
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, NULL, (int64_t*)yd, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 31;
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)cd, (int64_t*)cd + 1, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 32;
  if (!strstr(wfk_last_error(), "beyond overlaps counts")) return 33;
  if (wfk_curve_iir_dac_apply(plan, (char*)xd + 4, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 21;
  if (wfk_curve_iir_dac_apply_shared_in(plan, xd, (int16_t*)xd + 8, OUT_STRIDE, NULL, NULL, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 22;
  if (wfk_curve_iir_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)cd, (int64_t*)bd, NULL, (double*)zd,
                              (const double*)ld, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 23;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK || wfk_memcpy_d2h(beyond, bd, sizeof beyond) != WFK_OK || wfk_memcpy_d2h(zf, zd, sizeof zf) != WFK_OK)
    return 24;
  memset(want_counts, 0, sizeof want_counts);
  memset(want_beyond, 0, sizeof want_beyond);
  for (r = 0; r < ROWS; ++r) {
    const double *br = b + r * (ORD + 1), *ar = a + r * (ORD + 1);
    const double b0 = br[0] / ar[0], b1 = br[1] / ar[0], b2 = br[2] / ar[0], a1 = ar[1] / ar[0], a2 = ar[2] / ar[0];
    double z0 = 0.0, z1 = 0.0;
    long row_loose = 0;
    for (i = 0; i < N; ++i) {
      const double s = x[r * IN_STRIDE + i];
      const double *kx = xp + kp[r], *kf = fp + kp[r];
      const int K = (int)(kp[r + 1] - kp[r]);
      double volts, u;
      if (s < kx[0]) { volts = kf[0]; ++want_beyond[r * 3 + 0]; }
      else if (s > kx[K - 1]) { volts = right[r]; ++want_beyond[r * 3 + 1]; }
      else {
        for (j = K - 1; kx[j] > s; --j) {}
        if (s == kx[j]) volts = kf[j];
        else {
          volatile double slope = (kf[j + 1] - kf[j]) / (kx[j + 1] - kx[j]);
          volatile double prod = slope * (s - kx[j]);              /* rounded before the sum: no fused multiply-add */
          volts = prod + kf[j];
        }
      }
      u = volts - level[r];
      const double f = b0 * u + z0;
      z0 = b1 * u - a1 * f + z1;
      z1 = b2 * u - a2 * f;
      {
        volatile double prod = (f + level[r]) * gain[r];           /* rounded before the sum: no fused multiply-add */
        const double v = prod + offset[r];
        const double q = rint(v);                                  /* half to even in the default rounding mode */
        const int decided = fabs(v - floor(v) - 0.5) > 1e-4;
        double c = q;
        if (q < lo) { c = lo; ++want_counts[r * 3 + 0]; }
        else if (q > hi) { c = hi; ++want_counts[r * 3 + 1]; }
        {
          const int want = (int)c * (1 << SHIFT), got = y[r * OUT_STRIDE + i];
          if (decided ? got != want : abs(got - want) > (1 << SHIFT)) {
            fprintf(stderr, "row %d sample %d: got %d, want %d (v = %.17g)\n", r, i, got, want, v);
            return 25;
          }
          compared += decided;
          row_loose += !decided;
        }
      }
    }
    for (i = N; i < OUT_STRIDE; ++i)
      if (y[r * OUT_STRIDE + i] != -5) return 26;                  /* past a row: untouched */
    for (i = 0; i < 3; ++i)
      if (beyond[r * 3 + i] != want_beyond[r * 3 + i]) {
        fprintf(stderr, "row %d beyond %d: got %lld, want %lld\n", r, i, (long long)beyond[r * 3 + i],
                (long long)want_beyond[r * 3 + i]);
        return 36;
      }
    if (want_beyond[r * 3] < 10 || want_beyond[r * 3 + 1] < 10) return 37;   /* every row leaves its curve on both sides */
    for (i = 0; i < 3; ++i)
      if (llabs((long long)(counts[r * 3 + i] - want_counts[r * 3 + i])) > (i < 2 ? row_loose : 0)) {
        fprintf(stderr, "row %d count %d: got %lld, want %lld\n", r, i, (long long)counts[r * 3 + i],
                (long long)want_counts[r * 3 + i]);
        return 27;
      }
    if (fabs(zf[r * ORD] - z0) > 1e-9 * fmax(1.0, fabs(z0)) || fabs(zf[r * ORD + 1] - z1) > 1e-9 * fmax(1.0, fabs(z1))) {
      fprintf(stderr, "row %d zf: got %.17g %.17g, want %.17g %.17g\n", r, zf[r * ORD], zf[r * ORD + 1], z0, z1);
      return 28;
    }
    loose += row_loose;
  }
  if (loose * 1000 > (long)ROWS * N) return 29;                    /* all but a few samples are compared exactly */
  if (want_counts[0] + want_counts[1] < 10 || want_counts[6] + want_counts[7] < 10) return 30;   /* rows 0 and 2 clip */
  wfk_curve_iir_dac_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  wfk_free(cd);
  wfk_free(bd);
  wfk_free(zd);
  wfk_free(ld);
  printf("curve and filter to codes on the device, %ld codes ok\n", compared);
  return 0;
}
