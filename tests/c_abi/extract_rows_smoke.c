/* Plain-C consumer of the per-row kernel extraction declarations of include/wfk.h, on the device: the argument
 * checks, then three rows of 64 doubles whose sig_out is a known circular filter of sig_in,
 *   sig_out[i] = sig_in[i] + q sig_in[i - 1 mod n],
 * so that the extracted kernel is the filter's inverse in closed form, c[d] = (-q)^d / (1 - (-q)^n), rotated to the
 * centre and cropped: compared sample by sample, with strided rows, with and without a shared sig_in, and with three
 * smoothing taps against the same closed form convolved on the host.  Prints
 * "kernels extracted on the device, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 64
#define ROWS 3
#define SKIP 5
#define K (N - 2 * SKIP)
#define IN_STRIDE 67
#define OUT_STRIDE 71
#define KER_STRIDE 59

static const double q_of[ROWS] = {0.5, -0.25, 0.125};
static const double taps[3] = {0.25, 0.5, 0.25};

/* s[i] = c[(i + N/2) mod N], c[d] = (-q)^d / (1 - (-q)^N) */
static double centred(double q, int i) { return pow(-q, (i + N / 2) % N) / (1.0 - pow(-q, N)); }

static double smoothed(double q, int i) {                 /* 'same' with three taps: centre (3 - 1) / 2 = 1 */
  double t = 0.0;
  int m;
  for (m = 0; m < 3; ++m) {
    const int k = i + 1 - m;
    if (k >= 0 && k < N) t += taps[m] * centred(q, k);
  }
  return t;
}

static int compare(const double* ker, int shared, int smooth) {
  int r, j;
  for (r = 0; r < ROWS; ++r)
    for (j = 0; j < KER_STRIDE; ++j) {
      const double got = ker[r * KER_STRIDE + j];
      double want = -5.0, tol = 0.0;                      /* past the row: untouched */
      if (j < K) {
        want = smooth ? smoothed(q_of[r], j + SKIP) : centred(q_of[r], j + SKIP);
        tol = 1e-12 * (1.0 / (1.0 - fabs(q_of[r])));      /* 1e-12 of the scale (c[0] is ~1; the sum bounds it) */
      }
      if (!(fabs(got - want) <= tol)) {
        fprintf(stderr, "shared %d smooth %d row %d sample %d: got %.17g, want %.17g\n", shared, smooth, r, j, got, want);
        return 1;
      }
    }
  return 0;
}

int main(void) {
  static double a[ROWS * IN_STRIDE], b[ROWS * OUT_STRIDE], bs[ROWS * OUT_STRIDE], ker[ROWS * KER_STRIDE];
  const double bad_tap[3] = {0.25, NAN, 0.25};
  wfk_extract_rows_plan *plan = NULL, *shared = NULL, *smooth = NULL;
  void *ad = NULL, *bd = NULL, *bsd = NULL, *kd = NULL;
  int r, i;

  if (wfk_extract_rows_plan_create(0, ROWS, ROWS, NULL, 0, 0, &plan) != WFK_EINVAL || plan) return 1;
  if (wfk_extract_rows_plan_create(N, 0, 0, NULL, 0, 0, &plan) != WFK_EINVAL) return 2;
  if (wfk_extract_rows_plan_create(N, ROWS, 2, NULL, 0, 0, &plan) != WFK_EINVAL) return 3;
  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, NULL, 0, -1, &plan) != WFK_EINVAL) return 4;
  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, taps, -1, 0, &plan) != WFK_EINVAL) return 5;
  if (wfk_extract_rows_plan_create(2, ROWS, ROWS, taps, 3, 0, &plan) != WFK_EINVAL) return 6;      /* n_taps > n */
  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, bad_tap, 3, 0, &plan) != WFK_EINVAL) return 7;
  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, NULL, 3, 0, &plan) != WFK_EINVAL) return 8;
  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, NULL, 0, 0, NULL) != WFK_EINVAL) return 9;
  if (wfk_extract_rows_apply(NULL, NULL, N, NULL, N, NULL, N, NULL) != WFK_EINVAL) return 10;
  if (wfk_extract_rows_plan_destroy(NULL) != WFK_OK) return 11;
  if (strcmp(wfk_extract_rows_kernel_name(NULL), "") != 0) return 12;

  if (wfk_extract_rows_plan_create(N, ROWS, ROWS, NULL, 0, SKIP, &plan) != WFK_OK ||
      wfk_extract_rows_plan_create(N, ROWS, 1, NULL, 0, SKIP, &shared) != WFK_OK ||
      wfk_extract_rows_plan_create(N, ROWS, ROWS, taps, 3, SKIP, &smooth) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 13;
  }
  if (strcmp(wfk_extract_rows_kernel_name(plan), "extract_ratio + extract_smooth") != 0) return 14;
  for (i = 0; i < ROWS * IN_STRIDE; ++i) a[i] = -7.0;
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) b[i] = bs[i] = 9.0;
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < N; ++i) a[r * IN_STRIDE + i] = sin(0.37 * i + r) + 1e-3 * ((i * 7 + r) % 17) + (i == 3 * r);
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < N; ++i) {
      b[r * OUT_STRIDE + i] = a[r * IN_STRIDE + i] + q_of[r] * a[r * IN_STRIDE + (i + N - 1) % N];
      bs[r * OUT_STRIDE + i] = a[i] + q_of[r] * a[(i + N - 1) % N];                 /* all rows from row 0 of a */
    }
  for (i = 0; i < ROWS * KER_STRIDE; ++i) ker[i] = -5.0;
  if (wfk_malloc(&ad, sizeof a) != WFK_OK || wfk_malloc(&bd, sizeof b) != WFK_OK ||
      wfk_malloc(&bsd, sizeof bs) != WFK_OK || wfk_malloc(&kd, sizeof ker) != WFK_OK)
    return 15;
  if (wfk_memcpy_h2d(ad, a, sizeof a) != WFK_OK || wfk_memcpy_h2d(bd, b, sizeof b) != WFK_OK ||
      wfk_memcpy_h2d(bsd, bs, sizeof bs) != WFK_OK || wfk_memcpy_h2d(kd, ker, sizeof ker) != WFK_OK)
    return 16;
  /* the result may overlap neither input; strides below the row are refused */
  if (wfk_extract_rows_apply(plan, ad, IN_STRIDE, bd, OUT_STRIDE, ad, IN_STRIDE, NULL) != WFK_EINVAL) return 17;
  if (wfk_extract_rows_apply(plan, ad, IN_STRIDE, bd, OUT_STRIDE, (double*)bd + 100, KER_STRIDE, NULL) != WFK_EINVAL)
    return 18;
  if (wfk_extract_rows_apply(plan, ad, N - 1, bd, OUT_STRIDE, kd, KER_STRIDE, NULL) != WFK_EINVAL) return 19;
  if (wfk_extract_rows_apply(plan, ad, IN_STRIDE, bd, N - 1, kd, KER_STRIDE, NULL) != WFK_EINVAL) return 20;
  if (wfk_extract_rows_apply(plan, ad, IN_STRIDE, bd, OUT_STRIDE, kd, K - 1, NULL) != WFK_EINVAL) return 21;
  if (wfk_extract_rows_apply(plan, NULL, IN_STRIDE, bd, OUT_STRIDE, kd, KER_STRIDE, NULL) != WFK_EINVAL) return 22;

  if (wfk_extract_rows_apply(plan, ad, IN_STRIDE, bd, OUT_STRIDE, kd, KER_STRIDE, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 23;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(ker, kd, sizeof ker) != WFK_OK) return 24;
  if (compare(ker, 0, 0)) return 25;
  if (wfk_extract_rows_apply(shared, ad, IN_STRIDE, bsd, OUT_STRIDE, kd, KER_STRIDE, NULL) != WFK_OK) return 26;
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(ker, kd, sizeof ker) != WFK_OK) return 27;
  if (compare(ker, 1, 0)) return 28;
  if (wfk_extract_rows_apply(smooth, ad, IN_STRIDE, bd, OUT_STRIDE, kd, KER_STRIDE, NULL) != WFK_OK) return 29;
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(ker, kd, sizeof ker) != WFK_OK) return 30;
  if (compare(ker, 0, 1)) return 31;
  wfk_extract_rows_plan_destroy(plan);
  wfk_extract_rows_plan_destroy(shared);
  wfk_extract_rows_plan_destroy(smooth);
  wfk_free(ad);
  wfk_free(bd);
  wfk_free(bsd);
  wfk_free(kd);
  printf("kernels extracted on the device, parity ok\n");
  return 0;
}
