/* Plain-C consumer of the mix stage declarations of include/wfk.h, on the device: the argument checks, then two I/Q
 * pairs of 4 doubles (strided rows) through a 4 x 4 plan of two 2 x 2 blocks with DC offsets, one of the stored
 * coefficients a zero (not a term), and the 16 results against constants computed by hand -- every number here is a
 * small binary fraction, so the products and sums are exact.  Prints "mixed on the device, 16 values ok". */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wfk.h"

#define N 4
#define ROWS 4
#define IN_STRIDE 7
#define OUT_STRIDE 5

int main(void) {
  /* pair 0: [[1, 0.5], [-0.25, 2]] + [0.125, -1];   pair 1: [[2, 0], [0.5, -1]] + [0, 0.25] */
  const int64_t row_ptr[ROWS + 1] = {0, 2, 4, 6, 8};
  const int32_t col[8] = {0, 1, 0, 1, 2, 3, 2, 3};
  const double val[8] = {1.0, 0.5, -0.25, 2.0, 2.0, 0.0, 0.5, -1.0};
  const double offset[ROWS] = {0.125, -1.0, 0.0, 0.25};
  const double rows[ROWS][N] = {{1.0, 2.0, 3.0, 4.0}, {0.5, -0.5, 1.5, -1.5}, {8.0, 4.0, 2.0, 1.0}, {-1.0, -2.0, -3.0, -4.0}};
  const double want[ROWS][N] = {{1.375, 1.875, 3.875, 3.375},      /* I0 + 0.5 Q0 + 0.125 */
                                {-0.25, -2.5, 1.25, -5.0},         /* -0.25 I0 + 2 Q0 - 1 */
                                {16.0, 8.0, 4.0, 2.0},             /* 2 I1 */
                                {5.25, 4.25, 4.25, 4.75}};         /* 0.5 I1 - Q1 + 0.25 */
  const int32_t col_far[8] = {0, 1, 0, 1, 2, 4, 2, 3}, col_back[8] = {0, 1, 1, 0, 2, 3, 2, 3};
  const int64_t ptr_bad[ROWS + 1] = {0, 2, 1, 6, 8};
  const double val_nan[8] = {1.0, 0.5, -0.25, NAN, 2.0, 0.0, 0.5, -1.0}, off_inf[ROWS] = {0.0, 0.0, INFINITY, 0.0};
  double x[ROWS * IN_STRIDE], y[ROWS * OUT_STRIDE];
  wfk_mix_rows_plan* plan = NULL;
  void *xd = NULL, *yd = NULL;
  int r, i;

  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col_far, val, offset, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 2: column 4 is out of range")) return 2;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col_back, val, offset, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "row 1: columns are not ascending")) return 4;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val_nan, offset, &plan) != WFK_EINVAL) return 5;
  if (!strstr(wfk_last_error(), "row 1: coefficient (1, 1) is not finite")) return 6;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, off_inf, &plan) != WFK_EINVAL) return 7;
  if (!strstr(wfk_last_error(), "row 2: offset is not finite")) return 8;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, ptr_bad, col, val, offset, &plan) != WFK_EINVAL) return 9;
  if (!strstr(wfk_last_error(), "row_ptr is not non-decreasing from 0")) return 10;
  if (wfk_mix_rows_plan_create(-1, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, offset, &plan) != WFK_EINVAL) return 11;
  if (wfk_mix_rows_plan_create(N, 0, ROWS, WFK_OUT_F64, row_ptr, col, val, offset, &plan) != WFK_EINVAL) return 12;
  if (wfk_mix_rows_plan_create(N, ROWS, 0, WFK_OUT_F64, row_ptr, col, val, offset, &plan) != WFK_EINVAL) return 13;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_C128, row_ptr, col, val, offset, &plan) != WFK_EINVAL) return 14;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, NULL, col, val, offset, &plan) != WFK_EINVAL) return 15;
  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, offset, NULL) != WFK_EINVAL) return 16;
  if (wfk_mix_rows_apply(NULL, NULL, N, NULL, N, NULL) != WFK_EINVAL) return 17;
  if (wfk_mix_rows_plan_destroy(NULL) != WFK_OK || wfk_mix_rows_reads(NULL) != 0) return 18;
  if (strcmp(wfk_mix_rows_kernel_name(NULL), "") != 0) return 19;

  if (wfk_mix_rows_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, offset, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 20;
  }
  if (strcmp(wfk_mix_rows_kernel_name(plan), "mix_rows<double>") != 0) return 21;
  if (wfk_mix_rows_reads(plan) != ROWS || WFK_MIX_TILE_ROWS != 8) return 22;       /* one tile, four input rows */
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = NAN;                                /* between the rows: never read into a result */
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < N; ++i) x[r * IN_STRIDE + i] = rows[r][i];
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) y[i] = -5.0;
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK) return 23;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK) return 24;
  /* out of place only; strides; alignment */
  if (wfk_mix_rows_apply(plan, xd, IN_STRIDE, xd, OUT_STRIDE, NULL) != WFK_EINVAL) return 25;
  if (!strstr(wfk_last_error(), "mix rows is out of place: out overlaps in")) return 26;
  if (wfk_mix_rows_apply(plan, xd, IN_STRIDE, (double*)xd + (ROWS - 1) * IN_STRIDE + N - 1, OUT_STRIDE, NULL) != WFK_EINVAL) return 27;
  if (wfk_mix_rows_apply(plan, xd, N - 1, yd, OUT_STRIDE, NULL) != WFK_EINVAL) return 28;
  if (wfk_mix_rows_apply(plan, xd, IN_STRIDE, yd, N - 1, NULL) != WFK_EINVAL) return 29;
  if (wfk_mix_rows_apply(plan, (char*)xd + 4, IN_STRIDE, yd, OUT_STRIDE, NULL) != WFK_EINVAL) return 30;
  if (wfk_mix_rows_apply(plan, xd, IN_STRIDE, yd, OUT_STRIDE, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 31;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK) return 32;
  for (r = 0; r < ROWS; ++r) {
    for (i = 0; i < N; ++i)
      if (y[r * OUT_STRIDE + i] != want[r][i]) {
        fprintf(stderr, "row %d sample %d: got %.17g, want %.17g\n", r, i, y[r * OUT_STRIDE + i], want[r][i]);
        return 33;
      }
    if (y[r * OUT_STRIDE + N] != -5.0) return 34;                                  /* past a row: untouched */
  }
  wfk_mix_rows_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  printf("mixed on the device, 16 values ok\n");
  return 0;
}
