/* Plain-C consumer of the fused mix-to-codes declarations of include/wfk.h, on the device: the argument checks of both
 * halves, then two I/Q pairs of 4 doubles (strided rows) through the 4 x 4 plan of mix_rows_smoke.c (two 2 x 2 blocks with
 * DC offsets) into 6-bit codes left-justified by 2, pairs interleaved, and the 16 codes and 12 counters against
 * constants computed by hand -- every number here is a small binary fraction, so the products and sums are exact:
 *   row 0: I0 + 0.5 Q0 + 0.125 = {1.375, 1.875, 3.875, 3.375};  * 8 + 0.5 = {11.5, 15.5, 31.5, 27.5}: ties to even,
 *          {12, 16, 32 -> 31 (above), 28}
 *   row 1: -0.25 I0 + 2 Q0 - 1 = {-0.25, -2.5, 1.25, -5};       * 4       = {-1, -10, 5, -20}
 *   row 2: 2 I1                = {16, 8, 4, NaN};               * 2 - 3   = {29, 13, 5, NaN -> 0 (nan)}
 *   row 3: 0.5 I1 - Q1 + 0.25  = {5.25, 4.25, 4.25, NaN};       * -16     = {-84, -68, -68 -> -32 (below), NaN -> 0}
 * Prints "mixed to codes on the device, 16 codes ok". */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "wfk.h"

#define N 4
#define ROWS 4
#define IN_STRIDE 7
#define OUT_STRIDE 11
#define CANARY (-21846)

int main(void) {
  const int64_t row_ptr[ROWS + 1] = {0, 2, 4, 6, 8};
  const int32_t col[8] = {0, 1, 0, 1, 2, 3, 2, 3};
  const double val[8] = {1.0, 0.5, -0.25, 2.0, 2.0, 0.0, 0.5, -1.0};
  const double mix_offset[ROWS] = {0.125, -1.0, 0.0, 0.25};
  const double gain[ROWS] = {8.0, 4.0, 2.0, -16.0}, dac_offset[ROWS] = {0.5, 0.0, -3.0, 0.0};
  const double rows[ROWS][N] = {{1.0, 2.0, 3.0, 4.0}, {0.5, -0.5, 1.5, -1.5}, {8.0, 4.0, 2.0, NAN}, {-1.0, -2.0, -3.0, -4.0}};
  const int16_t want[ROWS / 2][2 * N] = {{48, -4, 64, -40, 124, 20, 112, -80}, {116, -128, 52, -128, 20, -128, 0, 0}};
  const int64_t want_counts[ROWS][3] = {{0, 1, 0}, {0, 0, 0}, {0, 0, 1}, {3, 0, 1}};
  const int32_t col_far[8] = {0, 1, 0, 1, 2, 4, 2, 3};
  const double gain_inf[ROWS] = {8.0, INFINITY, 2.0, -16.0};
  double x[ROWS * IN_STRIDE];
  int16_t y[(ROWS / 2) * OUT_STRIDE];
  int64_t counts[ROWS][3];
  wfk_mix_dac_plan* plan = NULL;
  void *xd = NULL, *yd = NULL, *cd = NULL;
  int r, i;

  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col_far, val, mix_offset, gain, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 2: column 4 is out of range")) return 2;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain_inf, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "row 1: gain is not finite")) return 4;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 17, 0, 2, &plan) != WFK_EINVAL) return 5;
  if (!strstr(wfk_last_error(), "dac rows plan: bits must lie in [2, 16]")) return 6;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 11, 2, &plan) != WFK_EINVAL) return 7;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 3, &plan) != WFK_EINVAL) return 8;
  if (wfk_mix_dac_plan_create(N, 3, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL) return 9;
  if (!strstr(wfk_last_error(), "dac rows plan: 3 rows are no multiple of the interleave")) return 10;
  if (wfk_mix_dac_plan_create(-1, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL) return 11;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_C128, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL) return 12;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, NULL, dac_offset, 6, 2, 2, &plan) != WFK_EINVAL) return 13;
  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 2, NULL) != WFK_EINVAL) return 14;
  if (wfk_mix_dac_apply(NULL, NULL, N, NULL, N, NULL, NULL) != WFK_EINVAL) return 15;
  if (wfk_mix_dac_plan_destroy(NULL) != WFK_OK || wfk_mix_dac_reads(NULL) != 0 || wfk_mix_dac_span(NULL) != 0) return 16;
  if (strcmp(wfk_mix_dac_kernel_name(NULL, 1), "") != 0) return 17;

  if (wfk_mix_dac_plan_create(N, ROWS, ROWS, WFK_OUT_F64, row_ptr, col, val, mix_offset, gain, dac_offset, 6, 2, 2, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 20;
  }
  if (strcmp(wfk_mix_dac_kernel_name(plan, 0), "mix_dac_rows<double,2,false>") != 0) return 21;
  if (strcmp(wfk_mix_dac_kernel_name(plan, 1), "mix_dac_rows<double,2,true>") != 0) return 21;
  if (wfk_mix_dac_reads(plan) != ROWS || wfk_mix_dac_span(plan) != 8192) return 22;   /* one tile, four input rows */
  for (i = 0; i < ROWS * IN_STRIDE; ++i) x[i] = NAN;                                 /* between the rows: never read into a code */
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < N; ++i) x[r * IN_STRIDE + i] = rows[r][i];
  for (i = 0; i < (ROWS / 2) * OUT_STRIDE; ++i) y[i] = CANARY;
  memset(counts, 0x5a, sizeof counts);                                               /* garbage: an apply overwrites it */
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK) return 23;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK ||
      wfk_memcpy_h2d(cd, counts, sizeof counts) != WFK_OK)
    return 24;
  /* out of place only; strides; alignment; the counts apart from both sides */
  if (wfk_mix_dac_apply(plan, xd, IN_STRIDE, (int16_t*)xd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 25;
  if (!strstr(wfk_last_error(), "mix dac is out of place: out overlaps in")) return 26;
  if (wfk_mix_dac_apply(plan, xd, N - 1, (int16_t*)yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 27;
  if (wfk_mix_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, 2 * N - 1, NULL, NULL) != WFK_EINVAL) return 28;
  if (wfk_mix_dac_apply(plan, (char*)xd + 4, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 29;
  if (wfk_mix_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)xd, NULL) != WFK_EINVAL) return 30;
  if (!strstr(wfk_last_error(), "counts overlaps in")) return 30;
  if (wfk_mix_dac_apply(plan, xd, IN_STRIDE, (int16_t*)yd, OUT_STRIDE, (int64_t*)cd, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 31;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 32;
  for (r = 0; r < ROWS / 2; ++r) {
    for (i = 0; i < 2 * N; ++i)
      if (y[r * OUT_STRIDE + i] != want[r][i]) {
        fprintf(stderr, "code row %d position %d: got %d, want %d\n", r, i, y[r * OUT_STRIDE + i], want[r][i]);
        return 33;
      }
    for (i = 2 * N; i < OUT_STRIDE; ++i)
      if (y[r * OUT_STRIDE + i] != CANARY) return 34;                                /* past a row: untouched */
  }
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < 3; ++i)
      if (counts[r][i] != want_counts[r][i]) {
        fprintf(stderr, "row %d counter %d: got %lld, want %lld\n", r, i, (long long)counts[r][i], (long long)want_counts[r][i]);
        return 35;
      }
  wfk_mix_dac_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  wfk_free(cd);
  printf("mixed to codes on the device, 16 codes ok\n");
  return 0;
}
