/* Plain-C consumer of the marker stage declarations of include/wfk.h, on the device: the argument checks, then two
 * I/Q pairs of 20000 doubles (bursts between exact zeros, an inf and a NaN among them) through
 * wfk_marker_rows_apply_codes with strided rows: the marker of each pair written into bit 0 of codes with every bit in
 * use, compared code by code and count by count with its own loop; then the same markers as bytes.
 * Prints "marked on the device, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 20000
#define ROWS 4
#define K 2
#define BIT 0
#define IN_STRIDE 20003
#define CODES_STRIDE (K * N + 11)
#define OUT_STRIDE (N + 5)

int main(void) {
  static double x[ROWS * IN_STRIDE];
  static int16_t codes[(ROWS / K) * CODES_STRIDE], filled[(ROWS / K) * CODES_STRIDE];
  static uint8_t m[(ROWS / K) * N], bytes[(ROWS / K) * OUT_STRIDE];
  int64_t counts[(ROWS / K) * 2], want_counts[(ROWS / K) * 2];
  const double threshold[ROWS / K] = {0.0, 0.25}, bad_thr[ROWS / K] = {0.0, -1.0}, nan_thr[ROWS / K] = {NAN, 0.0};
  const int32_t lead[ROWS / K] = {20, 1000}, trail[ROWS / K] = {10, 0};
  const int32_t long_lead[ROWS / K] = {20, WFK_MARKER_MAX_EDGE + 1}, neg_trail[ROWS / K] = {-1, 0};
  wfk_marker_rows_plan* plan = NULL;
  void *xd = NULL, *yd = NULL, *bd = NULL, *cd = NULL;
  int g, r, i, j;

  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, bad_thr, lead, trail, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "row 1: threshold is negative")) return 2;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, nan_thr, lead, trail, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "row 0: threshold is not finite")) return 4;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, threshold, long_lead, trail, &plan) != WFK_EINVAL) return 5;
  if (!strstr(wfk_last_error(), "row 1: lead exceeds 4096")) return 6;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, threshold, lead, neg_trail, &plan) != WFK_EINVAL) return 7;
  if (!strstr(wfk_last_error(), "row 0: trail is negative")) return 8;
  if (wfk_marker_rows_plan_create(-1, ROWS, WFK_OUT_F64, K, threshold, lead, trail, &plan) != WFK_EINVAL) return 9;
  if (wfk_marker_rows_plan_create(N, 0, WFK_OUT_F64, K, threshold, lead, trail, &plan) != WFK_EINVAL) return 10;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_C128, K, threshold, lead, trail, &plan) != WFK_EINVAL) return 11;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, 3, threshold, lead, trail, &plan) != WFK_EINVAL) return 12;
  if (wfk_marker_rows_plan_create(N, 3, WFK_OUT_F64, K, threshold, lead, trail, &plan) != WFK_EINVAL) return 13;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, NULL, lead, trail, &plan) != WFK_EINVAL) return 14;
  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, threshold, lead, trail, NULL) != WFK_EINVAL) return 15;
  if (wfk_marker_rows_apply(NULL, NULL, N, NULL, N, NULL, NULL) != WFK_EINVAL) return 16;
  if (wfk_marker_rows_apply_codes(NULL, NULL, N, NULL, N, 0, NULL, NULL) != WFK_EINVAL) return 17;
  if (wfk_marker_rows_plan_destroy(NULL) != WFK_OK || wfk_marker_rows_span(NULL, 0) != 0) return 18;

  if (wfk_marker_rows_plan_create(N, ROWS, WFK_OUT_F64, K, threshold, lead, trail, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 19;
  }
  if (strcmp(wfk_marker_rows_kernel_name(plan, 0, 0), "marker_rows<double>") != 0) return 20;
  if (strcmp(wfk_marker_rows_kernel_name(plan, 1, 1), "marker_rows_codes_count<double>") != 0) return 21;
  if (wfk_marker_rows_span(plan, 0) != 16384 || wfk_marker_rows_span(plan, 1) != 8192 / K) return 22;
  /* bursts of 30 .. 70 samples every 1500 .. 3300, the Q of a pair a little later than its I; exact zeros between */
  for (r = 0; r < ROWS; ++r)
    for (i = 0; i < N; ++i) {
      const int period = 1500 + 600 * (r / K) * 3, phase = (i + 40 * r) % period;
      x[r * IN_STRIDE + i] = phase >= 400 && phase < 430 + 20 * (r / K) * 2 ? 0.3 + 0.5 * sin(0.2 * phase) : 0.0;
    }
  for (i = 0; i < N; ++i)
    if (i % 97 == 0) x[2 * IN_STRIDE + i] = 0.25;      /* equal to the threshold of pair 1: not active */
  x[0 * IN_STRIDE + 9000] = INFINITY;                  /* active */
  x[1 * IN_STRIDE + 9500] = NAN;                       /* not active */
  x[3 * IN_STRIDE + 19999] = -1.0;                     /* the last sample of the row */
  for (i = 0; i < (ROWS / K) * CODES_STRIDE; ++i)
    filled[i] = codes[i] = (int16_t)((i * 2654435761u) >> 7);   /* every bit in use, bit 0 among them */
  for (i = 0; i < (ROWS / K) * OUT_STRIDE; ++i) bytes[i] = 0xAA;
  for (i = 0; i < (ROWS / K) * 2; ++i) counts[i] = 0x5a5a5a5a5a5aLL;   /* garbage: the apply overwrites it */
  if (wfk_malloc(&xd, sizeof x) != WFK_OK || wfk_malloc(&yd, sizeof codes) != WFK_OK ||
      wfk_malloc(&bd, sizeof bytes) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK)
    return 23;
  if (wfk_memcpy_h2d(xd, x, sizeof x) != WFK_OK || wfk_memcpy_h2d(yd, codes, sizeof codes) != WFK_OK ||
      wfk_memcpy_h2d(bd, bytes, sizeof bytes) != WFK_OK || wfk_memcpy_h2d(cd, counts, sizeof counts) != WFK_OK)
    return 24;
  /* the codes and the counts may not meet the input; strides; the bit */
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)xd, CODES_STRIDE, BIT, NULL, NULL) != WFK_EINVAL) return 25;
  if (wfk_marker_rows_apply_codes(plan, xd, N - 1, (int16_t*)yd, CODES_STRIDE, BIT, NULL, NULL) != WFK_EINVAL) return 26;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, K * N - 1, BIT, NULL, NULL) != WFK_EINVAL) return 27;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, CODES_STRIDE, BIT, (int64_t*)xd, NULL) != WFK_EINVAL) return 28;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, CODES_STRIDE, BIT, (int64_t*)yd, NULL) != WFK_EINVAL) return 29;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, CODES_STRIDE, 16, NULL, NULL) != WFK_EINVAL) return 30;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, CODES_STRIDE, -1, NULL, NULL) != WFK_EINVAL) return 31;
  if (wfk_marker_rows_apply(plan, xd, IN_STRIDE, (uint8_t*)xd + 8, OUT_STRIDE, NULL, NULL) != WFK_EINVAL) return 32;
  if (wfk_marker_rows_apply_codes(plan, xd, IN_STRIDE, (int16_t*)yd, CODES_STRIDE, BIT, (int64_t*)cd, NULL) != WFK_OK) {
    fprintf(stderr, "apply_codes: %s\n", wfk_last_error());
    return 33;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(codes, yd, sizeof codes) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 34;
  /* the definition as a loop */
  memset(want_counts, 0, sizeof want_counts);
  for (g = 0; g < ROWS / K; ++g)
    for (i = 0; i < N; ++i) {
      uint8_t high = 0;
      for (j = i - trail[g]; j <= i + lead[g] && !high; ++j)
        for (r = g * K; r < g * K + K && j >= 0 && j < N; ++r)
          if (fabs(x[r * IN_STRIDE + j]) > threshold[g]) high = 1;
      m[g * N + i] = high;
      want_counts[g * 2] += high;
      want_counts[g * 2 + 1] += high && (i == 0 || !m[g * N + i - 1]);
    }
  for (g = 0; g < ROWS / K; ++g) {
    for (i = 0; i < K * N; ++i) {
      const int16_t was = filled[g * CODES_STRIDE + i];
      const int16_t want = (int16_t)((was & ~(1 << BIT)) | (m[g * N + i / K] << BIT));
      if (codes[g * CODES_STRIDE + i] != want) {
        fprintf(stderr, "row %d code %d: got %d, want %d\n", g, i, codes[g * CODES_STRIDE + i], want);
        return 35;
      }
    }
    for (i = K * N; i < CODES_STRIDE; ++i)
      if (codes[g * CODES_STRIDE + i] != filled[g * CODES_STRIDE + i]) return 36;   /* past a row: untouched */
  }
  for (i = 0; i < (ROWS / K) * 2; ++i)
    if (counts[i] != want_counts[i]) {
      fprintf(stderr, "count %d: got %lld, want %lld\n", i, (long long)counts[i], (long long)want_counts[i]);
      return 37;
    }
  if (want_counts[1] < 10 || want_counts[3] < 3 || want_counts[0] >= N || want_counts[2] >= N) return 38;
  if (!m[9000] || m[9500 + 11] || !m[N + N - 1]) return 39;          /* inf marks, NaN does not, the last sample does */
  /* the same markers as bytes */
  if (wfk_marker_rows_apply(plan, xd, IN_STRIDE, (uint8_t*)bd, OUT_STRIDE, (int64_t*)cd, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 40;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(bytes, bd, sizeof bytes) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 41;
  for (g = 0; g < ROWS / K; ++g) {
    for (i = 0; i < N; ++i)
      if (bytes[g * OUT_STRIDE + i] != m[g * N + i]) {
        fprintf(stderr, "row %d marker %d: got %d, want %d\n", g, i, bytes[g * OUT_STRIDE + i], m[g * N + i]);
        return 42;
      }
    for (i = N; i < OUT_STRIDE; ++i)
      if (bytes[g * OUT_STRIDE + i] != 0xAA) return 43;
  }
  for (i = 0; i < (ROWS / K) * 2; ++i)
    if (counts[i] != want_counts[i]) return 44;                      /* overwritten, not added to */
  wfk_marker_rows_plan_destroy(plan);
  wfk_free(xd);
  wfk_free(yd);
  wfk_free(bd);
  wfk_free(cd);
  printf("marked on the device, parity ok\n");
  return 0;
}
