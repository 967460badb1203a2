/* Plain-C consumer of the segment stage declarations of include/wfk.h, on the device: the argument checks, then two
 * rows of 20000 I/Q samples (40000 codes each, every bit in use, the marker in bit 0 of either code of a pair) through
 * wfk_segment_rows_apply_bit with strided rows and granules of 16 samples, compared entry by entry and code by code
 * with its own loop, untouched memory included; then the sizing pass, and the marks form from bytes.
 * Prints "cut on the device, parity ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 20000
#define ROWS 2
#define K 2
#define A 16
#define BIT 0
#define MAXSEG 40
#define CAP 8000
#define CODES_STRIDE (K * N + 6)
#define TABLE_STRIDE (3 * MAXSEG + 5)
#define PACKED_STRIDE (K * CAP + 10)
#define MARKS_STRIDE (N + 3)

static int16_t codes[ROWS * CODES_STRIDE], packed[ROWS * PACKED_STRIDE], want_packed[ROWS * PACKED_STRIDE];
static int32_t table[ROWS * TABLE_STRIDE], want_table[ROWS * TABLE_STRIDE];
static uint8_t marks[ROWS * MARKS_STRIDE], mask[ROWS * N];

int main(void) {
  int64_t used[ROWS * 2], want_used[ROWS * 2];
  wfk_segment_rows_plan* plan = NULL;
  void *cd = NULL, *td = NULL, *pd = NULL, *ud = NULL, *md = NULL;
  int g, i, q, pass;

  if (wfk_segment_rows_plan_create(-1, ROWS, K, A, MAXSEG, 0, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "n must lie in")) return 2;
  if (wfk_segment_rows_plan_create(N, 0, K, A, MAXSEG, CAP, &plan) != WFK_EINVAL) return 3;
  if (wfk_segment_rows_plan_create(N, ROWS, 3, A, MAXSEG, CAP, &plan) != WFK_EINVAL) return 4;
  if (!strstr(wfk_last_error(), "width must be 1 or 2")) return 5;
  if (wfk_segment_rows_plan_create(N, ROWS, K, 24, MAXSEG, CAP, &plan) != WFK_EINVAL) return 6;
  if (!strstr(wfk_last_error(), "align must be a power of two")) return 7;
  if (wfk_segment_rows_plan_create(N, ROWS, K, 2 * WFK_SEGMENT_MAX_ALIGN, MAXSEG, CAP, &plan) != WFK_EINVAL) return 8;
  if (wfk_segment_rows_plan_create(N, ROWS, K, A, -1, CAP, &plan) != WFK_EINVAL) return 9;
  if (wfk_segment_rows_plan_create(N, ROWS, K, A, MAXSEG, N + 1, &plan) != WFK_EINVAL) return 10;
  if (!strstr(wfk_last_error(), "capacity must lie in [0, n]")) return 11;
  if (wfk_segment_rows_plan_create(N, ROWS, K, A, MAXSEG, CAP, NULL) != WFK_EINVAL) return 12;
  if (wfk_segment_rows_apply_bit(NULL, NULL, 0, 0, NULL, 0, NULL, 0, NULL, NULL) != WFK_EINVAL) return 13;
  if (wfk_segment_rows_apply_marks(NULL, NULL, 0, NULL, 0, NULL, 0, NULL, 0, NULL, NULL) != WFK_EINVAL) return 14;
  if (wfk_segment_rows_plan_destroy(NULL) != WFK_OK || wfk_segment_rows_span(NULL) != 0) return 15;

  if (wfk_segment_rows_plan_create(N, ROWS, K, A, MAXSEG, CAP, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 16;
  }
  if (wfk_segment_rows_span(plan) != 8192) return 17;
  if (strcmp(wfk_segment_rows_kernel_name(plan, 0, 0), "segment_count<2, false>") != 0) return 18;
  if (strcmp(wfk_segment_rows_kernel_name(plan, 1, 0), "segment_scan") != 0) return 19;
  if (strcmp(wfk_segment_rows_kernel_name(plan, 2, 1), "segment_pack<2, true>") != 0) return 20;

  /* gates of 100 .. 340 samples every 700 (row 0) or 450 (row 1: more than MAXSEG segments, more than CAP kept);
   * one crosses the block edge at 8192, row 0 ends inside a gate */
  for (g = 0; g < ROWS; ++g)
    for (i = 0; i < N; ++i) {
      const int period = g ? 450 : 700, phase = (i + 90 * g) % period;
      mask[g * N + i] = phase >= 500 - 260 * g && phase < 600 + 30 * ((i / period) % 9) - 260 * g;
      if (!g && i >= N - 37) mask[i] = 1;
    }
  for (i = 0; i < ROWS * CODES_STRIDE; ++i) codes[i] = (int16_t)(((unsigned)i * 2654435761u) >> 9 | 1);
  for (i = 0; i < ROWS * MARKS_STRIDE; ++i) marks[i] = 1;
  for (g = 0; g < ROWS; ++g)
    for (i = 0; i < N; ++i) {
      int16_t* c = codes + g * CODES_STRIDE + K * i;
      c[0] = (int16_t)(c[0] & ~1);
      c[1] = (int16_t)(c[1] & ~1);
      if (mask[g * N + i]) c[i % 2] |= 1;                        /* on one code of the pair only */
      marks[g * MARKS_STRIDE + i] = mask[g * N + i] ? (uint8_t)(1 + i % 255) : 0;
    }
  /* the definition as a loop over the granules */
  for (i = 0; i < ROWS * TABLE_STRIDE; ++i) want_table[i] = 0x5EC7AB1E;
  for (i = 0; i < ROWS * PACKED_STRIDE; ++i) want_packed[i] = -23101;
  for (g = 0; g < ROWS; ++g) {
    int64_t count = 0, kept = 0, start = -1;
    for (q = 0; q <= (N + A - 1) / A; ++q) {
      int on = 0;
      for (i = q * A; i < (q + 1) * A && i < N; ++i) on |= mask[g * N + i];
      if (on && start < 0) {
        start = (int64_t)q * A;
        if (count < MAXSEG) {
          want_table[g * TABLE_STRIDE + 3 * count] = (int32_t)start;
          want_table[g * TABLE_STRIDE + 3 * count + 2] = (int32_t)kept;
        }
      }
      if (on)
        for (i = q * A; i < (q + 1) * A && i < N; ++i, ++kept)
          if (kept < CAP) memcpy(want_packed + g * PACKED_STRIDE + K * kept, codes + g * CODES_STRIDE + K * i, K * 2);
      if (!on && start >= 0) {
        if (count < MAXSEG) want_table[g * TABLE_STRIDE + 3 * count + 1] = (int32_t)((q * A < N ? q * A : N) - start);
        ++count;
        start = -1;
      }
    }
    want_used[2 * g] = count;
    want_used[2 * g + 1] = kept;
  }
  if (want_used[0] < 20 || want_used[0] > MAXSEG || want_used[1] > CAP || want_used[2] <= MAXSEG || want_used[3] <= CAP) return 21;

  if (wfk_malloc(&cd, sizeof codes) != WFK_OK || wfk_malloc(&td, sizeof table) != WFK_OK ||
      wfk_malloc(&pd, sizeof packed) != WFK_OK || wfk_malloc(&ud, sizeof used) != WFK_OK ||
      wfk_malloc(&md, sizeof marks) != WFK_OK)
    return 22;
  if (wfk_memcpy_h2d(cd, codes, sizeof codes) != WFK_OK || wfk_memcpy_h2d(md, marks, sizeof marks) != WFK_OK) return 23;
  /* refused applies: the bit, a missing side, strides, overlap */
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, 16, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 24;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, TABLE_STRIDE, pd, PACKED_STRIDE, NULL, NULL) != WFK_EINVAL) return 25;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, NULL, 0, pd, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 26;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, TABLE_STRIDE, NULL, 0, ud, NULL) != WFK_EINVAL) return 27;
  if (wfk_segment_rows_apply_bit(plan, cd, K * N - 1, BIT, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 28;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, 3 * MAXSEG - 1, pd, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 29;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, TABLE_STRIDE, (int16_t*)cd + 8, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 30;
  if (wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, TABLE_STRIDE, pd, PACKED_STRIDE, (int64_t*)td, NULL) != WFK_EINVAL) return 31;
  if (wfk_segment_rows_apply_marks(plan, cd, CODES_STRIDE, NULL, MARKS_STRIDE, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL) != WFK_EINVAL) return 32;

  for (pass = 0; pass < 3; ++pass) {   /* the bit form, the sizing pass, the marks form */
    int rc;
    for (i = 0; i < ROWS * TABLE_STRIDE; ++i) table[i] = 0x5EC7AB1E;
    for (i = 0; i < ROWS * PACKED_STRIDE; ++i) packed[i] = -23101;
    for (i = 0; i < ROWS * 2; ++i) used[i] = 0x5a5a5a5a5a5aLL;   /* garbage: the apply overwrites it */
    if (wfk_memcpy_h2d(td, table, sizeof table) != WFK_OK || wfk_memcpy_h2d(pd, packed, sizeof packed) != WFK_OK ||
        wfk_memcpy_h2d(ud, used, sizeof used) != WFK_OK)
      return 33;
    if (pass == 0)
      rc = wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL);
    else if (pass == 1)
      rc = wfk_segment_rows_apply_bit(plan, cd, CODES_STRIDE, BIT, NULL, 0, NULL, 0, ud, NULL);
    else
      rc = wfk_segment_rows_apply_marks(plan, cd, CODES_STRIDE, md, MARKS_STRIDE, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL);
    if (rc != WFK_OK) {
      fprintf(stderr, "apply %d: %s\n", pass, wfk_last_error());
      return 34;
    }
    if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(table, td, sizeof table) != WFK_OK ||
        wfk_memcpy_d2h(packed, pd, sizeof packed) != WFK_OK || wfk_memcpy_d2h(used, ud, sizeof used) != WFK_OK)
      return 35;
    for (i = 0; i < ROWS * 2; ++i)
      if (used[i] != want_used[i]) {
        fprintf(stderr, "pass %d used %d: got %lld, want %lld\n", pass, i, (long long)used[i], (long long)want_used[i]);
        return 36;
      }
    for (i = 0; i < ROWS * TABLE_STRIDE; ++i)
      if (table[i] != (pass == 1 ? 0x5EC7AB1E : want_table[i])) {
        fprintf(stderr, "pass %d table %d: got %d, want %d\n", pass, i, table[i], want_table[i]);
        return 37;
      }
    for (i = 0; i < ROWS * PACKED_STRIDE; ++i)
      if (packed[i] != (pass == 1 ? -23101 : want_packed[i])) {
        fprintf(stderr, "pass %d packed %d: got %d, want %d\n", pass, i, packed[i], want_packed[i]);
        return 38;
      }
  }
  wfk_segment_rows_plan_destroy(plan);
  wfk_free(cd);
  wfk_free(td);
  wfk_free(pd);
  wfk_free(ud);
  wfk_free(md);
  printf("cut on the device, parity ok\n");
  return 0;
}
