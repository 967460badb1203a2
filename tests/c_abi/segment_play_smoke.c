/* Plain-C consumer of the segment player declarations of include/wfk.h, on the device: the argument checks, then two
 * strided rows of I/Q plays at every source phase (and a third row whose entries overlap) through
 * wfk_segment_play_apply -- the play with the comparison, the verifying pass, the checking pass -- compared code by
 * code and count by count with its own loop, untouched memory included.  Prints "played on the device, parity ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define ROWS 3
#define K 2
#define N 20011
#define MAXSEG 210
#define COUNT 200
#define CAP 9000
#define TABLE_STRIDE (3 * MAXSEG + 5)
#define PACKED_STRIDE (K * CAP + 7)
#define OUT_STRIDE (K * N + 9)
#define EXPECT_STRIDE (K * N + 3)
#define IDLE0 ((int16_t)-3)
#define IDLE1 ((int16_t)12)
#define SENTINEL ((int16_t)-23101)

static int16_t packed[ROWS * PACKED_STRIDE], out[ROWS * OUT_STRIDE], want_out[ROWS * OUT_STRIDE], expect[ROWS * EXPECT_STRIDE];
static int32_t table[ROWS * TABLE_STRIDE];

int main(void) {
  int64_t used[ROWS * 2], report[ROWS * 4], want_report[ROWS * 4];
  wfk_segment_play_plan* plan = NULL;
  void *td = NULL, *pd = NULL, *ud = NULL, *od = NULL, *ed = NULL, *rd = NULL;
  int g, i, j, p, pass;

  if (wfk_segment_play_plan_create(-1, ROWS, K, MAXSEG, CAP, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "n must lie in [0, 2^31 - 1]")) return 2;
  if (wfk_segment_play_plan_create(N, 0, K, MAXSEG, CAP, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "rows must be at least 1")) return 4;
  if (wfk_segment_play_plan_create(N, ROWS, 3, MAXSEG, CAP, &plan) != WFK_EINVAL) return 5;
  if (!strstr(wfk_last_error(), "width must be 1 or 2")) return 6;
  if (wfk_segment_play_plan_create(N, ROWS, K, -1, CAP, &plan) != WFK_EINVAL) return 7;
  if (wfk_segment_play_plan_create(N, ROWS, K, MAXSEG, -1, &plan) != WFK_EINVAL) return 8;
  if (wfk_segment_play_plan_create(N, ROWS, K, MAXSEG, CAP, NULL) != WFK_EINVAL) return 9;
  if (wfk_segment_play_apply(NULL, NULL, 0, NULL, 0, NULL, 0, 0, NULL, 0, NULL, 0, NULL, NULL) != WFK_EINVAL) return 10;
  if (wfk_segment_play_plan_destroy(NULL) != WFK_OK || wfk_segment_play_kernel_name(NULL, 0)[0] ||
      wfk_segment_play_span(NULL) != 0)
    return 11;

  if (wfk_segment_play_plan_create(N, ROWS, K, MAXSEG, CAP, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 12;
  }
  if (strcmp(wfk_segment_play_kernel_name(plan, 0), "segplay_check") != 0) return 13;
  if (strcmp(wfk_segment_play_kernel_name(plan, 3), "segplay_fill<2, true, true>") != 0) return 14;
  if (wfk_segment_play_kernel_name(plan, 4)[0] || wfk_segment_play_span(plan) != 8192) return 15;

  /* the rows: play j is 9 + j % 31 samples at 100 j + j % 7, its codes at an offset that runs through every phase */
  for (i = 0; i < ROWS * TABLE_STRIDE; ++i) table[i] = -9;
  for (i = 0; i < ROWS * PACKED_STRIDE; ++i) packed[i] = (int16_t)(((unsigned)(i + 1) * 2654435761u) >> 13);
  for (g = 0; g < ROWS; ++g) {
    int64_t off = g;
    for (j = 0; j < COUNT; ++j) {
      int32_t* t = table + g * TABLE_STRIDE + 3 * j;
      t[0] = 100 * j + j % 7;
      t[1] = 9 + j % 31;
      t[2] = (int32_t)off;
      off += t[1] + (j % 3);
    }
    used[2 * g] = COUNT;
    used[2 * g + 1] = off;
    if (off > CAP || table[g * TABLE_STRIDE + 3 * (COUNT - 1)] + 40 > N) return 16;
  }
  table[2 * TABLE_STRIDE + 3 * 17] = table[2 * TABLE_STRIDE + 3 * 16] + 8;   /* row 2: play 17 starts inside play 16 */

  /* the definition as a loop; expect = the played row with three codes changed and one stray sample */
  for (i = 0; i < ROWS * OUT_STRIDE; ++i) want_out[i] = SENTINEL;
  for (i = 0; i < ROWS * EXPECT_STRIDE; ++i) expect[i] = 0x2222;
  for (g = 0; g < 2; ++g) {
    const int32_t* t = table + g * TABLE_STRIDE;
    int16_t* w = want_out + g * OUT_STRIDE;
    int64_t played = 0;
    for (i = 0; i < N; ++i) {
      w[K * i] = IDLE0;
      w[K * i + 1] = IDLE1;
    }
    for (j = 0; j < COUNT; ++j) {
      for (p = 0; p < K * t[3 * j + 1]; ++p) w[K * t[3 * j] + p] = packed[g * PACKED_STRIDE + K * t[3 * j + 2] + p];
      played += t[3 * j + 1];
    }
    memcpy(expect + g * EXPECT_STRIDE, w, sizeof(int16_t) * K * N);
    expect[g * EXPECT_STRIDE + K * t[3 * 150] + 1] ^= 4;              /* the Q code of the first sample of play 150 */
    expect[g * EXPECT_STRIDE + K * (t[3 * 20] + t[3 * 20 + 1]) - 1] ^= 1;   /* the last code of play 20 */
    expect[g * EXPECT_STRIDE + K * (t[3 * 20] + 2)] ^= 0x100;         /* and one in its middle */
    expect[g * EXPECT_STRIDE + K * (N - 1)] ^= 2;                     /* the row's last sample: in no play */
    want_report[4 * g] = played;
    want_report[4 * g + 1] = 3;
    want_report[4 * g + 2] = 1;
    want_report[4 * g + 3] = t[3 * 20] + 2;
  }
  for (i = 8; i < 12; ++i) want_report[i] = -1;

  if (wfk_malloc(&td, sizeof table) != WFK_OK || wfk_malloc(&pd, sizeof packed) != WFK_OK ||
      wfk_malloc(&ud, sizeof used) != WFK_OK || wfk_malloc(&od, sizeof out) != WFK_OK ||
      wfk_malloc(&ed, sizeof expect) != WFK_OK || wfk_malloc(&rd, sizeof report) != WFK_OK)
    return 18;
  if (wfk_memcpy_h2d(td, table, sizeof table) != WFK_OK || wfk_memcpy_h2d(pd, packed, sizeof packed) != WFK_OK ||
      wfk_memcpy_h2d(ud, used, sizeof used) != WFK_OK || wfk_memcpy_h2d(ed, expect, sizeof expect) != WFK_OK)
    return 19;
  /* refused applies: a missing report, a missing input, a stride, an overlap */
  if (wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, od, OUT_STRIDE, ed, EXPECT_STRIDE, NULL, NULL) != WFK_EINVAL) return 20;
  if (wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, NULL, IDLE0, IDLE1, od, OUT_STRIDE, ed, EXPECT_STRIDE, rd, NULL) != WFK_EINVAL) return 21;
  if (wfk_segment_play_apply(plan, NULL, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, od, OUT_STRIDE, ed, EXPECT_STRIDE, rd, NULL) != WFK_EINVAL) return 22;
  if (wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, od, K * N - 1, ed, EXPECT_STRIDE, rd, NULL) != WFK_EINVAL) return 23;
  if (wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, (int16_t*)ed + 8, OUT_STRIDE, ed, EXPECT_STRIDE, rd, NULL) != WFK_EINVAL) return 24;
  if (!strstr(wfk_last_error(), "out overlaps expect")) return 25;
  if (wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, od, OUT_STRIDE, ed, EXPECT_STRIDE, (int64_t*)ud, NULL) != WFK_EINVAL) return 26;

  for (pass = 0; pass < 3; ++pass) {   /* play and compare, the verifying pass, the checking pass */
    int rc;
    for (i = 0; i < ROWS * OUT_STRIDE; ++i) out[i] = SENTINEL;
    for (i = 0; i < ROWS * 4; ++i) report[i] = 0x5a5a5a5a5a5aLL;   /* garbage: the apply overwrites it */
    if (wfk_memcpy_h2d(od, out, sizeof out) != WFK_OK || wfk_memcpy_h2d(rd, report, sizeof report) != WFK_OK) return 27;
    rc = wfk_segment_play_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, IDLE0, IDLE1, pass == 0 ? od : NULL,
                                pass == 0 ? OUT_STRIDE : 0, pass < 2 ? ed : NULL, pass < 2 ? EXPECT_STRIDE : 0, rd, NULL);
    if (rc != WFK_OK) {
      fprintf(stderr, "apply %d: %s\n", pass, wfk_last_error());
      return 28;
    }
    if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(out, od, sizeof out) != WFK_OK ||
        wfk_memcpy_d2h(report, rd, sizeof report) != WFK_OK)
      return 29;
    for (i = 0; i < ROWS * 4; ++i) {
      int64_t want = want_report[i];
      if (pass == 2 && want >= 0 && i % 4) want = i % 4 == 3 ? -1 : 0;   /* no expect: [played, 0, 0, -1] */
      if (report[i] != want) {
        fprintf(stderr, "pass %d report %d: got %lld, want %lld\n", pass, i, (long long)report[i], (long long)want);
        return 30;
      }
    }
    for (i = 0; i < ROWS * OUT_STRIDE; ++i)
      if (out[i] != (pass ? SENTINEL : want_out[i])) {
        fprintf(stderr, "pass %d out %d: got %d, want %d\n", pass, i, out[i], want_out[i]);
        return 31;
      }
  }
  wfk_segment_play_plan_destroy(plan);
  wfk_free(td);
  wfk_free(pd);
  wfk_free(ud);
  wfk_free(od);
  wfk_free(ed);
  wfk_free(rd);
  printf("played on the device, parity ok\n");
  return 0;
}
