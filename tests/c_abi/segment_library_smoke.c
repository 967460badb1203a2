/* Plain-C consumer of the segment library declarations of include/wfk.h, on the device: the argument checks, then two
 * strided rows of 300 I/Q segments drawn from 5 shapes (and a third row that cannot be read) through
 * wfk_segment_library_apply, compared entry by entry and code by code with its own double loop, untouched memory
 * included; then the sizing pass.  Prints "library on the device, parity ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define ROWS 3
#define K 2
#define MAXSEG 310
#define COUNT 300
#define SHAPES 5
#define CAP 20000
#define LIBCAP 100
#define TABLE_STRIDE (3 * MAXSEG + 5)
#define PACKED_STRIDE (K * CAP + 7)
#define SLOTS_STRIDE (MAXSEG + 3)
#define LIB_STRIDE (K * LIBCAP + 9)

static int16_t packed[ROWS * PACKED_STRIDE], library[ROWS * LIB_STRIDE], want_library[ROWS * LIB_STRIDE];
static int32_t table[ROWS * TABLE_STRIDE], plays[ROWS * TABLE_STRIDE], want_plays[ROWS * TABLE_STRIDE];
static int32_t slots[ROWS * SLOTS_STRIDE], want_slots[ROWS * SLOTS_STRIDE];

static int shape_length(int d) { return 9 + 8 * d + d % 2; }
static int16_t shape_code(int d, int p) { return (int16_t)(((unsigned)(p + 1) * 2654435761u * (unsigned)(d + 3)) >> 11); }

int main(void) {
  int64_t used[ROWS * 2], lib_used[ROWS * 2], want_used[ROWS * 2];
  wfk_segment_library_plan* plan = NULL;
  void *td = NULL, *pd = NULL, *ud = NULL, *yd = NULL, *sd = NULL, *ld = NULL, *rd = NULL;
  int g, i, j, p, pass;

  if (wfk_segment_library_plan_create(0, K, MAXSEG, CAP, LIBCAP, &plan) != WFK_EINVAL || plan) return 1;
  if (!strstr(wfk_last_error(), "rows must be at least 1")) return 2;
  if (wfk_segment_library_plan_create(ROWS, 3, MAXSEG, CAP, LIBCAP, &plan) != WFK_EINVAL) return 3;
  if (!strstr(wfk_last_error(), "width must be 1 or 2")) return 4;
  if (wfk_segment_library_plan_create(ROWS, K, -1, CAP, LIBCAP, &plan) != WFK_EINVAL) return 5;
  if (wfk_segment_library_plan_create(ROWS, K, MAXSEG, -1, 0, &plan) != WFK_EINVAL) return 6;
  if (wfk_segment_library_plan_create(ROWS, K, MAXSEG, CAP, CAP + 1, &plan) != WFK_EINVAL) return 7;
  if (!strstr(wfk_last_error(), "lib_capacity must lie in [0, capacity]")) return 8;
  if (wfk_segment_library_plan_create(ROWS, K, MAXSEG, CAP, LIBCAP, NULL) != WFK_EINVAL) return 9;
  if (wfk_segment_library_apply(NULL, NULL, 0, NULL, 0, NULL, NULL, 0, NULL, 0, NULL, 0, NULL, NULL) != WFK_EINVAL) return 10;
  if (wfk_segment_library_plan_destroy(NULL) != WFK_OK || wfk_segment_library_kernel_name(NULL, 0)[0]) return 11;

  if (wfk_segment_library_plan_create(ROWS, K, MAXSEG, CAP, LIBCAP, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 12;
  }
  if (strncmp(wfk_segment_library_kernel_name(plan, 0), "seglib_hash", 11) != 0) return 13;
  if (strcmp(wfk_segment_library_kernel_name(plan, 2), "seglib_scan") != 0) return 14;
  if (strcmp(wfk_segment_library_kernel_name(plan, 3), "seglib_copy") != 0 || wfk_segment_library_kernel_name(plan, 4)[0]) return 15;

  /* the rows: segment j plays shape (7 j + 3 g + j / 11) % SHAPES, the codes back to back at odd and even offsets */
  for (i = 0; i < ROWS * TABLE_STRIDE; ++i) table[i] = -9;
  for (i = 0; i < ROWS * PACKED_STRIDE; ++i) packed[i] = 0x3333;
  for (g = 0; g < ROWS; ++g) {
    int64_t off = g;
    for (j = 0; j < COUNT; ++j) {
      const int d = (7 * j + 3 * g + j / 11) % SHAPES, n = shape_length(d);
      int32_t* t = table + g * TABLE_STRIDE + 3 * j;
      t[0] = (int32_t)(40 * j);
      t[1] = n;
      t[2] = (int32_t)off;
      for (p = 0; p < K * n; ++p) packed[g * PACKED_STRIDE + K * off + p] = shape_code(d, p);
      off += n;
    }
    used[2 * g] = COUNT;
    used[2 * g + 1] = off;
    if (off > CAP) return 16;
  }
  table[2 * TABLE_STRIDE + 3 * 17 + 2] = CAP - 3;   /* row 2: an entry that reaches past the packed row */

  /* the definition as a double loop */
  for (i = 0; i < ROWS * TABLE_STRIDE; ++i) want_plays[i] = 0x5EC7AB1E;
  for (i = 0; i < ROWS * SLOTS_STRIDE; ++i) want_slots[i] = 0x51075;
  for (i = 0; i < ROWS * LIB_STRIDE; ++i) want_library[i] = -23101;
  for (g = 0; g < 2; ++g) {
    const int32_t* t = table + g * TABLE_STRIDE;
    const int16_t* y = packed + g * PACKED_STRIDE;
    int64_t unique = 0, kept = 0;
    for (j = 0; j < COUNT; ++j) {
      int first = j;
      for (i = 0; i < j; ++i)
        if (t[3 * i + 1] == t[3 * j + 1] && !memcmp(y + K * t[3 * i + 2], y + K * t[3 * j + 2], (size_t)(K * 2 * t[3 * j + 1]))) {
          first = i;
          break;
        }
      want_plays[g * TABLE_STRIDE + 3 * j] = t[3 * j];
      want_plays[g * TABLE_STRIDE + 3 * j + 1] = t[3 * j + 1];
      if (first == j) {
        want_plays[g * TABLE_STRIDE + 3 * j + 2] = (int32_t)kept;
        want_slots[g * SLOTS_STRIDE + j] = (int32_t)unique++;
        for (p = 0; p < K * t[3 * j + 1]; ++p)
          if (K * kept + p < K * LIBCAP) want_library[g * LIB_STRIDE + K * kept + p] = y[K * t[3 * j + 2] + p];
        kept += t[3 * j + 1];
      } else {
        want_plays[g * TABLE_STRIDE + 3 * j + 2] = want_plays[g * TABLE_STRIDE + 3 * first + 2];
        want_slots[g * SLOTS_STRIDE + j] = want_slots[g * SLOTS_STRIDE + first];
      }
    }
    want_used[2 * g] = unique;
    want_used[2 * g + 1] = kept;
  }
  want_used[4] = want_used[5] = -1;
  if (want_used[0] != SHAPES || want_used[2] != SHAPES || want_used[1] <= LIBCAP) return 17;   /* the library is cut */

  if (wfk_malloc(&td, sizeof table) != WFK_OK || wfk_malloc(&pd, sizeof packed) != WFK_OK ||
      wfk_malloc(&ud, sizeof used) != WFK_OK || wfk_malloc(&yd, sizeof plays) != WFK_OK ||
      wfk_malloc(&sd, sizeof slots) != WFK_OK || wfk_malloc(&ld, sizeof library) != WFK_OK ||
      wfk_malloc(&rd, sizeof lib_used) != WFK_OK)
    return 18;
  if (wfk_memcpy_h2d(td, table, sizeof table) != WFK_OK || wfk_memcpy_h2d(pd, packed, sizeof packed) != WFK_OK ||
      wfk_memcpy_h2d(ud, used, sizeof used) != WFK_OK)
    return 19;
  /* refused applies: a missing report, a missing input, a stride, an overlap */
  if (wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, ld, LIB_STRIDE, NULL, NULL) != WFK_EINVAL) return 20;
  if (wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, NULL, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, ld, LIB_STRIDE, rd, NULL) != WFK_EINVAL) return 21;
  if (wfk_segment_library_apply(plan, NULL, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, ld, LIB_STRIDE, rd, NULL) != WFK_EINVAL) return 22;
  if (wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, 3 * MAXSEG - 1, sd, SLOTS_STRIDE, ld, LIB_STRIDE, rd, NULL) != WFK_EINVAL) return 23;
  if (wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, (int16_t*)pd + 8, LIB_STRIDE, rd, NULL) != WFK_EINVAL) return 24;
  if (!strstr(wfk_last_error(), "library overlaps packed")) return 25;
  if (wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, ld, LIB_STRIDE, (int64_t*)ud, NULL) != WFK_EINVAL) return 26;

  for (pass = 0; pass < 2; ++pass) {   /* an apply, the sizing pass */
    int rc;
    for (i = 0; i < ROWS * TABLE_STRIDE; ++i) plays[i] = 0x5EC7AB1E;
    for (i = 0; i < ROWS * SLOTS_STRIDE; ++i) slots[i] = 0x51075;
    for (i = 0; i < ROWS * LIB_STRIDE; ++i) library[i] = -23101;
    for (i = 0; i < ROWS * 2; ++i) lib_used[i] = 0x5a5a5a5a5a5aLL;   /* garbage: the apply overwrites it */
    if (wfk_memcpy_h2d(yd, plays, sizeof plays) != WFK_OK || wfk_memcpy_h2d(sd, slots, sizeof slots) != WFK_OK ||
        wfk_memcpy_h2d(ld, library, sizeof library) != WFK_OK || wfk_memcpy_h2d(rd, lib_used, sizeof lib_used) != WFK_OK)
      return 27;
    if (pass == 0)
      rc = wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, yd, TABLE_STRIDE, sd, SLOTS_STRIDE, ld, LIB_STRIDE, rd, NULL);
    else
      rc = wfk_segment_library_apply(plan, td, TABLE_STRIDE, pd, PACKED_STRIDE, ud, NULL, 0, NULL, 0, NULL, 0, rd, NULL);
    if (rc != WFK_OK) {
      fprintf(stderr, "apply %d: %s\n", pass, wfk_last_error());
      return 28;
    }
    if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(plays, yd, sizeof plays) != WFK_OK ||
        wfk_memcpy_d2h(slots, sd, sizeof slots) != WFK_OK || wfk_memcpy_d2h(library, ld, sizeof library) != WFK_OK ||
        wfk_memcpy_d2h(lib_used, rd, sizeof lib_used) != WFK_OK)
      return 29;
    for (i = 0; i < ROWS * 2; ++i)
      if (lib_used[i] != want_used[i]) {
        fprintf(stderr, "pass %d lib_used %d: got %lld, want %lld\n", pass, i, (long long)lib_used[i], (long long)want_used[i]);
        return 30;
      }
    for (i = 0; i < ROWS * TABLE_STRIDE; ++i)
      if (plays[i] != (pass == 1 ? 0x5EC7AB1E : want_plays[i])) {
        fprintf(stderr, "pass %d plays %d: got %d, want %d\n", pass, i, plays[i], want_plays[i]);
        return 31;
      }
    for (i = 0; i < ROWS * SLOTS_STRIDE; ++i)
      if (slots[i] != (pass == 1 ? 0x51075 : want_slots[i])) {
        fprintf(stderr, "pass %d slots %d: got %d, want %d\n", pass, i, slots[i], want_slots[i]);
        return 32;
      }
    for (i = 0; i < ROWS * LIB_STRIDE; ++i)
      if (library[i] != (pass == 1 ? -23101 : want_library[i])) {
        fprintf(stderr, "pass %d library %d: got %d, want %d\n", pass, i, library[i], want_library[i]);
        return 33;
      }
  }
  wfk_segment_library_plan_destroy(plan);
  wfk_free(td);
  wfk_free(pd);
  wfk_free(ud);
  wfk_free(yd);
  wfk_free(sd);
  wfk_free(ld);
  wfk_free(rd);
  printf("library on the device, parity ok\n");
  return 0;
}
