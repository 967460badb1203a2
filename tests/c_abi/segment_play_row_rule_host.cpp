// segment_play_row_rule_host.cpp -- the segment player's lines of the row rule (csrc/wfk_row_rule.h; DESIGN.md "The
// row rule") held by a plain host program: no HIP, no device, addresses are plain integers and nothing is
// dereferenced.  `play` gives the rule the sides wfk_segment_play_apply gives it: out against the inputs (table, packed,
// used and, where given, expect), the report [played, differ, stray, first] against every side; without out the inputs
// and the report alone.  Exit status 0 and "segment play row rule ok" when every assertion holds; the first that does
// not prints its line and ends with 1.
#include "wfk_row_rule.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

#define HOLD(cond)                                                    \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);    \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

const void* at(uint64_t a) { return (const void*)(uintptr_t)a; }

std::string why;
int keep(int code, const std::string& text) {
  why = text;
  return code;
}

#define ACCEPTED(call) HOLD((call) == WFK_OK)
#define REFUSED(call, word)                                                                                     \
  do {                                                                                                          \
    why.clear();                                                                                                \
    HOLD((call) == WFK_EINVAL);                                                                                 \
    if (why.find("segment play") != 0 || !std::strstr(why.c_str(), word)) {                                     \
      std::printf("line %d: \"%s\" does not start with \"segment play\" or lacks \"%s\"\n", __LINE__, why.c_str(), word); \
      std::exit(1);                                                                                             \
    }                                                                                                           \
  } while (0)

typedef SegmentPlayShape Shape;

// as the apply calls the rule; out = 0: the verifying pass (expect given) or the checking pass (neither)
int play(const Shape& s, uint64_t table, int64_t table_stride, uint64_t packed, int64_t packed_stride, uint64_t used,
         uint64_t out, int64_t out_stride, uint64_t expect, int64_t expect_stride, uint64_t report) {
  return wfk_segment_play_row_rule(s, at(table), table_stride, at(packed), packed_stride, at(used), at(out), out_stride,
                                   at(expect), expect_stride, at(report), keep);
}

const uint64_t T = 1ull << 24, Y = 1ull << 25, U = 1ull << 26, O = 1ull << 27, E = 1ull << 28, R = 1ull << 30;

void clauses() {
  for (const int64_t k : {(int64_t)1, (int64_t)2}) {
    const Shape s{4, 101, k, 7, 33};
    const int64_t tn = 3 * s.max_segments, yn = k * s.capacity, on = k * s.n;
    const uint64_t t_ext = (uint64_t)(s.rows * tn) * 4, y_ext = (uint64_t)(s.rows * yn) * 2, u_ext = (uint64_t)s.rows * 16,
                   o_ext = (uint64_t)(s.rows * on) * 2, rep = (uint64_t)s.rows * 32;
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, E, on, R));
    ACCEPTED(play(s, T, tn + 3, Y, yn + 5, U, O, on + 7, E, on + 1, R));
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, 0, 0, R));                                // the play alone
    ACCEPTED(play(s, T, tn, Y, yn, U, 0, 0, E, on, R));                                // the verifying pass
    ACCEPTED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, R));                                 // the checking pass
    // an input that holds something is there, in every form of the apply
    REFUSED(play(s, 0, tn, Y, yn, U, O, on, E, on, R), "null");
    REFUSED(play(s, T, tn, 0, yn, U, O, on, E, on, R), "null");
    REFUSED(play(s, T, tn, Y, yn, 0, O, on, E, on, R), "null");
    REFUSED(play(s, 0, tn, Y, yn, U, 0, 0, E, on, R), "null");
    REFUSED(play(s, T, tn, 0, yn, U, 0, 0, 0, 0, R), "null");
    REFUSED(play(s, T, tn, Y, yn, 0, 0, 0, 0, 0, R), "null");
    // aligned to their element: codes to 2, the table to 4, used to 8
    REFUSED(play(s, T + 2, tn, Y, yn, U, O, on, E, on, R), "not aligned");
    REFUSED(play(s, T, tn, Y + 1, yn, U, O, on, E, on, R), "not aligned");
    REFUSED(play(s, T, tn, Y, yn, U + 4, O, on, E, on, R), "not aligned");
    REFUSED(play(s, T, tn, Y, yn, U, O + 1, on, E, on, R), "not aligned");
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E + 1, on, R), "not aligned");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, E + 1, on, R), "not aligned");
    REFUSED(play(s, T + 2, tn, Y, yn, U, 0, 0, 0, 0, R), "not aligned");
    for (uint64_t lead = 0; lead < 16; lead += 2)                                      // every lead of the code rows
      ACCEPTED(play(s, T + 4, tn, Y + lead, yn, U + 8, O + 14 - lead, on, E + (lead * 3) % 16, on, R + 8));
    // strides
    REFUSED(play(s, T, tn - 1, Y, yn, U, O, on, E, on, R), "table row stride smaller");
    REFUSED(play(s, T, tn, Y, yn - 1, U, O, on, E, on, R), "packed row stride smaller");
    REFUSED(play(s, T, tn, Y, yn, U, O, on - 1, E, on, R), "out row stride smaller");
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on - 1, R), "expect row stride smaller");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, E, on - 1, R), "expect row stride smaller");
    REFUSED(play(s, T, tn - 1, Y, yn, U, 0, 0, 0, 0, R), "table row stride smaller");
    // out meets no input, expect among them
    REFUSED(play(s, T, tn, Y, yn, U, Y, on, E, on, R), "out overlaps packed");
    REFUSED(play(s, T, tn, Y, yn, U, Y + y_ext - 2, on, E, on, R), "out overlaps packed");
    ACCEPTED(play(s, T, tn, Y, yn, U, Y + y_ext, on, E, on, R));
    REFUSED(play(s, T, tn, Y, yn, U, Y - o_ext + 2, on, E, on, R), "out overlaps packed");
    ACCEPTED(play(s, T, tn, Y, yn, U, Y - o_ext, on, E, on, R));
    REFUSED(play(s, T, tn, Y, yn, U, T + t_ext - 2, on, E, on, R), "out overlaps table");
    REFUSED(play(s, T, tn, Y, yn, U, U + u_ext - 2, on, E, on, R), "out overlaps used");
    REFUSED(play(s, T, tn, Y, yn, U, E, on, E, on, R), "out overlaps expect");
    REFUSED(play(s, T, tn, Y, yn, U, E + o_ext - 2, on, E, on, R), "out overlaps expect");
    ACCEPTED(play(s, T, tn, Y, yn, U, E + o_ext, on, E, on, R));
    ACCEPTED(play(s, T, tn, Y, yn, U, E, on, 0, 0, R));                                // an expect that is not given
    ACCEPTED(play(s, T, tn, T, yn, U, O, on, Y, on, R));                               // the inputs may meet each other
    ACCEPTED(play(s, T, tn, Y, yn, U, 0, 0, Y, on, R));
    // the report: rows x 4 int64, aligned to 8, meets no side
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, R + 4), "counts are not aligned");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, R + 4), "counts are not aligned");
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, T + t_ext - 8), "counts overlaps table");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, T + t_ext - 8), "counts overlaps table");
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, E, on, T + t_ext));
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, T - rep + 8), "counts overlaps table");
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, E, on, T - rep));
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, Y + y_ext - 8), "counts overlaps packed");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, Y + 8), "counts overlaps packed");
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, U), "counts overlaps used");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, U + u_ext - 8), "counts overlaps used");
    ACCEPTED(play(s, T, tn, Y, yn, U, 0, 0, 0, 0, U + u_ext));
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, O + o_ext - 8), "counts overlaps out");
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, E, on, O + o_ext));
    REFUSED(play(s, T, tn, Y, yn, U, O, on, E, on, E + 8), "counts overlaps expect");
    REFUSED(play(s, T, tn, Y, yn, U, 0, 0, E, on, E + o_ext - 8), "counts overlaps expect");
    ACCEPTED(play(s, T, tn, Y, yn, U, O, on, 0, 0, E));                                // where no expect is given
    ACCEPTED(play(s, T, tn, Y, yn, U, 0, 0, E, on, O));                                // where no out is given
    // the earlier clause speaks
    REFUSED(play(s, 0, tn, Y, yn, U, O, on, E, on, R + 4), "counts are not aligned");
    REFUSED(play(s, 0, tn, Y + 1, yn, U, O, on, E, on, R), "null");
    REFUSED(play(s, T + 2, tn - 1, Y, yn, U, O, on, E, on, R), "not aligned");
    REFUSED(play(s, T, tn - 1, Y, yn, U, Y, on, E, on, R), "stride smaller");
    // a side that holds nothing is not looked at: it may be null, misaligned or anywhere
    const Shape no_segments{4, 101, k, 0, 33}, no_codes{4, 101, k, 7, 0}, no_samples{4, 0, k, 7, 33},
        nothing{4, 0, k, 0, 0};
    ACCEPTED(play(no_segments, 0, 0, Y, yn, U, O, on, E, on, R));
    ACCEPTED(play(no_segments, Y + 1, 0, Y, yn, U, O, on, 0, 0, R));
    REFUSED(play(no_segments, 0, 0, Y, yn, U, Y, on, E, on, R), "out overlaps packed");
    ACCEPTED(play(no_codes, T, tn, 0, 0, U, O, on, E, on, R));
    ACCEPTED(play(no_codes, T, tn, T + 1, 0, U, O, on, E, on, R));
    REFUSED(play(no_codes, T, tn, 0, 0, U, T, on, E, on, R), "out overlaps table");
    ACCEPTED(play(no_samples, T, tn, Y, yn, U, 0, 0, 0, 0, R));
    ACCEPTED(play(no_samples, T, tn, Y, yn, U, Y + 1, 0, T + 1, 0, R));
    REFUSED(play(no_samples, T, tn, Y, yn, U, Y + 1, 0, T + 1, 0, Y), "counts overlaps packed");
    REFUSED(play(no_samples, 0, tn, Y, yn, U, Y + 1, 0, T + 1, 0, R), "null");
    ACCEPTED(play(nothing, 0, 0, 0, 0, U, 0, 0, 0, 0, R));
    ACCEPTED(play(nothing, U, 0, U, 0, U, U, 0, U, 0, R));
    REFUSED(play(nothing, 0, 0, 0, 0, U, 0, 0, 0, 0, U), "counts overlaps used");
    REFUSED(play(nothing, 0, 0, 0, 0, 0, 0, 0, 0, 0, R), "null");
  }
  // a lone row: no stride is read
  const Shape one{1, 101, 2, 7, 33};
  ACCEPTED(play(one, T, 0, Y, 0, U, O, 0, E, 0, R));
  ACCEPTED(play(one, T, 20, Y, 65, U, O, 201, E, 7, R));
  REFUSED(play(one, T, 0, Y, 0, U, Y + 130, 0, E, 0, R), "out overlaps packed");
  ACCEPTED(play(one, T, 0, Y, 0, U, Y + 132, 0, E, 0, R));
}

// out and expect rows more than 2^32 codes apart: the extent runs to the end of the far row
void far_rows() {
  const int64_t far = (1ll << 32) + 37;
  const Shape s{2, 15, 1, 4, 15};
  const uint64_t extent = (uint64_t)(far + 15) * 2, F = 1ull << 40, G = 1ull << 44;   // beyond every other side
  ACCEPTED(play(s, T, 12, Y, 15, U, F, far, E, 15, R));
  ACCEPTED(play(s, T, 12, F + extent, 15, U, F, far, E, 15, R));
  REFUSED(play(s, T, 12, F + extent - 2, 15, U, F, far, E, 15, R), "out overlaps packed");
  REFUSED(play(s, T, 12, F + 74, 15, U, F, far, E, 15, R), "out overlaps packed");   // between the rows
  REFUSED(play(s, T, 12, Y, 15, U, F, far, F + 76, 15, R), "out overlaps expect");
  REFUSED(play(s, T, 12, Y, 15, U, F, far, G, far, F + extent - 8), "counts overlaps out");
  ACCEPTED(play(s, T, 12, Y, 15, U, F, far, G, far, F + extent));
  REFUSED(play(s, T, 12, Y, 15, U, 0, 0, G, far, G + extent - 8), "counts overlaps expect");
  REFUSED(play(s, T, 12, Y, 15, U, G + 80, 15, G, far, R), "out overlaps expect");
}

}  // namespace

int main() {
  clauses();
  far_rows();
  std::printf("segment play row rule ok\n");
  return 0;
}
