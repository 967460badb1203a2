// segment_row_rule_host.cpp -- the segment stage's lines of the row rule (csrc/wfk_row_rule.h; DESIGN.md "The row
// rule") held by a plain host program: no HIP, no device, addresses are plain integers and nothing is dereferenced.
// `segment` gives the rule the sides wfk_segment_rows_apply_bit / _marks give it, in their order: packed against the
// inputs, then the table against the inputs and packed, the report [count, kept] against every side.  Exit status 0
// and "segment row rule ok" when every assertion holds; the first that does not prints its line and ends with 1.
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
    if (why.find("segment rows") != 0 || !std::strstr(why.c_str(), word)) {                                     \
      std::printf("line %d: \"%s\" does not start with \"segment rows\" or lacks \"%s\"\n", __LINE__, why.c_str(), word); \
      std::exit(1);                                                                                             \
    }                                                                                                           \
  } while (0)

typedef SegmentShape Shape;

// as both applies call the rule; marks = 0: the bit form; table = packed = 0: the sizing pass
int segment(const Shape& s, uint64_t codes, int64_t codes_stride, uint64_t marks, int64_t marks_stride, uint64_t table,
            int64_t table_stride, uint64_t packed, int64_t packed_stride, uint64_t used) {
  return wfk_segment_row_rule(s, at(codes), codes_stride, at(marks), marks_stride, at(table), table_stride, at(packed),
                              packed_stride, at(used), keep);
}

const uint64_t X = 1ull << 24, M = 1ull << 25, T = 1ull << 26, Y = 1ull << 27, U = 1ull << 28;

void clauses() {
  for (const int64_t k : {(int64_t)1, (int64_t)2}) {
    const Shape s{4, 40, k, 7, 33};
    const int64_t cn = k * s.n, tn = 3 * s.max_segments, yn = k * s.capacity;
    const uint64_t c_ext = (uint64_t)(s.rows * cn) * 2, m_ext = (uint64_t)(s.rows * s.n), t_ext = (uint64_t)(s.rows * tn) * 4,
                   y_ext = (uint64_t)(s.rows * yn) * 2, rep = (uint64_t)s.rows * 16;
    for (const uint64_t marks : {(uint64_t)0, M}) {
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, U));
      ACCEPTED(segment(s, X, cn + 5, marks, s.n + 3, T, tn + 1, Y, yn + 7, U));
      ACCEPTED(segment(s, X, cn, marks, s.n, 0, 0, 0, 0, U));                        // the sizing pass
      REFUSED(segment(s, 0, cn, marks, s.n, T, tn, Y, yn, U), "null");
      REFUSED(segment(s, 0, cn, marks, s.n, 0, 0, 0, 0, U), "null");
      // aligned to their element: codes and packed to 2, the table to 4, marks anywhere
      REFUSED(segment(s, X + 1, cn, marks, s.n, T, tn, Y, yn, U), "not aligned");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y + 1, yn, U), "not aligned");
      REFUSED(segment(s, X, cn, marks, s.n, T + 2, tn, Y, yn, U), "not aligned");
      ACCEPTED(segment(s, X + 2, cn, marks, s.n, T + 4, tn, Y + 2, yn, U));
      if (marks) ACCEPTED(segment(s, X, cn, marks + 1, s.n, T, tn, Y, yn, U));
      // strides
      REFUSED(segment(s, X, cn - 1, marks, s.n, T, tn, Y, yn, U), "codes row stride smaller");
      REFUSED(segment(s, X, cn - 1, marks, s.n, 0, 0, 0, 0, U), "codes row stride smaller");
      if (marks) REFUSED(segment(s, X, cn, marks, s.n - 1, T, tn, Y, yn, U), "marks row stride smaller");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn - 1, Y, yn, U), "table row stride smaller");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn - 1, U), "packed row stride smaller");
      // no output meets an input
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, X, yn, U), "packed overlaps codes");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, X + c_ext - 2, yn, U), "packed overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, X + c_ext, yn, U));
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, X - y_ext + 2, yn, U), "packed overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, X - y_ext, yn, U));
      REFUSED(segment(s, X, cn, marks, s.n, X + c_ext - 4, tn, Y, yn, U), "table overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, X + c_ext, tn, Y, yn, U));
      REFUSED(segment(s, X, cn, marks, s.n, X - t_ext + 4, tn, Y, yn, U), "table overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, X - t_ext, tn, Y, yn, U));
      if (marks) {
        REFUSED(segment(s, X, cn, M, s.n, T, tn, M + m_ext - 2, yn, U), "packed overlaps marks");
        ACCEPTED(segment(s, X, cn, M, s.n, T, tn, M + m_ext, yn, U));
        REFUSED(segment(s, X, cn, M, s.n, M + m_ext - 4, tn, Y, yn, U), "table overlaps marks");
        ACCEPTED(segment(s, X, cn, M, s.n, M + m_ext, tn, Y, yn, U));
        ACCEPTED(segment(s, X, cn, X, s.n, T, tn, Y, yn, U));                          // the inputs may meet each other
      }
      // nor another output
      REFUSED(segment(s, X, cn, marks, s.n, Y, tn, Y, yn, U), "table overlaps packed");
      REFUSED(segment(s, X, cn, marks, s.n, Y + y_ext - 4, tn, Y, yn, U), "table overlaps packed");
      ACCEPTED(segment(s, X, cn, marks, s.n, Y + y_ext, tn, Y, yn, U));
      REFUSED(segment(s, X, cn, marks, s.n, Y - t_ext + 4, tn, Y, yn, U), "table overlaps packed");
      ACCEPTED(segment(s, X, cn, marks, s.n, Y - t_ext, tn, Y, yn, U));
      // used: rows x 2 int64, aligned to 8, meets no side
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, U + 4), "counts are not aligned");
      REFUSED(segment(s, X, cn, marks, s.n, 0, 0, 0, 0, U + 4), "counts are not aligned");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, X + c_ext - 8), "counts overlaps codes");
      REFUSED(segment(s, X, cn, marks, s.n, 0, 0, 0, 0, X + c_ext - 8), "counts overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, X + c_ext));
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, X - rep + 8), "counts overlaps codes");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, X - rep));
      if (marks) REFUSED(segment(s, X, cn, M, s.n, T, tn, Y, yn, M + 8), "counts overlaps marks");
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, Y + y_ext - 8), "counts overlaps packed");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, Y + y_ext));
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, T + t_ext - 8), "counts overlaps table");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, T + t_ext));
      REFUSED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, T - rep + 8), "counts overlaps table");
      ACCEPTED(segment(s, X, cn, marks, s.n, T, tn, Y, yn, T - rep));
      // the earlier clause speaks
      REFUSED(segment(s, 0, cn, marks, s.n, T, tn, Y, yn, U + 4), "counts are not aligned");
      REFUSED(segment(s, 0, cn, marks, s.n, T, tn, Y + 1, yn, U), "null");
      REFUSED(segment(s, X + 1, cn - 1, marks, s.n, T, tn, Y, yn, U), "not aligned");
      REFUSED(segment(s, X, cn - 1, marks, s.n, T, tn, X, yn, U), "stride smaller");
    }
    // a side that holds nothing is not looked at: it may be null, misaligned or anywhere
    const Shape no_table{4, 40, k, 0, 33}, no_packed{4, 40, k, 7, 0}, neither{4, 40, k, 0, 0};
    ACCEPTED(segment(no_table, X, cn, M, 40, 0, 0, Y, yn, U));
    ACCEPTED(segment(no_table, X, cn, M, 40, X + 1, 0, Y, yn, U));
    REFUSED(segment(no_table, X, cn, M, 40, 0, 0, X, yn, U), "packed overlaps codes");
    ACCEPTED(segment(no_packed, X, cn, M, 40, T, tn, 0, 0, U));
    ACCEPTED(segment(no_packed, X, cn, M, 40, T, tn, X + 1, 0, U));
    REFUSED(segment(no_packed, X, cn, M, 40, X, tn, 0, 0, U), "table overlaps codes");
    ACCEPTED(segment(neither, X, cn, M, 40, X, 0, X, 0, U));
    REFUSED(segment(neither, X, cn, M, 40, X, 0, X, 0, X), "counts overlaps");
  }
  // a lone row: no stride is read
  const Shape one{1, 40, 2, 7, 33};
  ACCEPTED(segment(one, X, 0, M, 0, T, 0, Y, 0, U));
  ACCEPTED(segment(one, X, 79, M, 39, T, 20, Y, 65, U));
  REFUSED(segment(one, X, 0, M, 0, T, 0, X + 158, 0, U), "packed overlaps codes");
  ACCEPTED(segment(one, X, 0, M, 0, T, 0, X + 160, 0, U));
}

// rows more than 2^32 codes apart: the extent runs to the end of the far row
void far_rows() {
  const int64_t far = (1ll << 32) + 37;
  const Shape s{2, 15, 1, 4, 15};
  const uint64_t extent = (uint64_t)(far + 15) * 2, F = 1ull << 40;   // the codes: beyond every other side
  ACCEPTED(segment(s, F, far, 0, 0, T, 12, F + extent, 15, U));
  REFUSED(segment(s, F, far, 0, 0, T, 12, F + extent - 2, 15, U), "packed overlaps codes");
  REFUSED(segment(s, F, far, 0, 0, T, 12, F + 74, 15, U), "packed overlaps codes");    // between the rows
  REFUSED(segment(s, F, far, 0, 0, T, 12, Y, 15, F + extent - 8), "counts overlaps codes");
  ACCEPTED(segment(s, F, far, 0, 0, T, 12, Y, 15, F + extent));
}

}  // namespace

int main() {
  clauses();
  far_rows();
  std::printf("segment row rule ok\n");
  return 0;
}
