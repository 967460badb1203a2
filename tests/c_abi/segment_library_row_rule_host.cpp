// segment_library_row_rule_host.cpp -- the segment library's lines of the row rule (csrc/wfk_row_rule.h; DESIGN.md
// "The row rule") held by a plain host program: no HIP, no device, addresses are plain integers and nothing is
// dereferenced.  `library` gives the rule the sides wfk_segment_library_apply gives it, in its order: the library
// against the inputs, plays against the inputs and the library, slots against all of them, the report [unique,
// lib_kept] against every side.  Exit status 0 and "segment library row rule ok" when every assertion holds; the first
// that does not prints its line and ends with 1.
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
    if (why.find("segment library") != 0 || !std::strstr(why.c_str(), word)) {                                  \
      std::printf("line %d: \"%s\" does not start with \"segment library\" or lacks \"%s\"\n", __LINE__, why.c_str(), word); \
      std::exit(1);                                                                                             \
    }                                                                                                           \
  } while (0)

typedef SegmentLibraryShape Shape;

// as the apply calls the rule; plays, slots, library = 0: that output is not written; all three: the sizing pass
int library(const Shape& s, uint64_t table, int64_t table_stride, uint64_t packed, int64_t packed_stride, uint64_t used,
            uint64_t plays, int64_t plays_stride, uint64_t slots, int64_t slots_stride, uint64_t lib, int64_t lib_stride,
            uint64_t lib_used) {
  return wfk_segment_library_row_rule(s, at(table), table_stride, at(packed), packed_stride, at(used), at(plays),
                                      plays_stride, at(slots), slots_stride, at(lib), lib_stride, at(lib_used), keep);
}

const uint64_t T = 1ull << 24, Y = 1ull << 25, U = 1ull << 26, P = 1ull << 27, S = 1ull << 28, L = 1ull << 29,
               R = 1ull << 30;

void clauses() {
  for (const int64_t k : {(int64_t)1, (int64_t)2}) {
    const Shape s{4, k, 7, 33, 21};
    const int64_t tn = 3 * s.max_segments, sn = s.max_segments, yn = k * s.capacity, ln = k * s.lib_capacity;
    const uint64_t t_ext = (uint64_t)(s.rows * tn) * 4, y_ext = (uint64_t)(s.rows * yn) * 2, u_ext = (uint64_t)s.rows * 16,
                   s_ext = (uint64_t)(s.rows * sn) * 4, l_ext = (uint64_t)(s.rows * ln) * 2, rep = u_ext;
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, R));
    ACCEPTED(library(s, T, tn + 3, Y, yn + 5, U, P, tn + 1, S, sn + 2, L, ln + 7, R));
    ACCEPTED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, R));                        // the sizing pass
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, 0, 0, 0, 0, R));                       // each output alone
    ACCEPTED(library(s, T, tn, Y, yn, U, 0, 0, S, sn, 0, 0, R));
    ACCEPTED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, L, ln, R));
    // an input that holds something is there, in every form of the apply
    REFUSED(library(s, 0, tn, Y, yn, U, P, tn, S, sn, L, ln, R), "null");
    REFUSED(library(s, T, tn, 0, yn, U, P, tn, S, sn, L, ln, R), "null");
    REFUSED(library(s, T, tn, Y, yn, 0, P, tn, S, sn, L, ln, R), "null");
    REFUSED(library(s, 0, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, R), "null");
    REFUSED(library(s, T, tn, 0, yn, U, 0, 0, S, sn, 0, 0, R), "null");
    // aligned to their element: codes to 2, tables to 4, used to 8
    REFUSED(library(s, T + 2, tn, Y, yn, U, P, tn, S, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn, Y + 1, yn, U, P, tn, S, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn, Y, yn, U + 4, P, tn, S, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn, Y, yn, U, P + 2, tn, S, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S + 2, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L + 1, ln, R), "not aligned");
    REFUSED(library(s, T + 2, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, R), "not aligned");
    ACCEPTED(library(s, T + 4, tn, Y + 2, yn, U + 8, P + 4, tn, S + 4, sn, L + 2, ln, R + 8));
    // strides
    REFUSED(library(s, T, tn - 1, Y, yn, U, P, tn, S, sn, L, ln, R), "table row stride smaller");
    REFUSED(library(s, T, tn, Y, yn - 1, U, P, tn, S, sn, L, ln, R), "packed row stride smaller");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn - 1, S, sn, L, ln, R), "plays row stride smaller");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn - 1, L, ln, R), "slots row stride smaller");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln - 1, R), "library row stride smaller");
    REFUSED(library(s, T, tn - 1, Y, yn, U, 0, 0, 0, 0, 0, 0, R), "table row stride smaller");
    // no output meets an input
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, Y, ln, R), "library overlaps packed");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, Y + y_ext - 2, ln, R), "library overlaps packed");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, Y + y_ext, ln, R));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, Y - l_ext + 2, ln, R), "library overlaps packed");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, Y - l_ext, ln, R));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, T + t_ext - 2, ln, R), "library overlaps table");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, U + u_ext - 2, ln, R), "library overlaps used");
    REFUSED(library(s, T, tn, Y, yn, U, T, tn, S, sn, L, ln, R), "plays overlaps table");
    REFUSED(library(s, T, tn, Y, yn, U, T + t_ext - 4, tn, S, sn, L, ln, R), "plays overlaps table");
    ACCEPTED(library(s, T, tn, Y, yn, U, T + t_ext, tn, S, sn, L, ln, R));
    REFUSED(library(s, T, tn, Y, yn, U, Y + y_ext - 4, tn, S, sn, L, ln, R), "plays overlaps packed");
    REFUSED(library(s, T, tn, Y, yn, U, U + 8, tn, S, sn, L, ln, R), "plays overlaps used");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, T + t_ext - 4, sn, L, ln, R), "slots overlaps table");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, Y - s_ext + 4, sn, L, ln, R), "slots overlaps packed");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, Y - s_ext, sn, L, ln, R));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, U + u_ext - 4, sn, L, ln, R), "slots overlaps used");
    REFUSED(library(s, T, tn, Y, yn, U, 0, 0, T, sn, 0, 0, R), "slots overlaps table");   // alone, too
    ACCEPTED(library(s, T, tn, T, yn, U, P, tn, S, sn, L, ln, R));                        // the inputs may meet each other
    // nor another output
    REFUSED(library(s, T, tn, Y, yn, U, L, tn, S, sn, L, ln, R), "plays overlaps library");
    REFUSED(library(s, T, tn, Y, yn, U, L + l_ext - 4, tn, S, sn, L, ln, R), "plays overlaps library");
    ACCEPTED(library(s, T, tn, Y, yn, U, L + l_ext, tn, S, sn, L, ln, R));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, L + l_ext - 4, sn, L, ln, R), "slots overlaps library");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, P, sn, L, ln, R), "slots overlaps plays");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, P + t_ext - 4, sn, L, ln, R), "slots overlaps plays");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, P + t_ext, sn, L, ln, R));
    ACCEPTED(library(s, T, tn, Y, yn, U, 0, 0, L, sn, 0, 0, R));                          // an output that is not given
    // lib_used: rows x 2 int64, aligned to 8, meets no side
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, R + 4), "counts are not aligned");
    REFUSED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, R + 4), "counts are not aligned");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, T + t_ext - 8), "counts overlaps table");
    REFUSED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, T + t_ext - 8), "counts overlaps table");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, T + t_ext));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, T - rep + 8), "counts overlaps table");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, T - rep));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, Y + y_ext - 8), "counts overlaps packed");
    REFUSED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, Y + 8), "counts overlaps packed");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, U), "counts overlaps used");
    REFUSED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, U + u_ext - 8), "counts overlaps used");
    ACCEPTED(library(s, T, tn, Y, yn, U, 0, 0, 0, 0, 0, 0, U + u_ext));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, P + 8), "counts overlaps plays");
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, S + s_ext - 8), "counts overlaps slots");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, S + s_ext));
    REFUSED(library(s, T, tn, Y, yn, U, P, tn, S, sn, L, ln, L + l_ext - 8), "counts overlaps library");
    ACCEPTED(library(s, T, tn, Y, yn, U, P, tn, S, sn, 0, 0, L));                         // where no library is given
    // the earlier clause speaks
    REFUSED(library(s, 0, tn, Y, yn, U, P, tn, S, sn, L, ln, R + 4), "counts are not aligned");
    REFUSED(library(s, 0, tn, Y + 1, yn, U, P, tn, S, sn, L, ln, R), "null");
    REFUSED(library(s, T + 2, tn - 1, Y, yn, U, P, tn, S, sn, L, ln, R), "not aligned");
    REFUSED(library(s, T, tn - 1, Y, yn, U, P, tn, S, sn, Y, ln, R), "stride smaller");
    // a side that holds nothing is not looked at: it may be null, misaligned or anywhere
    const Shape no_segments{4, k, 0, 33, 21}, no_codes{4, k, 7, 0, 0}, no_room{4, k, 7, 33, 0}, nothing{4, k, 0, 0, 0};
    ACCEPTED(library(no_segments, 0, 0, Y, yn, U, 0, 0, 0, 0, L, ln, R));
    ACCEPTED(library(no_segments, Y + 1, 0, Y, yn, U, Y + 1, 0, Y + 1, 0, L, ln, R));
    REFUSED(library(no_segments, 0, 0, Y, yn, U, 0, 0, 0, 0, Y, ln, R), "library overlaps packed");
    ACCEPTED(library(no_codes, T, tn, 0, 0, U, P, tn, S, sn, 0, 0, R));
    ACCEPTED(library(no_codes, T, tn, T + 1, 0, U, P, tn, S, sn, T + 1, 0, R));
    REFUSED(library(no_codes, T, tn, 0, 0, U, T, tn, S, sn, 0, 0, R), "plays overlaps table");
    ACCEPTED(library(no_room, T, tn, Y, yn, U, P, tn, S, sn, Y + 1, 0, R));
    REFUSED(library(no_room, T, tn, Y, yn, U, P, tn, Y, sn, Y + 1, 0, R), "slots overlaps packed");
    ACCEPTED(library(nothing, 0, 0, 0, 0, U, 0, 0, 0, 0, 0, 0, R));
    ACCEPTED(library(nothing, U, 0, U, 0, U, U, 0, U, 0, U, 0, R));
    REFUSED(library(nothing, 0, 0, 0, 0, U, 0, 0, 0, 0, 0, 0, U), "counts overlaps used");
    REFUSED(library(nothing, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, R), "null");
  }
  // a lone row: no stride is read
  const Shape one{1, 2, 7, 33, 21};
  ACCEPTED(library(one, T, 0, Y, 0, U, P, 0, S, 0, L, 0, R));
  ACCEPTED(library(one, T, 20, Y, 65, U, P, 20, S, 6, L, 41, R));
  REFUSED(library(one, T, 0, Y, 0, U, P, 0, S, 0, Y + 130, 0, R), "library overlaps packed");
  ACCEPTED(library(one, T, 0, Y, 0, U, P, 0, S, 0, Y + 132, 0, R));
}

// packed rows more than 2^32 codes apart: the extent runs to the end of the far row
void far_rows() {
  const int64_t far = (1ll << 32) + 37;
  const Shape s{2, 1, 4, 15, 15};
  const uint64_t extent = (uint64_t)(far + 15) * 2, F = 1ull << 40;   // packed: beyond every other side
  ACCEPTED(library(s, T, 12, F, far, U, P, 12, S, 4, F + extent, 15, R));
  REFUSED(library(s, T, 12, F, far, U, P, 12, S, 4, F + extent - 2, 15, R), "library overlaps packed");
  REFUSED(library(s, T, 12, F, far, U, P, 12, S, 4, F + 74, 15, R), "library overlaps packed");   // between the rows
  REFUSED(library(s, T, 12, F, far, U, P, 12, F + 76, 4, L, 15, R), "slots overlaps packed");
  REFUSED(library(s, T, 12, F, far, U, P, 12, S, 4, L, 15, F + extent - 8), "counts overlaps packed");
  ACCEPTED(library(s, T, 12, F, far, U, P, 12, S, 4, L, 15, F + extent));
}

}  // namespace

int main() {
  clauses();
  far_rows();
  std::printf("segment library row rule ok\n");
  return 0;
}
