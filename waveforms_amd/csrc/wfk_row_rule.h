// wfk_row_rule.h -- the row rule of every apply (DESIGN.md "The row rule") as integer arithmetic on addresses: no
// HIP, no device, no state, so a plain C++ program holds it to its table (tests/c_abi/row_rule_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "wfk.h"

namespace {

// do the half-open byte ranges [a, a + bytes_a) and [b, b + bytes_b) meet
inline bool wfk_ranges_overlap(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bytes_b && b0 < a0 + bytes_a;
}

// One side of an apply: `rows` rows of `n` elements of `es` bytes, `stride` elements apart.  The sides of one apply
// may differ in all of these.
struct RowSide {
  const char* what;   // its name in a refusal: "in", "out", "codes", ...
  const void* ptr;
  int64_t rows, stride, n;
  size_t es;
  bool lone_stride = true;   // is the stride of a single row held to n (no kernel reads it: dac and marker let it pass)
  // the bytes from the first element of row 0 to the END of row rows - 1 -- not rows * stride
  size_t bytes() const { return ((size_t)(rows - 1) * (size_t)stride + (size_t)n) * es; }
  bool meets(const void* p, size_t b) const { return wfk_ranges_overlap(ptr, bytes(), p, b); }
};

// What a counting stage writes next to its output: rows x counters contiguous int64 (ptr null: it does not count)
struct RowReport {
  const void* ptr = nullptr;
  int64_t rows = 0, counters = 0;
  size_t bytes() const { return (size_t)rows * (size_t)counters * sizeof(int64_t); }
};

// the clauses a stage may leave out: every side starts at a multiple of its element size; `out` meets no input
enum : unsigned { kRowsAligned = 1, kRowsDisjoint = 2 };

// Every refusal is WFK_EINVAL with a text that names the stage first, handed to `fail` (code, text) -> code: wfk_fail
// of wfk_host.h in the library.

// what remains of the rule for rows of no elements: a report that is there starts at a multiple of 8
template <typename Fail>
int wfk_report_rule(const char* stage, const RowReport& report, Fail&& fail) {
  if (!((uintptr_t)report.ptr & 7)) return WFK_OK;
  return fail(WFK_EINVAL, std::string(stage) + ": counts are not aligned to int64");
}

// The rule, after the apply's own `null plan` / `n == 0` exits, clause by clause in this order: the report's alignment;
// no null side; (kRowsAligned) every side aligned to its element; every stride >= that side's own n, but for a single
// row with lone_stride off; (kRowsDisjoint) `out` meets no side of `in`; the report meets no side.  An apply without
// an input gives `out` as its input.
template <typename Fail>
int wfk_row_rule(const char* stage, std::initializer_list<RowSide> in, const RowSide& out, unsigned clauses,
                 Fail&& fail, const RowReport& report = RowReport()) {
  if (const int rc = wfk_report_rule(stage, report, fail)) return rc;
  const auto refuse = [&](const std::string& text) { return fail(WFK_EINVAL, stage + text); };
  const auto sides = [&](auto&& f) {   // the inputs, then `out`
    for (const RowSide& s : in) f(s);
    f(out);
  };
  bool null = false, misaligned = false;
  const RowSide *narrow = nullptr, *counted = nullptr;   // the first side with a stride below its n / under the report
  std::string names;
  sides([&](const RowSide& s) {
    null = null || !s.ptr;
    misaligned = misaligned || ((uintptr_t)s.ptr & (s.es - 1));
    if (!narrow && s.stride < s.n && (s.rows > 1 || s.lone_stride)) narrow = &s;
    if (!counted && report.ptr && s.meets(report.ptr, report.bytes())) counted = &s;
    names += std::string(names.empty() ? "" : " / ") + s.what;
  });
  if (null) return refuse(": null " + names + " buffer");
  if ((clauses & kRowsAligned) && misaligned) return refuse(": rows are not aligned to their element");
  if (narrow)
    return refuse(std::string(": ") + narrow->what + " row stride smaller than n (" + std::to_string(narrow->stride) +
                  " < " + std::to_string(narrow->n) + ")");
  for (const RowSide& s : in) {
    if ((clauses & kRowsDisjoint) && s.meets(out.ptr, out.bytes()))
      return refuse(std::string(" is out of place: ") + out.what + " overlaps " + s.what);
  }
  if (counted) return refuse(std::string(": counts overlaps ") + counted->what);
  return WFK_OK;
}

// The segment stage has two inputs and two outputs next to its report `used` (rows x [count, kept]): `rows` rows of
// k n codes, of n marks (marks null: the bit form, which reads the codes alone), of 3 max_segments int32 and of
// k capacity codes.  table = packed = null is the sizing pass: the inputs and the report alone.  A side that holds
// nothing (max_segments = 0, capacity = 0) is not looked at.  The rule runs once per output: packed against the
// inputs, then the table against the inputs and packed; the report meets no side.
struct SegmentShape { int64_t rows, n, k, max_segments, capacity; };
template <typename Fail>
int wfk_segment_row_rule(const SegmentShape& s, const void* codes, int64_t codes_stride, const void* marks,
                         int64_t marks_stride, const void* table, int64_t table_stride, const void* packed,
                         int64_t packed_stride, const void* used, Fail&& fail) {
  const char* stage = "segment rows";
  const bool sizing = !table && !packed;
  const bool has_table = !sizing && s.max_segments > 0, has_packed = !sizing && s.capacity > 0;
  const RowReport report{used, s.rows, 2};
  const RowSide c{"codes", codes, s.rows, codes_stride, s.k * s.n, sizeof(int16_t), false};
  const RowSide m = marks ? RowSide{"marks", marks, s.rows, marks_stride, s.n, sizeof(uint8_t), false} : c;
  const RowSide y{"packed", packed, s.rows, packed_stride, s.k * s.capacity, sizeof(int16_t), false};
  const RowSide t{"table", table, s.rows, table_stride, 3 * s.max_segments, sizeof(int32_t), false};
  if (has_packed) {
    if (const int rc = wfk_row_rule(stage, {c, m}, y, kRowsAligned | kRowsDisjoint, fail, report)) return rc;
  }
  if (has_table) {
    if (const int rc = wfk_row_rule(stage, {c, m, has_packed ? y : c}, t, kRowsAligned | kRowsDisjoint, fail, report))
      return rc;
  }
  if (!has_packed && !has_table) return wfk_row_rule(stage, {m}, c, kRowsAligned, fail, report);
  return WFK_OK;
}

// The segment library reads what the segment stage wrote -- `rows` rows of 3 max_segments int32 (table), of k capacity
// codes (packed) and the contiguous rows x [count, kept] int64 (used) -- and has three outputs next to its report
// `lib_used` (rows x [unique, lib_kept]): rows of 3 max_segments int32 (plays), of max_segments int32 (slots) and of
// k lib_capacity codes (library).  An output that is null is not written; all three null is the sizing pass: the
// inputs and the report alone.  A side that holds nothing (max_segments = 0, capacity = 0, lib_capacity = 0) is not
// looked at.  The rule runs once per output: the library against the inputs, then plays against the inputs and the
// library, then slots against all of them; the report meets no side.
struct SegmentLibraryShape { int64_t rows, k, max_segments, capacity, lib_capacity; };
template <typename Fail>
int wfk_segment_library_row_rule(const SegmentLibraryShape& s, const void* table, int64_t table_stride,
                                 const void* packed, int64_t packed_stride, const void* used, const void* plays,
                                 int64_t plays_stride, const void* slots, int64_t slots_stride, const void* library,
                                 int64_t library_stride, const void* lib_used, Fail&& fail) {
  const char* stage = "segment library";
  const bool has_plays = plays && s.max_segments > 0, has_slots = slots && s.max_segments > 0;
  const bool has_library = library && s.lib_capacity > 0;
  const RowReport report{lib_used, s.rows, 2};
  const RowSide u{"used", used, s.rows, 2, 2, sizeof(int64_t), false};
  const RowSide t = s.max_segments > 0 ? RowSide{"table", table, s.rows, table_stride, 3 * s.max_segments,
                                                 sizeof(int32_t), false} : u;
  const RowSide y = s.capacity > 0 ? RowSide{"packed", packed, s.rows, packed_stride, s.k * s.capacity,
                                             sizeof(int16_t), false} : u;
  const RowSide l = has_library ? RowSide{"library", library, s.rows, library_stride, s.k * s.lib_capacity,
                                          sizeof(int16_t), false} : u;
  const RowSide p = has_plays ? RowSide{"plays", plays, s.rows, plays_stride, 3 * s.max_segments, sizeof(int32_t),
                                        false} : u;
  const RowSide o{"slots", slots, s.rows, slots_stride, s.max_segments, sizeof(int32_t), false};
  if (has_library) {
    if (const int rc = wfk_row_rule(stage, {t, y, u}, l, kRowsAligned | kRowsDisjoint, fail, report)) return rc;
  }
  if (has_plays) {
    if (const int rc = wfk_row_rule(stage, {t, y, u, l}, p, kRowsAligned | kRowsDisjoint, fail, report)) return rc;
  }
  if (has_slots) {
    if (const int rc = wfk_row_rule(stage, {t, y, u, l, p}, o, kRowsAligned | kRowsDisjoint, fail, report)) return rc;
  }
  if (!has_library && !has_plays && !has_slots) return wfk_row_rule(stage, {t, y}, u, kRowsAligned, fail, report);
  return WFK_OK;
}

// The segment player reads a table, a waveform memory and the totals as the two stages above write them -- `rows` rows
// of 3 max_segments int32 (table), of k capacity codes (packed) and the contiguous rows x [count, kept] int64 (used) --
// and, where it is given, `expect`, rows of k n codes.  It has one output, `out`, rows of k n codes, next to its
// report (rows x [played, differ, stray, first]).  out null: the verifying pass (expect given) or the checking pass
// (neither): the inputs and the report alone.  A side that holds nothing (max_segments = 0, capacity = 0; n = 0 for
// out and expect) is not looked at.  out meets no input, expect among them; the report meets no side.
struct SegmentPlayShape { int64_t rows, n, k, max_segments, capacity; };
template <typename Fail>
int wfk_segment_play_row_rule(const SegmentPlayShape& s, const void* table, int64_t table_stride, const void* packed,
                              int64_t packed_stride, const void* used, const void* out, int64_t out_stride,
                              const void* expect, int64_t expect_stride, const void* report_ptr, Fail&& fail) {
  const char* stage = "segment play";
  const bool has_out = out && s.n > 0, has_expect = expect && s.n > 0;
  const RowReport report{report_ptr, s.rows, 4};
  const RowSide u{"used", used, s.rows, 2, 2, sizeof(int64_t), false};
  const RowSide t = s.max_segments > 0 ? RowSide{"table", table, s.rows, table_stride, 3 * s.max_segments,
                                                 sizeof(int32_t), false} : u;
  const RowSide y = s.capacity > 0 ? RowSide{"packed", packed, s.rows, packed_stride, s.k * s.capacity,
                                             sizeof(int16_t), false} : u;
  const RowSide e = has_expect ? RowSide{"expect", expect, s.rows, expect_stride, s.k * s.n, sizeof(int16_t), false}
                               : u;
  const RowSide o{"out", out, s.rows, out_stride, s.k * s.n, sizeof(int16_t), false};
  if (has_out) return wfk_row_rule(stage, {t, y, u, e}, o, kRowsAligned | kRowsDisjoint, fail, report);
  return wfk_row_rule(stage, {t, y, e}, u, kRowsAligned, fail, report);
}

}  // namespace
