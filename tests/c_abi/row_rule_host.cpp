// row_rule_host.cpp -- the row rule of csrc/wfk_row_rule.h held to its table (DESIGN.md "The row rule") by a plain
// host program: no HIP, no device, addresses are plain integers and nothing is dereferenced.  Each stage below gives
// the rule the sides its apply gives it.  Exit status 0 and "row rule ok" when every assertion holds; the first
// one that does not prints its line and ends the program with status 1.
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
int keep(int code, const std::string& text) {   // the program's wfk_fail
  why = text;
  return code;
}

// accepted / refused with WFK_EINVAL, the stage named and `word` in the text
#define ACCEPTED(call) HOLD((call) == WFK_OK)
#define REFUSED(call, stage, word)                                                                              \
  do {                                                                                                          \
    why.clear();                                                                                                \
    HOLD((call) == WFK_EINVAL);                                                                                 \
    if (why.find(stage) != 0 || !std::strstr(why.c_str(), word)) {                                              \
      std::printf("line %d: \"%s\" does not start with \"%s\" or lacks \"%s\"\n", __LINE__, why.c_str(), stage, word); \
      std::exit(1);                                                                                             \
    }                                                                                                           \
  } while (0)

// ---- the stages, as their applies call the rule -------------------------------------------------------------------

// wfk_check_rows of wfk_host.h: FIR, IIR, spectral rows, shift rows, ... -- one n, one element size, no alignment clause
int plain(uint64_t in, int64_t in_rows, int64_t in_stride, uint64_t out, int64_t out_rows, int64_t out_stride, int64_t n,
          size_t es, bool disjoint) {
  return wfk_row_rule("FIR", {{"in", at(in), in_rows, in_stride, n, es}}, {"out", at(out), out_rows, out_stride, n, es},
                      disjoint ? kRowsDisjoint : 0u, keep);
}

int dac(uint64_t in, int64_t in_stride, uint64_t out, int64_t out_stride, uint64_t counts, int64_t batch, int64_t k,
        int64_t n, size_t es) {
  return wfk_row_rule("dac rows", {{"in", at(in), batch, in_stride, n, es}},
                      {"out", at(out), batch / k, out_stride, k * n, 2, false}, kRowsAligned | kRowsDisjoint, keep,
                      RowReport{at(counts), batch, 3});
}

int marker(uint64_t in, int64_t in_stride, uint64_t out, int64_t out_stride, bool into_codes, uint64_t counts,
           int64_t batch, int64_t k, int64_t n, size_t es) {
  const int64_t rows = batch / k;
  const RowSide o = into_codes ? RowSide{"codes", at(out), rows, out_stride, k * n, 2, false}
                               : RowSide{"out", at(out), rows, out_stride, n, 1, false};
  return wfk_row_rule("marker rows", {{"in", at(in), batch, in_stride, n, es}}, o, kRowsAligned | kRowsDisjoint, keep,
                      RowReport{at(counts), rows, 2});
}

int mix(uint64_t in, int64_t rows_in, int64_t in_stride, uint64_t out, int64_t rows_out, int64_t out_stride, int64_t n,
        size_t es) {
  return wfk_row_rule("mix rows", {{"in", at(in), rows_in, in_stride, n, es}},
                      {"out", at(out), rows_out, out_stride, n, es}, kRowsAligned | kRowsDisjoint, keep);
}

int extract(uint64_t sig_in, int64_t in_rows, int64_t in_stride, uint64_t sig_out, int64_t out_sig_stride, uint64_t ker,
            int64_t ker_stride, int64_t batch, int64_t n, int64_t K) {
  return wfk_row_rule("extract rows",
                      {{"sig_in", at(sig_in), in_rows, in_stride, n, 8}, {"sig_out", at(sig_out), batch, out_sig_stride, n, 8}},
                      {"ker", at(ker), batch, ker_stride, K, 8}, kRowsAligned | kRowsDisjoint, keep);
}

// ---- the extents: tests/test_rows_cpu.py::test_disjointness, the two sides differing in everything ---------------

bool meet(const RowSide& a, const RowSide& b) {
  const bool ab = a.meets(b.ptr, b.bytes()), ba = b.meets(a.ptr, a.bytes());
  HOLD(ab == ba);   // either way round
  return ab;
}

void extents() {
  const uint64_t base = 1ull << 20;
  const size_t sizes[4][2] = {{8, 2}, {4, 2}, {8, 1}, {4, 1}};
  const int64_t ns[] = {1000, 5, 1};
  for (const auto& es : sizes) {
    for (const int64_t n : ns) {
      // a: 8 rows of n elements of 8 / 4 bytes; b: 3 rows of 2 n elements of 2 / 1 bytes
      const auto A = [&](uint64_t p, int64_t stride) { return RowSide{"a", at(p), 8, stride, n, es[0]}; };
      const auto B = [&](uint64_t p, int64_t stride) { return RowSide{"b", at(p), 3, stride, 2 * n, es[1]}; };
      const uint64_t ext_a = (uint64_t)(7 * n + n) * es[0], ext_b = (uint64_t)(2 * 2 * n + 2 * n) * es[1];
      HOLD(A(base, n).bytes() == ext_a && B(base, 2 * n).bytes() == ext_b);
      // the same start, one row on, 8 bytes on, one shared element at either end
      const uint64_t shifts[] = {0, (uint64_t)n * es[0], 8, ext_a - es[1]};
      for (const uint64_t shift : shifts)
        if (shift < ext_a) HOLD(meet(A(base, n), B(base + shift, 2 * n)));
      HOLD(meet(A(base, n), B(base - ext_b + es[1], 2 * n)));
      // only touching, on either side, and apart
      HOLD(!meet(A(base, n), B(base + ext_a, 2 * n)));
      HOLD(!meet(A(base, n), B(base - ext_b, 2 * n)));
      HOLD(!meet(A(base, n), B(base + ext_a + es[1], 2 * n)));
      HOLD(!meet(A(base, n), B(base - ext_b - es[0], 2 * n)));
      // strided rows: an extent runs to the END of the last row, not to rows * stride
      const int64_t sa = n + 7, sb = 2 * n + 5;
      const uint64_t end_a = (uint64_t)(7 * sa + n) * es[0], end_b = (uint64_t)(2 * sb + 2 * n) * es[1];
      HOLD(A(base, sa).bytes() == end_a && end_a < (uint64_t)(8 * sa) * es[0]);
      HOLD(B(base, sb).bytes() == end_b && end_b < (uint64_t)(3 * sb) * es[1]);
      HOLD(meet(A(base, sa), B(base + end_a - es[1], sb)));
      HOLD(!meet(A(base, sa), B(base + end_a, sb)));
      HOLD(meet(A(base, sa), B(base - end_b + es[1], sb)));
      HOLD(!meet(A(base, sa), B(base - end_b, sb)));
    }
  }
}

// ---- rows more than 2^32 elements apart (FAR_STRIDE of tests/row_windows.py) --------------------------------------

void far_rows() {
  const int64_t far = (1ll << 32) + 37, n = 15;
  const uint64_t base = 1ull << 21;
  const size_t sizes[] = {8, 4, 2};
  for (const size_t es : sizes) {
    const RowSide rows{"far", at(base), 2, far, n, es};
    const uint64_t extent = (uint64_t)(far + n) * es;
    HOLD(rows.bytes() == extent && extent > (1ull << 32) * es);
    // row 1 starts far * es bytes on: a range at the offset a 32-bit product gives (296 for 8-byte elements) is not in it
    const uint64_t cut = (uint32_t)((uint64_t)far * es);
    HOLD(es != 8 || cut == 296);
    const RowSide row1{"row 1", at(base + extent - (uint64_t)n * es), 1, n, n, es};
    HOLD(row1.ptr == at(base + (uint64_t)far * es));
    HOLD(!row1.meets(at(base + cut), (size_t)n * es));
    HOLD(row1.meets(at(base + (uint64_t)far * es + (uint64_t)(n - 1) * es), es));
    // the extent is one range: what lies between the two rows meets it, what starts at its end does not
    HOLD(rows.meets(at(base + cut), es) && rows.meets(at(base + extent - es), es));
    HOLD(!rows.meets(at(base + extent), es) && !rows.meets(at(base - es), es));
    // through the rule: out of place against a near batch that touches the far one, refused one element earlier
    ACCEPTED(mix(base, 2, far, base + extent, 3, n, n, es));
    REFUSED(mix(base, 2, far, base + extent - es, 3, n, n, es), "mix rows", "overlaps");
    ACCEPTED(mix(base + 3 * n * es, 2, far, base, 3, n, n, es));
    REFUSED(mix(base + 3 * n * es - es, 2, far, base, 3, n, n, es), "mix rows", "overlaps");
    REFUSED(mix(base, 2, far, base + cut, 1, n, n, es), "mix rows", "overlaps");   // between the rows: in the extent
  }
}

// ---- every clause of the table, stage by stage ----------------------------------------------------------------

const uint64_t X = 1ull << 24, Y = 1ull << 25, C = 1ull << 26;   // in, out, counts: far apart, aligned to anything

void plain_clauses() {
  const int64_t n = 40, rows = 4;
  for (const size_t es : {(size_t)8, (size_t)4}) {
    ACCEPTED(plain(X, rows, n, Y, rows, n, n, es, true));
    REFUSED(plain(0, rows, n, Y, rows, n, n, es, true), "FIR", "null in / out");
    REFUSED(plain(X, rows, n, 0, rows, n, n, es, true), "FIR", "null in / out");
    ACCEPTED(plain(X + 1, rows, n, Y + 3, rows, n, n, es, true));                 // no alignment clause
    REFUSED(plain(X, rows, n - 1, Y, rows, n, n, es, false), "FIR", "in row stride smaller than n");
    REFUSED(plain(X, rows, n, Y, rows, n - 1, n, es, false), "FIR", "out row stride smaller than n");
    REFUSED(plain(X, 1, n - 1, Y, rows, n, n, es, false), "FIR", "stride smaller");   // a lone row's stride counts
    REFUSED(plain(X, rows, n, Y, 1, n - 1, n, es, false), "FIR", "stride smaller");
    ACCEPTED(plain(X, rows, n, X, rows, n, n, es, false));                          // in place
    REFUSED(plain(X, rows, n, X, rows, n, n, es, true), "FIR", "FIR is out of place: out overlaps in");
    const uint64_t extent = (uint64_t)(rows * n) * es;
    REFUSED(plain(X, rows, n, X + extent - 1, rows, n, n, es, true), "FIR", "overlaps");
    ACCEPTED(plain(X, rows, n, X + extent, rows, n, n, es, true));
    ACCEPTED(plain(X, 1, n, X + n * es, rows, n, n, es, true));                     // one shared input row
    REFUSED(plain(X, 1, n, X + n * es - 1, rows, n, n, es, true), "FIR", "overlaps");
    REFUSED(plain(0, rows, n - 1, Y, rows, n, n, es, true), "FIR", "null");         // the earlier clause speaks
    REFUSED(plain(X, rows, n - 1, X, rows, n, n, es, true), "FIR", "stride smaller");
  }
}

void dac_clauses() {
  const int64_t n = 40, batch = 4;
  for (const size_t es : {(size_t)8, (size_t)4}) {
    for (const int64_t k : {(int64_t)1, (int64_t)2}) {
      const int64_t rows = batch / k, on = k * n;
      const uint64_t in_ext = (uint64_t)(batch * n) * es, out_ext = (uint64_t)(rows * on) * 2;
      ACCEPTED(dac(X, n, Y, on, 0, batch, k, n, es));
      ACCEPTED(dac(X, n, Y, on, C, batch, k, n, es));
      REFUSED(dac(0, n, Y, on, 0, batch, k, n, es), "dac rows", "null in / out");
      REFUSED(dac(X, n, 0, on, 0, batch, k, n, es), "dac rows", "null in / out");
      REFUSED(dac(X + es / 2, n, Y, on, 0, batch, k, n, es), "dac rows", "not aligned to their element");
      REFUSED(dac(X, n, Y + 1, on, 0, batch, k, n, es), "dac rows", "not aligned to their element");
      ACCEPTED(dac(X + es, n, Y + 2, on, 0, batch, k, n, es));
      REFUSED(dac(X, n - 1, Y, on, 0, batch, k, n, es), "dac rows", "in row stride smaller than n");
      REFUSED(dac(X, n, Y, on - 1, 0, batch, k, n, es), "dac rows", "out row stride smaller than n");
      // out of place
      REFUSED(dac(X, n, X, on, 0, batch, k, n, es), "dac rows", "dac rows is out of place: out overlaps in");
      REFUSED(dac(X, n, X + in_ext - 2, on, 0, batch, k, n, es), "dac rows", "overlaps");
      ACCEPTED(dac(X, n, X + in_ext, on, 0, batch, k, n, es));
      REFUSED(dac(Y + out_ext - es, n, Y, on, 0, batch, k, n, es), "dac rows", "overlaps");
      ACCEPTED(dac(Y + out_ext, n, Y, on, 0, batch, k, n, es));
      // the report: batch x 3 int64
      const uint64_t rep = (uint64_t)batch * 3 * 8;
      REFUSED(dac(X, n, Y, on, C + 4, batch, k, n, es), "dac rows", "counts are not aligned");
      REFUSED(dac(X, n, Y, on, X + in_ext - 8, batch, k, n, es), "dac rows", "counts overlaps in");
      ACCEPTED(dac(X, n, Y, on, X + in_ext, batch, k, n, es));
      REFUSED(dac(X, n, Y, on, X - rep + 8, batch, k, n, es), "dac rows", "counts overlaps in");
      ACCEPTED(dac(X, n, Y, on, X - rep, batch, k, n, es));
      REFUSED(dac(X, n, Y, on, Y + out_ext - 8, batch, k, n, es), "dac rows", "counts overlaps out");
      ACCEPTED(dac(X, n, Y, on, Y + out_ext, batch, k, n, es));
      REFUSED(dac(X, n, Y, on, Y - rep + 8, batch, k, n, es), "dac rows", "counts overlaps out");
      ACCEPTED(dac(X, n, Y, on, Y - rep, batch, k, n, es));
      // the earlier clause speaks
      REFUSED(dac(0, n, Y, on, C + 4, batch, k, n, es), "dac rows", "counts are not aligned");
      REFUSED(dac(0, n, Y + 1, on, 0, batch, k, n, es), "dac rows", "null");
      REFUSED(dac(X + es / 2, n - 1, Y, on, 0, batch, k, n, es), "dac rows", "not aligned");
      REFUSED(dac(X, n - 1, X, on, 0, batch, k, n, es), "dac rows", "stride smaller");
      REFUSED(dac(X, n, X, on, X, batch, k, n, es), "dac rows", "out of place");
    }
    // a lone output row: its stride is not read, and its extent is the row
    ACCEPTED(dac(X, n, Y, 2 * n - 1, 0, 2, 2, n, es));
    ACCEPTED(dac(X, n, Y, 0, 0, 2, 2, n, es));
    ACCEPTED(dac(X, n, Y, n - 1, 0, 1, 1, n, es));
    REFUSED(dac(X, n - 1, Y, n, 0, 1, 1, n, es), "dac rows", "in row stride smaller");   // the input's counts
    ACCEPTED(dac(X, n, X + n * es, 1, 0, 1, 1, n, es));
    REFUSED(dac(X, n, X - 2 * n + 2, 1, 0, 1, 1, n, es), "dac rows", "overlaps");
    ACCEPTED(dac(X, n, X - 2 * n, 1, 0, 1, 1, n, es));
  }
}

void marker_clauses() {
  const int64_t n = 40, batch = 4;
  for (const size_t es : {(size_t)8, (size_t)4}) {
    for (const int64_t k : {(int64_t)1, (int64_t)2}) {
      for (const bool codes : {false, true}) {
        const char* o = codes ? "codes" : "out";
        const int64_t rows = batch / k, on = codes ? k * n : n;
        const size_t oes = codes ? 2 : 1;
        const uint64_t in_ext = (uint64_t)(batch * n) * es, out_ext = (uint64_t)(rows * on) * oes;
        ACCEPTED(marker(X, n, Y, on, codes, 0, batch, k, n, es));
        ACCEPTED(marker(X, n, Y, on, codes, C, batch, k, n, es));
        REFUSED(marker(0, n, Y, on, codes, 0, batch, k, n, es), "marker rows", "null in / ");
        REFUSED(marker(X, n, 0, on, codes, 0, batch, k, n, es), "marker rows", o);
        REFUSED(marker(X + es / 2, n, Y, on, codes, 0, batch, k, n, es), "marker rows", "not aligned");
        if (codes)
          REFUSED(marker(X, n, Y + 1, on, codes, 0, batch, k, n, es), "marker rows", "not aligned");
        else
          ACCEPTED(marker(X, n, Y + 1, on, codes, 0, batch, k, n, es));             // bytes are aligned anywhere
        REFUSED(marker(X, n - 1, Y, on, codes, 0, batch, k, n, es), "marker rows", "in row stride smaller");
        REFUSED(marker(X, n, Y, on - 1, codes, 0, batch, k, n, es), "marker rows", "row stride smaller");
        REFUSED(marker(X, n, X, on, codes, 0, batch, k, n, es), "marker rows", "overlaps in");
        REFUSED(marker(X, n, X + in_ext - oes, on, codes, 0, batch, k, n, es), "marker rows", "overlaps in");
        ACCEPTED(marker(X, n, X + in_ext, on, codes, 0, batch, k, n, es));
        REFUSED(marker(Y + out_ext - es, n, Y, on, codes, 0, batch, k, n, es), "marker rows", "overlaps in");
        ACCEPTED(marker(Y + out_ext, n, Y, on, codes, 0, batch, k, n, es));
        // the report: rows x 2 int64
        const uint64_t rep = (uint64_t)rows * 2 * 8;
        REFUSED(marker(X, n, Y, on, codes, C + 4, batch, k, n, es), "marker rows", "counts are not aligned");
        REFUSED(marker(X, n, Y, on, codes, X + in_ext - 8, batch, k, n, es), "marker rows", "counts overlaps in");
        ACCEPTED(marker(X, n, Y, on, codes, X + in_ext, batch, k, n, es));
        REFUSED(marker(X, n, Y, on, codes, X - rep + 8, batch, k, n, es), "marker rows", "counts overlaps in");
        ACCEPTED(marker(X, n, Y, on, codes, X - rep, batch, k, n, es));
        REFUSED(marker(X, n, Y, on, codes, Y + out_ext - 8, batch, k, n, es), "marker rows", "counts overlaps");
        ACCEPTED(marker(X, n, Y, on, codes, Y + out_ext, batch, k, n, es));
        REFUSED(marker(X, n, Y, on, codes, Y - rep + 8, batch, k, n, es), "marker rows", "counts overlaps");
        ACCEPTED(marker(X, n, Y, on, codes, Y - rep, batch, k, n, es));
        if (!codes) {   // bytes may end anywhere: the report meets them by ONE byte, or only touches
          REFUSED(marker(X, n, C + rep - 1, on, codes, C, batch, k, n, es), "marker rows", "counts overlaps out");
          ACCEPTED(marker(X, n, C + rep, on, codes, C, batch, k, n, es));
          REFUSED(marker(X, n, C - out_ext + 1, on, codes, C, batch, k, n, es), "marker rows", "counts overlaps out");
          ACCEPTED(marker(X, n, C - out_ext, on, codes, C, batch, k, n, es));
        }
        REFUSED(marker(0, n, Y, on, codes, C + 4, batch, k, n, es), "marker rows", "counts are not aligned");
        REFUSED(marker(X + es / 2, n - 1, Y, on, codes, 0, batch, k, n, es), "marker rows", "not aligned");
        REFUSED(marker(X, n - 1, X, on, codes, 0, batch, k, n, es), "marker rows", "stride smaller");
      }
    }
    // a lone output row: its stride is not read
    ACCEPTED(marker(X, n, Y, n - 1, false, 0, 2, 2, n, es));
    ACCEPTED(marker(X, n, Y, 2 * n - 1, true, 0, 2, 2, n, es));
    ACCEPTED(marker(X, n, Y, 0, false, 0, 1, 1, n, es));
    REFUSED(marker(X, n - 1, Y, n, false, 0, 1, 1, n, es), "marker rows", "in row stride smaller");
  }
}

void mix_clauses() {
  const int64_t n = 40, rows_in = 4;
  for (const size_t es : {(size_t)8, (size_t)4}) {
    for (const int64_t rows_out : {(int64_t)4, (int64_t)7, (int64_t)2}) {
      const uint64_t in_ext = (uint64_t)(rows_in * n) * es, out_ext = (uint64_t)(rows_out * n) * es;
      ACCEPTED(mix(X, rows_in, n, Y, rows_out, n, n, es));
      REFUSED(mix(0, rows_in, n, Y, rows_out, n, n, es), "mix rows", "null in / out");
      REFUSED(mix(X, rows_in, n, 0, rows_out, n, n, es), "mix rows", "null in / out");
      REFUSED(mix(X + es / 2, rows_in, n, Y, rows_out, n, n, es), "mix rows", "not aligned to their element");
      REFUSED(mix(X, rows_in, n, Y + es / 2, rows_out, n, n, es), "mix rows", "not aligned to their element");
      REFUSED(mix(X, rows_in, n - 1, Y, rows_out, n, n, es), "mix rows", "stride smaller than n");
      REFUSED(mix(X, rows_in, n, Y, rows_out, n - 1, n, es), "mix rows", "stride smaller than n");
      REFUSED(mix(X, rows_in, n, X, rows_out, n, n, es), "mix rows", "mix rows is out of place: out overlaps in");
      REFUSED(mix(X, rows_in, n, X + in_ext - es, rows_out, n, n, es), "mix rows", "overlaps");
      ACCEPTED(mix(X, rows_in, n, X + in_ext, rows_out, n, n, es));
      REFUSED(mix(X, rows_in, n, X - out_ext + es, rows_out, n, n, es), "mix rows", "overlaps");
      ACCEPTED(mix(X, rows_in, n, X - out_ext, rows_out, n, n, es));
      REFUSED(mix(0, rows_in, n, Y + es / 2, rows_out, n, n, es), "mix rows", "null");
      REFUSED(mix(X + es / 2, rows_in, n - 1, Y, rows_out, n, n, es), "mix rows", "not aligned");
      REFUSED(mix(X, rows_in, n - 1, X, rows_out, n, n, es), "mix rows", "stride smaller");
    }
    // a lone row on either side: its stride counts here
    REFUSED(mix(X, rows_in, n, Y, 1, n - 1, n, es), "mix rows", "out row stride smaller than n");
    REFUSED(mix(X, 1, n - 1, Y, 4, n, n, es), "mix rows", "in row stride smaller than n");
    ACCEPTED(mix(X, 1, n, Y, 1, n, n, es));
  }
}

void extract_clauses() {
  const int64_t n = 40, skip = 3, K = n - 2 * skip, batch = 4;
  const uint64_t Z = 1ull << 27;   // the result
  for (const int64_t in_rows : {batch, (int64_t)1}) {
    const uint64_t in_ext = (uint64_t)(in_rows * n) * 8, out_ext = (uint64_t)(batch * n) * 8, ker_ext = (uint64_t)(batch * K) * 8;
    ACCEPTED(extract(X, in_rows, n, Y, n, Z, K, batch, n, K));
    ACCEPTED(extract(X, in_rows, n, X, n, Z, K, batch, n, K));                     // the inputs may overlap each other
    REFUSED(extract(0, in_rows, n, Y, n, Z, K, batch, n, K), "extract rows", "null");
    REFUSED(extract(X, in_rows, n, 0, n, Z, K, batch, n, K), "extract rows", "null");
    REFUSED(extract(X, in_rows, n, Y, n, 0, K, batch, n, K), "extract rows", "null");
    REFUSED(extract(X + 4, in_rows, n, Y, n, Z, K, batch, n, K), "extract rows", "not aligned");
    REFUSED(extract(X, in_rows, n, Y + 4, n, Z, K, batch, n, K), "extract rows", "not aligned");
    REFUSED(extract(X, in_rows, n, Y, n, Z + 4, K, batch, n, K), "extract rows", "not aligned");
    REFUSED(extract(X, in_rows, n - 1, Y, n, Z, K, batch, n, K), "extract rows", "sig_in row stride smaller");
    REFUSED(extract(X, in_rows, n, Y, n - 1, Z, K, batch, n, K), "extract rows", "sig_out row stride smaller");
    REFUSED(extract(X, in_rows, n, Y, n, Z, K - 1, batch, n, K), "extract rows", "ker row stride smaller");
    ACCEPTED(extract(X, in_rows, n, Y, n, Z, K, batch, n, K));
    REFUSED(extract(X, in_rows, n, Y, n, X + in_ext - 8, K, batch, n, K), "extract rows", "ker overlaps sig_in");
    ACCEPTED(extract(X, in_rows, n, Y, n, X + in_ext, K, batch, n, K));
    REFUSED(extract(X, in_rows, n, Y, n, X - ker_ext + 8, K, batch, n, K), "extract rows", "ker overlaps sig_in");
    ACCEPTED(extract(X, in_rows, n, Y, n, X - ker_ext, K, batch, n, K));
    REFUSED(extract(X, in_rows, n, Y, n, Y + out_ext - 8, K, batch, n, K), "extract rows", "ker overlaps sig_out");
    ACCEPTED(extract(X, in_rows, n, Y, n, Y + out_ext, K, batch, n, K));
    REFUSED(extract(X, in_rows, n, Y, n, Y - ker_ext + 8, K, batch, n, K), "extract rows", "ker overlaps sig_out");
    ACCEPTED(extract(X, in_rows, n, Y, n, Y - ker_ext, K, batch, n, K));
    REFUSED(extract(0, in_rows, n, Y + 4, n, Z, K, batch, n, K), "extract rows", "null");
    REFUSED(extract(X + 4, in_rows, n - 1, Y, n, Z, K, batch, n, K), "extract rows", "not aligned");
    REFUSED(extract(X, in_rows, n, Y, n, Y, K - 1, batch, n, K), "extract rows", "stride smaller");
  }
  // lone rows: every stride counts
  REFUSED(extract(X, 1, n - 1, Y, n, Z, K, batch, n, K), "extract rows", "sig_in row stride smaller");
  REFUSED(extract(X, 1, n, Y, n, Z, K - 1, 1, n, K), "extract rows", "ker row stride smaller");
  REFUSED(extract(X, 1, n, Y, n - 1, Z, K, 1, n, K), "extract rows", "sig_out row stride smaller");
}

// ---- the report on its own ------------------------------------------------------------------------------------

void report() {
  const int64_t rows = 5, counters = 3;
  const RowReport r{at(C), rows, counters};
  HOLD(r.bytes() == (size_t)rows * counters * 8 && RowReport().bytes() == 0);
  ACCEPTED(wfk_report_rule("dac rows", r, keep));
  ACCEPTED(wfk_report_rule("dac rows", RowReport(), keep));                         // no report
  REFUSED(wfk_report_rule("dac rows", RowReport{at(C + 4), rows, counters}, keep), "dac rows", "counts are not aligned");
  REFUSED(wfk_report_rule("dac rows", RowReport{at(C + 1), rows, counters}, keep), "dac rows", "counts are not aligned");
  // one byte of either side inside it; sides that only touch it
  const int64_t n = 15;
  for (const size_t es : {(size_t)8, (size_t)4, (size_t)2, (size_t)1}) {
    const RowSide side{"in", nullptr, 4, n + 3, n, es};
    const auto at_ptr = [&](uint64_t p) { RowSide s = side; s.ptr = at(p); return s; };
    HOLD(at_ptr(C + r.bytes() - 1).meets(r.ptr, r.bytes()));
    HOLD(!at_ptr(C + r.bytes()).meets(r.ptr, r.bytes()));
    HOLD(at_ptr(C - side.bytes() + 1).meets(r.ptr, r.bytes()));
    HOLD(!at_ptr(C - side.bytes()).meets(r.ptr, r.bytes()));
  }
}

}  // namespace

int main() {
  extents();
  far_rows();
  plain_clauses();
  dac_clauses();
  marker_clauses();
  mix_clauses();
  extract_clauses();
  report();
  std::printf("row rule ok\n");
  return 0;
}
