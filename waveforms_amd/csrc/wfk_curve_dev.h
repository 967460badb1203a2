// wfk_curve_dev.h -- what the kernels that look a sample up in a row's calibration curve share: the row as the device
// reads it (CurveRow), its knots in LDS (Knots) and the lookup inside the knots (curve_at) -- curve_rows
// (wfk_curve_rows.hip) and the per-row IIR kernels that take the curve in front of their tile
// (wfk_iir_rows_curve_dac.hip) -- and, for the host, the one check of a batch of curves and the
// one builder of their device tables, so that both plans refuse with the same texts and look up through the same tables.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"

namespace {

// one row as the device reads it
struct CurveRow {
  int64_t off;     // of the row's knots in the knot table, in doubles: xp[K], fp[K], slope[K] from there
  int64_t boff;    // of the row's buckets in the bucket table
  int32_t K;
  int32_t nb;      // buckets: a power of two >= 2 K, or 0 (none: the bracket is every knot)
  double left, right;
  double x0, xl;   // xp[0], xp[K - 1]
  double scale;    // nb / (xl - x0)
};

// the knots of a row in LDS
struct Knots {
  const double* xp;
  const double* fp;
  const double* slope;
  const uint32_t* bucket;   // lo | hi << 16: the knots j with xp[j] <= x for some x of the bucket lie in [lo, hi]
};

// the curve at x, inside [x0, xl]
__device__ __forceinline__ double curve_at(const Knots& t, const CurveRow& row, double x) {
#pragma clang fp contract(off)   // a rounded difference, a rounded product and a rounded sum, wherever this is inlined
  int lo = 0, hi = row.K - 1;
  if (row.nb) {
    const double b = fmin(fmax((x - row.x0) * row.scale, 0.0), (double)(row.nb - 1));
    const uint32_t e = t.bucket[(int)b];
    lo = (int)(e & 0xffffu);
    hi = (int)(e >> 16);
  }
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.xp[mid] <= x) lo = mid; else hi = mid - 1;
  }
  // exact whatever the bracket was: the largest j with xp[j] <= x
  int j = lo;
  while (j > 0 && x < t.xp[j]) --j;
  while (j + 1 < row.K && t.xp[j + 1] <= x) ++j;
  const double xj = t.xp[j], fj = t.fp[j];
  return x == xj ? fj : t.slope[j] * (x - xj) + fj;
}

// ---- host: the check and the tables ---------------------------------------------------------------------------------

// What every plan with per-row curves asks of them, with its texts (WFK_EINVAL), before any device work: n >= 0, rows,
// a CSR-like knot_ptr from 0, per row 2 .. WFK_CURVE_MAX_KNOTS finite, strictly increasing knots and finite values.
inline int curve_check(int64_t n, int32_t batch, int kind, const int64_t* knot_ptr, const double* xp, const double* fp) {
  if (n < 0 || batch < 1 || !knot_ptr || !xp || !fp) return wfk_fail(WFK_EINVAL, "bad curve rows plan arguments");
  if (const int rc = wfk_check_kind(kind)) return rc;
  if (knot_ptr[0] != 0) return wfk_fail(WFK_EINVAL, "curve rows plan: knot_ptr is not non-decreasing from 0");
  for (int32_t r = 0; r < batch; ++r)
    if (knot_ptr[r + 1] < knot_ptr[r])
      return wfk_fail(WFK_EINVAL, "curve rows plan: knot_ptr is not non-decreasing from 0");
  for (int32_t r = 0; r < batch; ++r) {
    const std::string row = "row " + std::to_string(r) + ": ";
    const int64_t k = knot_ptr[r + 1] - knot_ptr[r];
    if (k < 2) return wfk_fail(WFK_EINVAL, row + "fewer than 2 knots");
    if (k > WFK_CURVE_MAX_KNOTS)
      return wfk_fail(WFK_EINVAL, row + "more than " + std::to_string(WFK_CURVE_MAX_KNOTS) + " knots");
    const double* x = xp + knot_ptr[r];
    const double* f = fp + knot_ptr[r];
    for (int64_t j = 0; j < k; ++j) {
      if (!std::isfinite(x[j])) return wfk_fail(WFK_EINVAL, row + "knot " + std::to_string(j) + " is not finite");
      if (j && !(x[j] > x[j - 1]))
        return wfk_fail(WFK_EINVAL, row + "knots are not strictly increasing at " + std::to_string(j));
    }
    for (int64_t j = 0; j < k; ++j)
      if (!std::isfinite(f[j])) return wfk_fail(WFK_EINVAL, row + "value " + std::to_string(j) + " is not finite");
  }
  return WFK_OK;
}

// the largest j with xp[j] <= v, for v >= xp[0]
inline int knot_at_or_below(const double* xp, int K, double v) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (xp[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the device tables of a batch of checked curves
struct CurveTables {
  std::vector<CurveRow> rows;
  std::vector<double> knots;       // per row xp[K], fp[K], slope[K]
  std::vector<uint32_t> buckets;
  int max_k = 0, max_nb = 0;       // of the largest row: what a workgroup's LDS has to hold
  size_t lds_bytes() const { return (size_t)24 * max_k + (size_t)4 * max_nb; }
};

// A row gets a power of two >= 2 K buckets over [xp[0], xp[K - 1]] (none where `use_buckets` is off or the range or its
// scale overflows), halved while the plan's largest row -- 24 bytes a knot and 4 a bucket -- exceeds `lds_budget`
// bytes, down to none: the bucket count never changes a result (curve_at's fix-up makes j exact).
inline CurveTables curve_build(int32_t batch, const int64_t* knot_ptr, const double* xp, const double* fp,
                               const double* left, const double* right, bool use_buckets, size_t lds_budget) {
  CurveTables t;
  for (int32_t r = 0; r < batch; ++r) t.max_k = std::max(t.max_k, (int)(knot_ptr[r + 1] - knot_ptr[r]));
  int cap = 1 << 30;
  if ((size_t)24 * t.max_k + 4 > lds_budget) cap = 0;
  else while ((size_t)24 * t.max_k + (size_t)4 * cap > lds_budget) cap >>= 1;
  std::vector<int> nbs((size_t)batch, 0);
  for (int32_t r = 0; r < batch; ++r) {
    const int k = (int)(knot_ptr[r + 1] - knot_ptr[r]);
    const double* x = xp + knot_ptr[r];
    int nb = 1;
    while (nb < 2 * k) nb *= 2;
    nb = std::min(nb, cap);
    const double scale = (double)nb / (x[k - 1] - x[0]);
    // (a range that overflows, or one so narrow that the scale does: plain bisection)
    if (use_buckets && nb && std::isfinite(scale) && scale > 0.0) nbs[r] = nb;
    t.max_nb = std::max(t.max_nb, nbs[r]);
  }
  t.rows.resize((size_t)batch);
  t.knots.resize((size_t)3 * (size_t)knot_ptr[batch]);
  for (int32_t r = 0; r < batch; ++r) {
    const int k = (int)(knot_ptr[r + 1] - knot_ptr[r]);
    const double* x = xp + knot_ptr[r];
    const double* f = fp + knot_ptr[r];
    CurveRow& row = t.rows[r];
    row.off = 3 * knot_ptr[r];
    row.boff = (int64_t)t.buckets.size();
    row.K = k;
    row.nb = nbs[r];
    row.left = left ? left[r] : f[0];
    row.right = right ? right[r] : f[k - 1];
    row.x0 = x[0];
    row.xl = x[k - 1];
    row.scale = row.nb ? (double)row.nb / (x[k - 1] - x[0]) : 0.0;
    double* g = t.knots.data() + row.off;
    for (int j = 0; j < k; ++j) {
      g[j] = x[j];
      g[k + j] = f[j];
      g[2 * k + j] = j + 1 < k ? (f[j + 1] - f[j]) / (x[j + 1] - x[j]) : 0.0;
    }
    // bucket b covers [x0 + b w, x0 + (b + 1) w), w = (xl - x0) / nb; what rounding does to an edge the fix-up absorbs
    const double w = (x[k - 1] - x[0]) / (double)std::max(row.nb, 1);
    for (int b = 0; b < row.nb; ++b) {
      const int lo = knot_at_or_below(x, k, x[0] + (double)b * w);
      const int hi = b + 1 < row.nb ? knot_at_or_below(x, k, x[0] + (double)(b + 1) * w) : k - 1;
      t.buckets.push_back((uint32_t)lo | ((uint32_t)std::max(lo, hi) << 16));
    }
  }
  return t;
}

// a second report next to `counts`: aligned, apart from both sides and from the first report
inline int curve_beyond_rule(const std::string& stage, const void* beyond, int32_t batch, const void* counts,
                    std::initializer_list<RowSide> sides) {
  if (!beyond) return WFK_OK;
  const size_t bytes = (size_t)batch * 3 * sizeof(int64_t);
  if ((uintptr_t)beyond & 7) return wfk_fail(WFK_EINVAL, stage + ": beyond is not aligned to int64");
  for (const RowSide& sd : sides)
    if (sd.meets(beyond, bytes)) return wfk_fail(WFK_EINVAL, stage + ": beyond overlaps " + sd.what);
  if (counts && wfk_ranges_overlap(beyond, bytes, counts, bytes))
    return wfk_fail(WFK_EINVAL, stage + ": beyond overlaps counts");
  return WFK_OK;
}

}  // namespace
