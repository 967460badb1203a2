// wfk_mix_tables.h -- what the host side of the two mixing kernels shares (mix_rows of wfk_mix_rows.hip, mix_dac_rows of
// wfk_mix_dac.hip): the refusals of a CSR matrix and its offsets, and the builder of the per-tile tables both kernels
// walk, at the caller's tile height.  Host code, but for MixEntry, which the kernels read.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"

namespace {

// one entry of a tile's input list: the input row, and bit j set where row j of the tile has a term on it
struct MixEntry {
  int32_t col;
  uint32_t mask;
};

// the refusals of wfk_mix_rows_plan_create behind `null out`, in their order and with their texts
inline int wfk_mix_check(int64_t n, int32_t rows_out, int32_t rows_in, int kind, const int64_t* row_ptr,
                         const int32_t* col, const double* val, const double* offset) {
  if (!row_ptr) return wfk_fail(WFK_EINVAL, "mix rows plan: null row_ptr");
  if (rows_out < 1) return wfk_fail(WFK_EINVAL, "mix rows plan: rows_out < 1");
  if (rows_in < 1) return wfk_fail(WFK_EINVAL, "mix rows plan: rows_in < 1");
  if (n < 0) return wfk_fail(WFK_EINVAL, "mix rows plan: n < 0");
  if (const int rc = wfk_check_kind(kind)) return rc;
  bool rising = row_ptr[0] == 0;
  for (int32_t r = 0; r < rows_out && rising; ++r) rising = row_ptr[r + 1] >= row_ptr[r];
  if (!rising) return wfk_fail(WFK_EINVAL, "mix rows plan: row_ptr is not non-decreasing from 0");
  if (row_ptr[rows_out] > 0 && (!col || !val)) return wfk_fail(WFK_EINVAL, "mix rows plan: null col / val");
  for (int32_t r = 0; r < rows_out; ++r) {
    const std::string row = "row " + std::to_string(r) + ": ";
    for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; ++k) {
      if (col[k] < 0 || col[k] >= rows_in)
        return wfk_fail(WFK_EINVAL, row + "column " + std::to_string(col[k]) + " is out of range");
      if (k > row_ptr[r] && col[k] <= col[k - 1]) return wfk_fail(WFK_EINVAL, row + "columns are not ascending");
      if (!std::isfinite(val[k]))
        return wfk_fail(WFK_EINVAL, row + "coefficient (" + std::to_string(r) + ", " + std::to_string(col[k]) +
                                        ") is not finite");
    }
    if (offset && !std::isfinite(offset[r])) return wfk_fail(WFK_EINVAL, row + "offset is not finite");
  }
  return WFK_OK;
}

// The tables of a checked matrix for tiles of `tile` consecutive output rows.  Per tile: the sorted union of the columns
// its rows have terms on (zeros in val are not terms), tile t at entries[tile_ptr[t] .. tile_ptr[t + 1]), and per
// (union entry, tile row) the coefficient, coef[u * tile + j] (0.0: no term).
struct MixTiles {
  std::vector<int64_t> tile_ptr;
  std::vector<MixEntry> entries;
  std::vector<double> coef;
};

inline MixTiles wfk_mix_tiles(int tile, int32_t rows_out, const int64_t* row_ptr, const int32_t* col,
                              const double* val) {
  const int64_t tiles = ((int64_t)rows_out + tile - 1) / tile;
  MixTiles t;
  t.tile_ptr.assign((size_t)tiles + 1, 0);
  std::vector<int32_t> cols;
  for (int64_t i = 0; i < tiles; ++i) {
    const int64_t o0 = i * tile, o1 = std::min<int64_t>(o0 + tile, rows_out);
    cols.clear();
    for (int64_t k = row_ptr[o0]; k < row_ptr[o1]; ++k)
      if (val[k] != 0.0) cols.push_back(col[k]);
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    const size_t u0 = t.entries.size();
    for (const int32_t c : cols) t.entries.push_back(MixEntry{c, 0u});
    t.coef.resize(t.entries.size() * (size_t)tile, 0.0);
    for (int64_t o = o0; o < o1; ++o) {
      for (int64_t k = row_ptr[o]; k < row_ptr[o + 1]; ++k) {
        if (val[k] == 0.0) continue;
        const size_t u = u0 + (size_t)(std::lower_bound(cols.begin(), cols.end(), col[k]) - cols.begin());
        t.entries[u].mask |= 1u << (o - o0);
        t.coef[u * (size_t)tile + (size_t)(o - o0)] = val[k];
      }
    }
    t.tile_ptr[(size_t)i + 1] = (int64_t)t.entries.size();
  }
  return t;
}

}  // namespace
