// wfk_mix_dac.hip -- the mix ACROSS rows (wfk_mix_rows.hip) that ends in int16 DAC codes (wfk_dac_rows.hip): the last
// float stage of a flux line (inverse crosstalk matrix) or a drive line (2 x 2 mixer correction and DC offset per IQ
// pair) and the converter behind it in one kernel, without the float rows between them.  Per sample, in double (a float
// sample is widened first), without a fused multiply-add,
//   acc = 0.0;   for the terms of o in ascending c:  acc = fl(acc + fl(x[c, i] * M[o, c]));   y = fl(acc + mix_offset[o])
//   y = (double)(float)y                      float plans only: the two stages round the mixed row to float once
//   v = fl(fl(y * gain[o]) + dac_offset[o]);  q = rint(v);  c = 0 if v is NaN, lo if q < lo, hi if q > hi, else q
//   code = (int)c << shift as int16;          interleave K:  out[g, i K + j] = code[g K + j, i]
// -- the statements of mix_rows and of dac_block, in their order: codes and counts equal the two launches bit for bit.
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) in which a workgroup owns a column span of a TILE of
// WFK_MIX_DAC_TILE_ROWS consecutive mix output rows (tile / K code rows): blockIdx.x = tile * blocks_per_row + block.
// The tables are those of mix_rows at this tile height -- per tile the sorted union of the input rows its rows have
// terms on with the mask of the rows that have one, and per (union entry, tile row) the coefficient -- at
// workgroup-uniform addresses: scalar loads and scalar branches on a mask bit.  A slot is a run of kRun = 4 SAMPLES of
// every row of the tile: 4 codes, one 8-byte store, per code row under K = 1; 4 + 4 codes, one 16-byte store, under
// K = 2.  (8 samples per lane in double are 16 accumulator registers per tile row before any load is in flight: see
// DESIGN 3.22 for the figures.)  The sample grid starts at the 16-byte boundary at or before the first code of the
// tile's FIRST code row.  Every other row of the tile, input or code, may sit at another alignment (odd strides): whether
// its slot addresses are aligned -- to 16 bytes for an input row, to the store's 8 K bytes for a code row -- is the same
// for every slot of the row in the workgroup and is tested once; aligned rows move whole slots with vector accesses, the
// others (a pair row that starts at an odd code among them) and the partial slots at the two ends of a row element by
// element inside [0, n): a partial group is written code by code, never read-modify-written.
// Counting (COUNT; the plain build carries none of it) is dac_block's: the lane masks of the three comparisons are
// counted per wave in converged code, the waves' counts summed through LDS, and one thread per counter adds a non-zero
// sum to the row's int64 counter with one atomic add.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_mix_tables.h"
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)   // a rounded product and a rounded sum, as the host formulas of both parents

namespace {

constexpr int kTile = WFK_MIX_DAC_TILE_ROWS;   // mix output rows per tile
constexpr int kChunk = 8;                      // input rows whose loads are in flight together
constexpr int kRun = 4;                        // samples of every tile row per slot
static_assert(kTile <= 32 && kTile % 2 == 0, "one 32-bit term mask per union entry; a pair never straddles two tiles");

// one mix output row as the device reads it
struct MixDacRow {
  double mix_offset, gain, dac_offset;
};

// the kRun samples from element i0 of the row x[0 .. n); `vec`: the row's slot addresses are 16-byte aligned.
// Elements outside [0, n) are not read (and come out 0).
template <typename T>
__device__ __forceinline__ void load_run(const T* __restrict__ x, int64_t n, int64_t i0, bool vec, T (&r)[kRun]) {
  if (vec && i0 >= 0 && i0 + kRun <= n) {
    typedef typename Slot<T>::type Q;
    const Q* __restrict__ p = reinterpret_cast<const Q*>(x + i0);
    if constexpr (sizeof(T) == 8) {
      const Q a = p[0], b = p[1];
      r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
    } else {
      const Q a = p[0];
      r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) r[e] = (i0 + e >= 0 && i0 + e < n) ? x[i0 + e] : (T)0;
  }
}

// w: the codes of samples i0 .. i0 + kRun - 1 of the K mix rows of the code row y[0 .. K n); VEC: the row's slot
// addresses are aligned to the store.  Codes of samples outside [0, n) are not written.
template <int K, bool VEC>
__device__ __forceinline__ void store_codes(int16_t* __restrict__ y, int64_t n, int64_t i0, const int (&w)[K][kRun]) {
  if (VEC && i0 >= 0 && i0 + kRun <= n) {
    if constexpr (K == 1) {
      uint2 q;
      q.x = (uint32_t)(w[0][0] & 0xffff) | ((uint32_t)w[0][1] << 16);
      q.y = (uint32_t)(w[0][2] & 0xffff) | ((uint32_t)w[0][3] << 16);
      *reinterpret_cast<uint2*>(y + i0) = q;
    } else {
      uint4 q;
      q.x = (uint32_t)(w[0][0] & 0xffff) | ((uint32_t)w[K - 1][0] << 16);
      q.y = (uint32_t)(w[0][1] & 0xffff) | ((uint32_t)w[K - 1][1] << 16);
      q.z = (uint32_t)(w[0][2] & 0xffff) | ((uint32_t)w[K - 1][2] << 16);
      q.w = (uint32_t)(w[0][3] & 0xffff) | ((uint32_t)w[K - 1][3] << 16);
      *reinterpret_cast<uint4*>(y + 2 * i0) = q;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) {
      if (i0 + e >= 0 && i0 + e < n) {
#pragma unroll
        for (int k = 0; k < K; ++k) y[(i0 + e) * K + k] = (int16_t)w[k][e];
      }
    }
  }
}

// in: [rows_in] rows of n samples; out: [rows_out / K] rows of K n codes that share no memory with them.  entries /
// coef: the tiles' input lists back to back, tile t at [tile_ptr[t], tile_ptr[t + 1]), coef[u * kTile + j] the
// coefficient of tile row j on entry u (0.0: no term); rowtab: [tiles * kTile]; counts (COUNT): [rows_out][3], zeroed
// before the launch.  Row strides in elements of their own side.
template <typename T, int K, bool COUNT>
__global__ void __launch_bounds__(kThreads)
    mix_dac_rows(const T* __restrict__ in, int64_t in_stride, int16_t* __restrict__ out, int64_t out_stride,
                 const int64_t* __restrict__ tile_ptr, const MixEntry* __restrict__ entries,
                 const double* __restrict__ coef, const MixDacRow* __restrict__ rowtab,
                 unsigned long long* __restrict__ counts, int64_t n, int32_t rows_out, uint32_t blocks_per_row,
                 double lo, double hi, int shift) {
  constexpr int64_t span = (int64_t)kSlots * kThreads * kRun;     // samples
  constexpr int kStore = 2 * kRun * K;                            // bytes of a code row's slot
  const auto [tile, blk] = row_block(blocks_per_row);
  const int64_t o0 = (int64_t)tile * kTile;                       // the tile's first mix output row
  const int rows = (int)min((int64_t)kTile, (int64_t)rows_out - o0);
  int16_t* __restrict__ y0 = out + (o0 / K) * out_stride;         // the tile's first code row
  const int64_t first = (int64_t)blk * span - row_lead(y0) / K;   // the block's first sample index
  if (first >= n) return;
  const int64_t u_begin = tile_ptr[tile], u_end = tile_ptr[tile + 1];
  // alignment of the slot addresses of a row: one test per row and workgroup
  const auto aligned = [first](const T* p) {
    return (((uintptr_t)p + (uintptr_t)(first * (int64_t)sizeof(T))) & 15) == 0;
  };
  uint32_t live = 0, vec_out = 0;   // bit j (j a multiple of K): the tile has a code row j / K; its slots are aligned
#pragma unroll
  for (int j = 0; j < kTile; j += K) {
    if (j < rows) {
      live |= 1u << j;
      const int16_t* y = y0 + (int64_t)(j / K) * out_stride;
      if ((((uintptr_t)y + (uintptr_t)(first * (int64_t)(2 * K))) & (kStore - 1)) == 0) vec_out |= 1u << j;
    }
  }
  // (the same in every lane; said so, because otherwise the compiler forms the word in a vector register and the
  // scalar constraint in the slot loop is refused)
  vec_out = __builtin_amdgcn_readfirstlane(vec_out);
  [[maybe_unused]] unsigned cnt[kTile][3];   // [tile row][below, above, nan] of this wave
  if constexpr (COUNT) {
#pragma unroll
    for (int j = 0; j < kTile; ++j) cnt[j][0] = cnt[j][1] = cnt[j][2] = 0;
  }
#pragma unroll 1
  for (int s = 0; s < kSlots; ++s) {
    const int64_t base = first + (int64_t)s * kThreads * kRun;
    if (base >= n) break;   // (the same for every thread: what follows is converged)
    const int64_t i0 = base + (int64_t)threadIdx.x * kRun;
    double acc[kTile][kRun];
#pragma unroll
    for (int j = 0; j < kTile; ++j)
#pragma unroll
      for (int e = 0; e < kRun; ++e) acc[j][e] = 0.0;
#pragma unroll 1
    for (int64_t u0 = u_begin; u0 < u_end; u0 += kChunk) {
      const int m = (int)min((int64_t)kChunk, u_end - u0);
      T x[kChunk][kRun];   // (a float sample is widened where it is used)
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        if (q < m) {
          const T* __restrict__ xr = in + (int64_t)entries[u0 + q].col * in_stride;
          load_run<T>(xr, n, i0, aligned(xr), x[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        if (q < m) {
          const uint32_t mask = entries[u0 + q].mask;
          const double* __restrict__ c = coef + (u0 + q) * kTile;
#pragma unroll
          for (int j = 0; j < kTile; ++j) {
            if (mask & (1u << j)) {
              const double cj = c[j];
#pragma unroll
              for (int e = 0; e < kRun; ++e) acc[j][e] = acc[j][e] + (double)x[q][e] * cj;
            }
          }
        }
      }
    }
    // From here on every lane of the wave runs every statement but the stores: the counts are ballots.
    const bool whole = i0 >= 0 && i0 + kRun <= n;
    // (as in mix_rows: the empty statement makes the three words values of this iteration, so the tests stay scalar
    // branches on a bit instead of lane masks kept across the slot loop)
    uint32_t live_s = live, vec_s = vec_out;
    int64_t stride_s = out_stride;
    asm volatile("" : "+s"(live_s), "+s"(vec_s), "+s"(stride_s));
#pragma unroll
    for (int j = 0; j < kTile; j += K) {
      if (live_s & (1u << j)) {
        int w[K][kRun];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const MixDacRow r = rowtab[o0 + j + k];
#pragma unroll
          for (int e = 0; e < kRun; ++e) {
            double y = acc[j + k][e] + r.mix_offset;
            if constexpr (sizeof(T) == 4) y = (double)(float)y;
            const double v = y * r.gain + r.dac_offset;
            const double q = rint(v);
            const bool nan = v != v, below = q < lo, above = q > hi;
            const double c = nan ? 0.0 : below ? lo : above ? hi : q;
            w[k][e] = (int)c * (1 << shift);
            if constexpr (COUNT) {
              const bool in_row = whole || (i0 + e >= 0 && i0 + e < n);
              cnt[j + k][0] += (unsigned)__popcll(__ballot(in_row && below));
              cnt[j + k][1] += (unsigned)__popcll(__ballot(in_row && above));
              cnt[j + k][2] += (unsigned)__popcll(__ballot(in_row && nan));
              // (as in dac_block: the sums exist here, in scalar registers, not as lane masks kept to the end)
#pragma unroll
              for (int t = 0; t < 3; ++t) asm volatile("" : "+s"(cnt[j + k][t]));
            }
          }
        }
        int16_t* __restrict__ y = y0 + (int64_t)(j / K) * stride_s;
        if (vec_s & (1u << j))   // (a scalar branch of its own, as in mix_rows; `whole` is tested per lane inside)
          store_codes<K, true>(y, n, i0, w);
        else
          store_codes<K, false>(y, n, i0, w);
      }
    }
  }
  if constexpr (COUNT) {
    __shared__ unsigned wave_counts[kThreads / 64][kTile * 3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < kTile; ++j)
#pragma unroll
        for (int t = 0; t < 3; ++t) wave_counts[wave][3 * j + t] = cnt[j][t];
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * rows) {
      unsigned sum = 0;
#pragma unroll
      for (int wv = 0; wv < kThreads / 64; ++wv) sum += wave_counts[wv][threadIdx.x];
      if (sum) atomicAdd(counts + o0 * 3 + threadIdx.x, (unsigned long long)sum);
    }
  }
}

}  // namespace

struct wfk_mix_dac_plan {
  int64_t n = 0, reads = 0;
  int32_t rows_out = 0, rows_in = 0, kind = 0;
  int bits = 0, shift = 0, k = 0;
  uint32_t tiles = 0, blocks_per_row = 0;
  size_t ptr_off = 0, entries_off = 0, coef_off = 0, rows_off = 0;
  DevBuf<char> tables;   // tile_ptr [tiles + 1], MixEntry [reads], coef [reads * kTile], MixDacRow [tiles * kTile]
};

namespace {

template <typename T, int K, bool COUNT>
void mix_dac_launch(const wfk_mix_dac_plan* p, const void* in, int64_t in_stride, int16_t* out, int64_t out_stride,
                    int64_t* counts, hipStream_t s) {
  char* t = p->tables.get();
  const double lo = -(double)(1 << (p->bits - 1)), hi = (double)((1 << (p->bits - 1)) - 1);
  hipLaunchKernelGGL((mix_dac_rows<T, K, COUNT>), dim3(p->blocks_per_row * p->tiles), dim3(kThreads), 0, s,
                     (const T*)in, in_stride, out, out_stride, DevTables::at<const int64_t>(t, p->ptr_off),
                     DevTables::at<const MixEntry>(t, p->entries_off), DevTables::at<const double>(t, p->coef_off),
                     DevTables::at<const MixDacRow>(t, p->rows_off), (unsigned long long*)counts, p->n, p->rows_out,
                     p->blocks_per_row, lo, hi, p->shift);
}

template <typename T>
void mix_dac_pick(const wfk_mix_dac_plan* p, const void* in, int64_t in_stride, int16_t* out, int64_t out_stride,
                  int64_t* counts, hipStream_t s) {
  if (p->k == 2) {
    if (counts) mix_dac_launch<T, 2, true>(p, in, in_stride, out, out_stride, counts, s);
    else mix_dac_launch<T, 2, false>(p, in, in_stride, out, out_stride, counts, s);
  } else {
    if (counts) mix_dac_launch<T, 1, true>(p, in, in_stride, out, out_stride, counts, s);
    else mix_dac_launch<T, 1, false>(p, in, in_stride, out, out_stride, counts, s);
  }
}

}  // namespace

extern "C" {

int wfk_mix_dac_plan_destroy(wfk_mix_dac_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_mix_dac_kernel_name(const wfk_mix_dac_plan* p, int with_counts) {
  if (!p) return "";
  static const char* const names[2][2][2] = {
      {{"mix_dac_rows<double,1,false>", "mix_dac_rows<double,1,true>"},
       {"mix_dac_rows<double,2,false>", "mix_dac_rows<double,2,true>"}},
      {{"mix_dac_rows<float,1,false>", "mix_dac_rows<float,1,true>"},
       {"mix_dac_rows<float,2,false>", "mix_dac_rows<float,2,true>"}}};
  return names[p->kind == WFK_OUT_F32][p->k == 2][with_counts != 0];
}

int64_t wfk_mix_dac_reads(const wfk_mix_dac_plan* p) { return p ? p->reads : 0; }

int64_t wfk_mix_dac_span(const wfk_mix_dac_plan* p) { return p ? (int64_t)kSlots * kThreads * kRun * p->k : 0; }

// The refusals are those of wfk_mix_rows_plan_create, then those of wfk_dac_rows_plan_create for rows_out rows, word
// for word.
int wfk_mix_dac_plan_create(int64_t n, int32_t rows_out, int32_t rows_in, int kind, const int64_t* row_ptr,
                            const int32_t* col, const double* val, const double* mix_offset, const double* gain,
                            const double* dac_offset, int bits, int shift, int interleave,
                            wfk_mix_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (const int rc = wfk_mix_check(n, rows_out, rows_in, kind, row_ptr, col, val, mix_offset)) return rc;
  if (!gain || !dac_offset) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  if (bits < 2 || bits > 16) return wfk_fail(WFK_EINVAL, "dac rows plan: bits must lie in [2, 16]");
  if (shift < 0 || shift > 16 - bits) return wfk_fail(WFK_EINVAL, "dac rows plan: shift must lie in [0, 16 - bits]");
  if (interleave != 1 && interleave != 2) return wfk_fail(WFK_EINVAL, "dac rows plan: interleave must be 1 or 2");
  if (rows_out % interleave)
    return wfk_fail(WFK_EINVAL,
                    "dac rows plan: " + std::to_string(rows_out) + " rows are no multiple of the interleave");
  for (int32_t r = 0; r < rows_out; ++r) {
    if (!std::isfinite(gain[r])) return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": gain is not finite");
    if (!std::isfinite(dac_offset[r]))
      return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": offset is not finite");
  }
  if (n > INT64_MAX / interleave) return wfk_fail(WFK_EINVAL, "dac rows plan: batch * n too large for one launch");
  const int64_t tiles = ((int64_t)rows_out + kTile - 1) / kTile;
  uint32_t bpr = 0;
  // the sample grid starts up to 7 / K samples before the row
  if (const int rc = wfk_row_blocks("mix dac plan", n, (int64_t)kSlots * kThreads * kRun, 7 / interleave, tiles, &bpr))
    return rc;
  const MixTiles tiled = wfk_mix_tiles(kTile, rows_out, row_ptr, col, val);   // mix_rows' tables at this tile height
  std::vector<MixDacRow> rows((size_t)tiles * kTile, MixDacRow{0.0, 0.0, 0.0});
  for (int32_t o = 0; o < rows_out; ++o)
    rows[(size_t)o] = MixDacRow{mix_offset ? mix_offset[o] : 0.0, gain[o], dac_offset[o]};
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_mix_dac_plan> p(new wfk_mix_dac_plan());
  p->n = n; p->rows_out = rows_out; p->rows_in = rows_in; p->kind = kind;
  p->bits = bits; p->shift = shift; p->k = interleave;
  p->reads = (int64_t)tiled.entries.size();
  p->tiles = (uint32_t)tiles; p->blocks_per_row = bpr;
  DevTables tab;
  p->ptr_off = tab.add(tiled.tile_ptr);
  p->entries_off = tab.add(tiled.entries);
  p->coef_off = tab.add(tiled.coef);
  p->rows_off = tab.add(rows);
  if (const int rc = wfk_upload_tables("mix dac plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the mix dac plan");
}

int wfk_mix_dac_apply(wfk_mix_dac_plan* p, const void* in_dev, int64_t in_stride, int16_t* out_dev,
                      int64_t out_stride, int64_t* counts_dev, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, p->rows_out, 3};
  // nothing to mix (the pointers of empty rows may be null): no kernel of this file; the report is still zeroed
  if (p->n == 0) return wfk_zero_report("mix dac", report, s);
  // a lone code row's stride is not read
  if (const int rc = wfk_row_rule("mix dac", {{"in", in_dev, p->rows_in, in_stride, p->n, wfk_elem_size(p->kind)}},
                                  {"out", out_dev, p->rows_out / p->k, out_stride, p->k * p->n, sizeof(int16_t), false},
                                  kRowsAligned | kRowsDisjoint, wfk_fail, report))
    return rc;
  if (const int rc = wfk_zero_report("mix dac", report, s)) return rc;
  if (p->kind == WFK_OUT_F32)
    mix_dac_pick<float>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  else
    mix_dac_pick<double>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "mix dac kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
