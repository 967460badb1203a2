// wfk_mix_rows.hip -- a linear map ACROSS rows, per sample: rows_out output rows from rows_in input rows through a
// sparse rows_out x rows_in matrix M (CSR) and an offset per output row -- flux crosstalk compensation (a band), IQ
// mixer correction (2 x 2 blocks and a DC offset).  A term of output row o is a pair (c, M[o, c]) with M[o, c] != 0;
// per sample, in double (a float sample is widened first), without a fused multiply-add,
//   acc = 0.0;   for the terms of o in ascending c:  acc = fl(acc + fl(x[c, i] * M[o, c]));   y[o, i] = fl(acc + offset[o])
// -- what the NumPy loop `acc = acc + x[c] * m` computes -- and a float result is rounded once at the end.  An input
// row on which o has no term is never read for o: its NaN and inf stay out of y[o].
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) in which a workgroup owns a column span of a TILE of
// WFK_MIX_TILE_ROWS consecutive output rows, not of one row: blockIdx.x = tile * blocks_per_row + block.  The host
// builds per tile the sorted union of the input rows its rows have terms on (MixEntry: the input row and the mask of
// the tile rows with a term on it) and, per (union entry, tile row), the coefficient.  These tables sit at
// workgroup-uniform addresses: they arrive by scalar loads, and "has a term" is a scalar branch on a mask bit.  A thread
// takes kSlots slots, kThreads apart; per slot it walks the tile's union in ascending order in chunks of at most
// kChunk input rows -- the chunk's loads issued together, then its terms added into the tile's accumulators, ascending
// c -- so every output row sums in ascending c whatever the tiling, and every input element a tile needs is read once.
// Slots are laid out on the element index from the lead of the tile's FIRST output row.  Every other row of the tile,
// input or output, may sit at another alignment (odd strides): whether its slot addresses are 16-byte aligned is the
// same for every slot of the row in the workgroup and is tested once; aligned rows move whole slots with 16-byte
// accesses, the others -- and the partial slots at the two ends of a row -- element by element inside [0, n).
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

#pragma clang fp contract(off)   // a rounded product and a rounded sum, as the host formula

namespace {

constexpr int kTile = WFK_MIX_TILE_ROWS;   // output rows per tile
constexpr int kChunk = 8;                  // input rows whose loads are in flight together
static_assert(kTile <= 32, "the term mask of a union entry is one 32-bit word");

// the V elements of the slot that starts at element i0 of the row x[0 .. n); `vec`: the row's slot addresses are
// 16-byte aligned.  Elements outside [0, n) are not read (and come out 0).
template <typename T>
__device__ __forceinline__ void load_slot(const T* __restrict__ x, int64_t n, int64_t i0, bool vec,
                                          T (&r)[16 / sizeof(T)]) {
  constexpr int V = 16 / sizeof(T);
  if (vec && i0 >= 0 && i0 + V <= n) {
    const typename Slot<T>::type v = *reinterpret_cast<const typename Slot<T>::type*>(x + i0);
    if constexpr (V == 2) {
      r[0] = v.x; r[1] = v.y;
    } else {
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) r[e] = (i0 + e >= 0 && i0 + e < n) ? x[i0 + e] : (T)0;
  }
}

// in: [rows_in] rows of n samples; out: [rows_out] rows of n samples that share no memory with them.  entries /
// coef: the tiles' input lists back to back, tile t at [tile_ptr[t], tile_ptr[t + 1]), coef[u * kTile + j] the
// coefficient of tile row j on entry u (0.0: no term); offset: [tiles * kTile].  Row strides in elements.
template <typename T>
__global__ void __launch_bounds__(kThreads)
    mix_rows(const T* __restrict__ in, int64_t in_stride, T* __restrict__ out, int64_t out_stride,
             const int64_t* __restrict__ tile_ptr, const MixEntry* __restrict__ entries,
             const double* __restrict__ coef, const double* __restrict__ offset, int64_t n, int32_t rows_out,
             uint32_t blocks_per_row) {
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t span = (int64_t)kSlots * kThreads * V;
  const auto [tile, blk] = row_block(blocks_per_row);
  const int64_t o0 = (int64_t)tile * kTile;                       // the tile's first output row
  const int rows = (int)min((int64_t)kTile, (int64_t)rows_out - o0);
  T* __restrict__ y0 = out + o0 * out_stride;
  const int64_t first = (int64_t)blk * span - row_lead(y0);       // the block's first element index
  if (first >= n) return;
  const int64_t u_begin = tile_ptr[tile], u_end = tile_ptr[tile + 1];
  // 16-byte alignment of the slot addresses of row p: one test per row and workgroup
  const auto aligned = [first](const T* p) {
    return (((uintptr_t)p + (uintptr_t)(first * (int64_t)sizeof(T))) & 15) == 0;
  };
  uint32_t live = 0, vec_out = 0;   // bit j: the tile has a row j; its slot addresses are aligned
#pragma unroll
  for (int j = 0; j < kTile; ++j) {
    if (j < rows) {
      live |= 1u << j;
      if (aligned(y0 + (int64_t)j * out_stride)) vec_out |= 1u << j;
    }
  }
#pragma unroll 1
  for (int s = 0; s < kSlots; ++s) {
    const int64_t base = first + (int64_t)s * kThreads * V;
    if (base >= n) break;   // (the same for every thread: what follows is converged)
    const int64_t i0 = base + (int64_t)threadIdx.x * V;
    double acc[kTile][V];
#pragma unroll
    for (int j = 0; j < kTile; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[j][e] = 0.0;
#pragma unroll 1
    for (int64_t u0 = u_begin; u0 < u_end; u0 += kChunk) {
      const int m = (int)min((int64_t)kChunk, u_end - u0);
      T x[kChunk][V];   // (a float sample is widened where it is used)
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        if (q < m) {
          const T* __restrict__ xr = in + (int64_t)entries[u0 + q].col * in_stride;
          load_slot<T>(xr, n, i0, aligned(xr), x[q]);
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
              for (int e = 0; e < V; ++e) acc[j][e] = acc[j][e] + (double)x[q][e] * cj;
            }
          }
        }
      }
    }
    if (i0 >= n) continue;
    const bool whole = i0 >= 0 && i0 + V <= n;
    // Left alone the compiler forms the 8 row pointers and the 16 tests of the two masks before the slot loop and
    // keeps them, each test as a lane mask in a pair of scalar registers (they spill).  The empty statement makes the
    // three words values of this iteration: the tests stay scalar branches on a bit.
    uint32_t live_s = live, vec_s = vec_out;
    int64_t stride_s = out_stride;
    asm volatile("" : "+s"(live_s), "+s"(vec_s), "+s"(stride_s));
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
      if (live_s & (1u << j)) {
        T* __restrict__ y = y0 + (int64_t)j * stride_s;
        const double off = offset[o0 + j];
        T v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = (T)(acc[j][e] + off);
        if (vec_s & (1u << j)) {
          store_slot<T>(y, n, i0, v);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (whole || (i0 + e >= 0 && i0 + e < n)) y[i0 + e] = v[e];
        }
      }
    }
  }
}

}  // namespace

struct wfk_mix_rows_plan {
  int64_t n = 0, reads = 0;
  int32_t rows_out = 0, rows_in = 0, kind = 0;
  uint32_t tiles = 0, blocks_per_row = 0;
  size_t ptr_off = 0, entries_off = 0, coef_off = 0, offset_off = 0;
  DevBuf<char> tables;   // tile_ptr [tiles + 1], MixEntry [reads], coef [reads * kTile], offset [tiles * kTile]
};

namespace {

template <typename T>
void mix_launch(const wfk_mix_rows_plan* p, const void* in, int64_t in_stride, void* out, int64_t out_stride,
                hipStream_t s) {
  char* t = p->tables.get();
  hipLaunchKernelGGL(mix_rows<T>, dim3(p->blocks_per_row * p->tiles), dim3(kThreads), 0, s, (const T*)in, in_stride,
                     (T*)out, out_stride, DevTables::at<const int64_t>(t, p->ptr_off),
                     DevTables::at<const MixEntry>(t, p->entries_off), DevTables::at<const double>(t, p->coef_off),
                     DevTables::at<const double>(t, p->offset_off), p->n, p->rows_out, p->blocks_per_row);
}

}  // namespace

extern "C" {

int wfk_mix_rows_plan_destroy(wfk_mix_rows_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_mix_rows_kernel_name(const wfk_mix_rows_plan* p) {
  if (!p) return "";
  return p->kind == WFK_OUT_F32 ? "mix_rows<float>" : "mix_rows<double>";
}

int64_t wfk_mix_rows_reads(const wfk_mix_rows_plan* p) { return p ? p->reads : 0; }

int wfk_mix_rows_plan_create(int64_t n, int32_t rows_out, int32_t rows_in, int kind, const int64_t* row_ptr,
                             const int32_t* col, const double* val, const double* offset,
                             wfk_mix_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (const int rc = wfk_mix_check(n, rows_out, rows_in, kind, row_ptr, col, val, offset)) return rc;
  const int64_t tiles = ((int64_t)rows_out + kTile - 1) / kTile;
  const int V = 16 / (int)wfk_elem_size(kind);
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("mix rows plan", n, (int64_t)kSlots * kThreads * V, V - 1, tiles, &bpr)) return rc;
  const MixTiles tiled = wfk_mix_tiles(kTile, rows_out, row_ptr, col, val);
  std::vector<double> offs((size_t)tiles * kTile, 0.0);
  if (offset) std::copy(offset, offset + rows_out, offs.begin());
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_mix_rows_plan> p(new wfk_mix_rows_plan());
  p->n = n; p->rows_out = rows_out; p->rows_in = rows_in; p->kind = kind;
  p->reads = (int64_t)tiled.entries.size();
  p->tiles = (uint32_t)tiles; p->blocks_per_row = bpr;
  DevTables tab;
  p->ptr_off = tab.add(tiled.tile_ptr);
  p->entries_off = tab.add(tiled.entries);
  p->coef_off = tab.add(tiled.coef);
  p->offset_off = tab.add(offs);
  if (const int rc = wfk_upload_tables("mix rows plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the mix rows plan");
}

int wfk_mix_rows_apply(wfk_mix_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                       int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;   // nothing to mix (the pointers of empty rows may be null)
  const size_t es = wfk_elem_size(p->kind);
  if (const int rc = wfk_row_rule("mix rows", {{"in", in_dev, p->rows_in, in_stride, p->n, es}},
                                  {"out", out_dev, p->rows_out, out_stride, p->n, es}, kRowsAligned | kRowsDisjoint,
                                  wfk_fail))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (p->kind == WFK_OUT_F32)
    mix_launch<float>(p, in_dev, in_stride, out_dev, out_stride, s);
  else
    mix_launch<double>(p, in_dev, in_stride, out_dev, out_stride, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "mix rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
