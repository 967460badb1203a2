// wfk_rows_dev.h -- the geometry of the row-slot kernels (spec_rows_mul, shift_rows, extract_ratio, extract_smooth).
// Device code; the launch arithmetic is wfk_row_blocks in wfk_host.h.
//
// The grid is flat, blockIdx.x = row * blocks_per_row + block in row: a workgroup never straddles rows, so whatever a
// kernel reads per row (a table entry, a term list, taps) sits at a wave-uniform address, arrives by scalar loads, and
// a branch on it is a scalar branch.  A thread owns kSlots 16-byte slots of its row, kThreads slots apart; a slot is
// V = 16 / sizeof(element) elements.  Slots are laid out from the 16-byte boundary at or before the row's first
// element -- `lead` is that element's offset into its slot, taken from the address, since rows may be windows of a
// wider buffer -- so whole slots are aligned wherever the row starts; the first and the last slot of a row may be
// partial.  A slot is stored with one 16-byte store where it lies inside [0, n) and element by element at the two ends:
// the element before the row and the elements past its end are never touched.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;   // threads per workgroup
constexpr int kSlots = 4;       // 16-byte slots per thread, kThreads slots apart

// blockIdx.x -> (row, block in row)
struct RowBlock { uint32_t row, blk; };
__device__ __forceinline__ RowBlock row_block(uint32_t blocks_per_row) {
  const uint32_t row = blockIdx.x / blocks_per_row;
  return {row, blockIdx.x - row * blocks_per_row};
}

// elements from the 16-byte boundary at or before y to y
template <typename T>
__device__ __forceinline__ int64_t row_lead(const T* y) {
  return (int64_t)((reinterpret_cast<uintptr_t>(y) / sizeof(T)) & (16 / sizeof(T) - 1));
}

template <typename T> struct Slot;
template <> struct Slot<double> { typedef double2 type; };
template <> struct Slot<float> { typedef float4 type; };

// v: the V elements of the slot that starts at element i0 of the row y[0 .. n)
template <typename T>
__device__ __forceinline__ void store_slot(T* __restrict__ y, int64_t n, int64_t i0, const T (&v)[16 / sizeof(T)]) {
  constexpr int V = 16 / sizeof(T);
  if (i0 >= 0 && i0 + V <= n) {
    typename Slot<T>::type q;
    if constexpr (V == 2) {
      q.x = v[0]; q.y = v[1];
    } else {
      q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    }
    *reinterpret_cast<typename Slot<T>::type*>(y + i0) = q;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (i0 + e >= 0 && i0 + e < n) y[i0 + e] = v[e];
  }
}

}  // namespace
