// wfk_shift_rows.hip -- per-row delay in time, the reference's shift(signal, delay, dt) (distortion.py:12-39) for a
// batch of rows, every row its own delay.  The host splits a delay with the reference's own expressions,
//   p = int(delay // dt),   delta = delay / dt - p   (delta in [0, 1]; 1.0 // 0.1 is 9 and delta then 1: legal),
// and the device computes, with x[k] = 0 for k < 0,
//   s[j] = (1 - delta) x[j] + delta x[j - 1]   if delta > 0,      s[j] = x[j] otherwise (a copy: no arithmetic),
//   y[i] = s[i - p]   if 0 <= i - p < n,       0 otherwise
// -- linear interpolation between neighbours and zero fill at both ends (nothing comes in from past the end of a
// row: the reference truncates its 'same' convolution before it shifts).  One read and one write per sample.
// Departures from the reference, on purpose: rows keep n samples for n < 3 (np.convolve 'same' returns 3 there), and
// the reference's zero tap on x[j + 1] is not multiplied (an inf at j + 1 does not turn sample j into NaN).
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) over the OUTPUT rows: the row's table entry (p, 1 - delta,
// delta, has_frac) arrives by scalar loads, and the delta = 0 path is a wave-uniform branch into a loop that only
// copies.  The source index i - p is misaligned against the destination whenever p is not a multiple of the slot: the
// loads are element loads.  A lane needs one sample more
// than it stores, x[j0 - 1]: it loads it (the neighbouring lane has just pulled the same line into the cache; a
// cross-lane move costs more instructions than the load).  A workgroup whose outputs are all zero fill
// (the head or the tail of a shifted row, every block of a row with |p| >= n) stores zeros and issues no loads.
// float rows are computed in double and rounded once on the store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)   // two rounded products and one rounded sum, as the host formula

namespace {

// 1: a lane takes x[j0 - 1] from the lane below it instead of loading it (an experiment's switch)
#ifndef WFK_SHIFT_NEIGHBOUR_SHFL
#define WFK_SHIFT_NEIGHBOUR_SHFL 0
#endif

// one row as the device reads it
struct ShiftRow {
  int64_t p;        // whole samples (either sign)
  double w0, w1;    // 1 - delta, delta
  int32_t frac;     // delta > 0
  int32_t pad;
};

// the V outputs of the slot that starts at output sample i0 (source sample j0 = i0 - p); ZERO: all zero fill
template <typename T, bool FRAC, bool ZERO>
__device__ __forceinline__ void shift_slot(const T* __restrict__ x, T* __restrict__ y, int64_t n, int64_t i0,
                                           int64_t j0, double w0, double w1) {
  constexpr int V = 16 / sizeof(T);
  T v[V];
  if constexpr (ZERO) {
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = T(0);
  } else if constexpr (FRAC) {
    const int64_t jm = j0 - 1;
    double cur[V];
#pragma unroll
    for (int e = 0; e < V; ++e) cur[e] = (j0 + e >= 0 && j0 + e < n) ? (double)x[j0 + e] : 0.0;
    double prev;
#if WFK_SHIFT_NEIGHBOUR_SHFL
    // x[j0 - 1] is the last sample of the lane below (it owns the slot before this one and is active if this one
    // is); the first lane of a wave has no such neighbour and loads it
    prev = __shfl_up(cur[V - 1], 1);
    if ((threadIdx.x & 63) == 0) prev = (jm >= 0 && jm < n) ? (double)x[jm] : 0.0;
#else
    prev = (jm >= 0 && jm < n) ? (double)x[jm] : 0.0;
#endif
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int64_t j = j0 + e;
      v[e] = (j >= 0 && j < n) ? (T)(w0 * cur[e] + w1 * prev) : T(0);
      prev = cur[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int64_t j = j0 + e;
      v[e] = (j >= 0 && j < n) ? x[j] : T(0);
    }
  }
  store_slot(y, n, i0, v);
}

template <typename T, bool FRAC, bool ZERO>
__device__ __forceinline__ void shift_block(const T* __restrict__ x, T* __restrict__ y, int64_t n, int64_t first,
                                            int64_t p, double w0, double w1) {
  constexpr int V = 16 / sizeof(T);
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int64_t i0 = first + ((int64_t)u * kThreads + threadIdx.x) * V;
    if (i0 >= n) break;
    shift_slot<T, FRAC, ZERO>(x, y, n, i0, i0 - p, w0, w1);
  }
}

// in / out: [batch] rows of n samples, row strides in elements; out rows share no memory with in rows
template <typename T>
__global__ void __launch_bounds__(kThreads)
    shift_rows(const T* __restrict__ in, int64_t in_stride, T* __restrict__ out, int64_t out_stride,
               const ShiftRow* __restrict__ tab, int64_t n, uint32_t blocks_per_row) {
  constexpr int V = 16 / sizeof(T);
  const auto [row, blk] = row_block(blocks_per_row);
  const int64_t p = tab[row].p;
  const double w0 = tab[row].w0, w1 = tab[row].w1;
  const bool frac = tab[row].frac != 0;
  const T* __restrict__ x = in + (int64_t)row * in_stride;
  T* __restrict__ y = out + (int64_t)row * out_stride;
  const int64_t lead = row_lead(y);
  const int64_t first = (int64_t)blk * (kSlots * kThreads * V) - lead;   // the block's first output sample
  if (first >= n) return;
  // sources of the block's outputs: [first - p, first - p + block span); none inside [0, n): zero fill, no loads
  const int64_t span = (int64_t)kSlots * kThreads * V;
  if (p >= n || p <= -n || first + span <= p || first - p >= n)
    shift_block<T, false, true>(x, y, n, first, p, w0, w1);
  else if (frac)
    shift_block<T, true, false>(x, y, n, first, p, w0, w1);
  else
    shift_block<T, false, false>(x, y, n, first, p, w0, w1);
}

}  // namespace

struct wfk_shift_rows_plan {
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  uint32_t blocks_per_row = 0;
  size_t rows_off = 0;
  DevBuf<char> tables;   // ShiftRow [batch]
};

extern "C" {

int wfk_shift_rows_plan_destroy(wfk_shift_rows_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_shift_rows_kernel_name(const wfk_shift_rows_plan* p) {
  if (!p) return "";
  return p->kind == WFK_OUT_F32 ? "shift_rows<float>" : "shift_rows<double>";
}

int wfk_shift_rows_plan_create(int64_t n, int32_t batch, int kind, const int64_t* points_host,
                               const double* delta_host, wfk_shift_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 0 || batch < 1 || !points_host || !delta_host) return wfk_fail(WFK_EINVAL, "bad shift rows plan arguments");
  if (const int rc = wfk_check_kind(kind)) return rc;
  const int V = 16 / (int)wfk_elem_size(kind);
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("shift rows plan", n, V * kThreads * kSlots, V - 1, batch, &bpr)) return rc;
  std::vector<ShiftRow> rows((size_t)batch);
  for (int32_t r = 0; r < batch; ++r) {
    const double d = delta_host[r];
    if (!(d >= 0.0 && d <= 1.0))   // (NaN fails both)
      return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": delta must lie in [0, 1]");
    rows[r] = ShiftRow{points_host[r], 1.0 - d, d, d > 0.0 ? 1 : 0, 0};
  }
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_shift_rows_plan> p(new wfk_shift_rows_plan());
  p->n = n; p->batch = batch; p->kind = kind;
  p->blocks_per_row = bpr;
  DevTables tab;
  p->rows_off = tab.add(rows);
  if (const int rc = wfk_upload_tables("shift rows plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the shift rows plan");
}

int wfk_shift_rows_apply(wfk_shift_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                         int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;   // nothing to move (the pointers of empty rows may be null)
  const size_t es = wfk_elem_size(p->kind);
  if (((uintptr_t)in_dev | (uintptr_t)out_dev) & (es - 1)) return wfk_fail(WFK_EINVAL, "rows are not aligned to their element");
  if (const int rc = wfk_check_rows("shift rows", p->n, es, in_dev, p->batch, in_stride, out_dev, p->batch, out_stride, true))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const dim3 grid(p->blocks_per_row * (uint32_t)p->batch);
  const ShiftRow* tab = DevTables::at<const ShiftRow>(p->tables.get(), p->rows_off);
  if (p->kind == WFK_OUT_F32)
    hipLaunchKernelGGL(shift_rows<float>, grid, dim3(kThreads), 0, s, (const float*)in_dev, in_stride,
                       (float*)out_dev, out_stride, tab, p->n, p->blocks_per_row);
  else
    hipLaunchKernelGGL(shift_rows<double>, grid, dim3(kThreads), 0, s, (const double*)in_dev, in_stride,
                       (double*)out_dev, out_stride, tab, p->n, p->blocks_per_row);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "shift rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
