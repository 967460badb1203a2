// wfk_curve_rows.hip -- a calibration curve over sample VALUES for a batch of rows, every row its own knots: flux or
// detuning to volts through a measured monotone curve, an amplifier's compression table, a DAC's INL table.  Row r has
// K knots xp[0 .. K) (finite, strictly increasing, 2 <= K <= WFK_CURVE_MAX_KNOTS), values fp[0 .. K) (finite), and what
// a sample below / above the knots becomes, left / right (any double).  The host computes, once,
//   slope[j] = fl(fl(fp[j + 1] - fp[j]) / fl(xp[j + 1] - xp[j]))
// and the device, per sample, in double (a float sample is widened first, the result rounded once on the store),
//   x is NaN           -> y = x                              (counted: nan)
//   x < xp[0]          -> y = left                           (counted: below; -inf too)
//   x > xp[K - 1]      -> y = right                          (counted: above; +inf too)
//   j = the largest index with xp[j] <= x
//   x == xp[j]         -> y = fp[j]                          (j = K - 1 is this case)
//   otherwise          -> y = fl(fl(slope[j] * fl(x - xp[j])) + fp[j])       (no fused multiply-add)
// -- np.interp(x, xp, fp, left, right), bit for bit.
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) over the OUTPUT rows.  The row's scalars (CurveRow) arrive by
// scalar loads; the workgroup copies the row's knots (xp, fp, slope: 24 bytes a knot) and its bucket table into dynamic
// LDS, sized by the plan to its largest row, and then walks `spans` consecutive spans of kSlots * kThreads slots, so the
// copy is paid once for spans * 32 KiB of samples.  The search: a uniform bucket table over [xp[0], xp[K - 1]] (a power
// of two >= 2 K buckets, built by the host) gives a bracket [lo, hi] of knot indices, a bisection narrows it (no step
// where the bracket is one knot), and a fix-up against xp[j] and xp[j + 1] makes j exact whatever the rounding of the
// bucket index did -- a row without buckets (nb = 0) brackets [0, K - 1] and is plain bisection.  A thread loads its
// kSlots slots, then computes and stores them: in == out with equal strides is allowed (no __restrict__ on the two).
// An input that is not 16-byte aligned where the output's slots are uses element loads.
// Counting (the curve_rows_counts kernels; curve_rows does none of it): every lane counts its own samples, a wave adds
// its lanes' counts by shuffles, the waves' sums meet in LDS, and one thread per counter adds a non-zero sum to the
// row's int64 counter with one atomic add.  Integer sums: the report does not depend on the order of arrival.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)   // a rounded difference, a rounded product and a rounded sum, as the host formula

#include "wfk_curve_dev.h"       // CurveRow, Knots, curve_at; the host's check and table builder

namespace {

constexpr int kMaxSpans = 16;   // spans a workgroup may walk

// One workgroup's share of row `row`: `spans` consecutive spans from span blk * spans on.
template <typename T, bool COUNT>
__device__ __forceinline__ void curve_block(const T* in, int64_t in_stride, T* out, int64_t out_stride,
                                            const CurveRow* __restrict__ rows, const double* __restrict__ knots,
                                            const uint32_t* __restrict__ buckets,
                                            unsigned long long* __restrict__ counts, int64_t n, uint32_t blocks_per_row,
                                            int spans, int lds_knots) {
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t span = (int64_t)kSlots * kThreads * V;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  // [waves][4] unsigned (the counts of the waves), xp, fp, slope: lds_knots doubles each, then the buckets
  unsigned* wave_counts = reinterpret_cast<unsigned*>(lds);
  double* sx = reinterpret_cast<double*>(lds + 64);
  double* sf = sx + lds_knots;
  double* ss = sf + lds_knots;
  uint32_t* sb = reinterpret_cast<uint32_t*>(ss + lds_knots);

  const auto [r, blk] = row_block(blocks_per_row);
  const T* x = in + (int64_t)r * in_stride;
  T* y = out + (int64_t)r * out_stride;
  const int64_t lead = row_lead(y);
  const int64_t begin = (int64_t)blk * spans * span - lead;   // the block's first output sample
  if (begin >= n) return;
  const CurveRow row = rows[r];
  {
    const double* __restrict__ g = knots + row.off;
    for (int i = threadIdx.x; i < row.K; i += kThreads) {
      sx[i] = g[i];
      sf[i] = g[row.K + i];
      ss[i] = g[2 * row.K + i];
    }
    const uint32_t* __restrict__ gb = buckets + row.boff;
    for (int i = threadIdx.x; i < row.nb; i += kThreads) sb[i] = gb[i];
  }
  __syncthreads();
  const Knots t{sx, sf, ss, sb};
  // the slots of a row start 16-byte aligned in the output; are they in the input
  const bool vec = (((uintptr_t)x - (uintptr_t)(lead * (int64_t)sizeof(T))) & 15) == 0;
  unsigned cnt[3] = {0, 0, 0};   // [below, above, nan] of this lane
  for (int s = 0; s < spans; ++s) {
    const int64_t first = begin + (int64_t)s * span;
    if (first >= n) break;   // (the same for every thread)
    T v[kSlots][V];
    // every load of the thread before its first store: in place, a slot is read before it is written
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int64_t i0 = first + ((int64_t)u * kThreads + threadIdx.x) * V;
      if (i0 >= 0 && i0 + V <= n && vec) {
        const typename Slot<T>::type q = *reinterpret_cast<const typename Slot<T>::type*>(x + i0);
        if constexpr (V == 2) {
          v[u][0] = q.x; v[u][1] = q.y;
        } else {
          v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) v[u][e] = (i0 + e >= 0 && i0 + e < n) ? x[i0 + e] : T(0);
      }
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int64_t i0 = first + ((int64_t)u * kThreads + threadIdx.x) * V;
      if (i0 >= n) break;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double xe = (double)v[u][e];
        const bool nan = xe != xe, below = xe < row.x0, above = xe > row.xl;
        // a sample outside the knots searches for x0: every lane of a wave stays in one loop
        const double inside = curve_at(t, row, (nan || below || above) ? row.x0 : xe);
        v[u][e] = (T)(nan ? xe : below ? row.left : above ? row.right : inside);
        if constexpr (COUNT) {
          const bool live = i0 + e >= 0 && i0 + e < n;
          cnt[0] += live && below;
          cnt[1] += live && above;
          cnt[2] += live && nan;
        }
      }
      store_slot(y, n, i0, v[u]);
    }
  }
  if constexpr (COUNT) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) cnt[c] += __shfl_xor(cnt[c], d);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) wave_counts[4 * wave + c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      unsigned sum = 0;
#pragma unroll
      for (int wv = 0; wv < kThreads / 64; ++wv) sum += wave_counts[4 * wv + threadIdx.x];
      if (sum) atomicAdd(counts + (int64_t)r * 3 + threadIdx.x, (unsigned long long)sum);
    }
  }
}

// in / out: [batch] rows of n samples, row strides in elements; the same rows (in place) or rows that share no memory.
// counts (the _counts kernel): [batch][3], zeroed before the launch.  Dynamic LDS: 64 + 24 lds_knots + 4 * the largest
// nb of the plan.
template <typename T>
__global__ void __launch_bounds__(kThreads)
    curve_rows(const T* in, int64_t in_stride, T* out, int64_t out_stride, const CurveRow* __restrict__ rows,
               const double* __restrict__ knots, const uint32_t* __restrict__ buckets, int64_t n,
               uint32_t blocks_per_row, int spans, int lds_knots) {
  curve_block<T, false>(in, in_stride, out, out_stride, rows, knots, buckets, nullptr, n, blocks_per_row, spans,
                        lds_knots);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    curve_rows_counts(const T* in, int64_t in_stride, T* out, int64_t out_stride, const CurveRow* __restrict__ rows,
                      const double* __restrict__ knots, const uint32_t* __restrict__ buckets,
                      unsigned long long* __restrict__ counts, int64_t n, uint32_t blocks_per_row, int spans,
                      int lds_knots) {
  curve_block<T, true>(in, in_stride, out, out_stride, rows, knots, buckets, counts, n, blocks_per_row, spans,
                       lds_knots);
}

// an experiment's switch (tools/curve_rows_bench.py), read when a plan is made: the value of `name`, or `otherwise`
int env_int(const char* name, int otherwise) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoi(v) : otherwise;
}

}  // namespace

struct wfk_curve_rows_plan {
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  uint32_t blocks_per_row = 0;
  int spans = 1, lds_knots = 0;
  size_t lds_bytes = 0;
  size_t rows_off = 0, knots_off = 0, buckets_off = 0;
  DevBuf<char> tables;   // CurveRow [batch], the knots, the buckets
};

namespace {

template <typename T>
void curve_launch(const wfk_curve_rows_plan* p, const void* in, int64_t in_stride, void* out, int64_t out_stride,
                  int64_t* counts, hipStream_t s) {
  const dim3 grid(p->blocks_per_row * (uint32_t)p->batch);
  const CurveRow* rows = DevTables::at<const CurveRow>(p->tables.get(), p->rows_off);
  const double* knots = DevTables::at<const double>(p->tables.get(), p->knots_off);
  const uint32_t* buckets = DevTables::at<const uint32_t>(p->tables.get(), p->buckets_off);
  if (counts)
    hipLaunchKernelGGL(curve_rows_counts<T>, grid, dim3(kThreads), p->lds_bytes, s, (const T*)in, in_stride, (T*)out,
                       out_stride, rows, knots, buckets, (unsigned long long*)counts, p->n, p->blocks_per_row,
                       p->spans, p->lds_knots);
  else
    hipLaunchKernelGGL(curve_rows<T>, grid, dim3(kThreads), p->lds_bytes, s, (const T*)in, in_stride, (T*)out,
                       out_stride, rows, knots, buckets, p->n, p->blocks_per_row, p->spans, p->lds_knots);
}

}  // namespace

extern "C" {

int wfk_curve_rows_plan_destroy(wfk_curve_rows_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_curve_rows_kernel_name(const wfk_curve_rows_plan* p, int with_counts) {
  if (!p) return "";
  if (with_counts) return p->kind == WFK_OUT_F32 ? "curve_rows_counts<float>" : "curve_rows_counts<double>";
  return p->kind == WFK_OUT_F32 ? "curve_rows<float>" : "curve_rows<double>";
}

int wfk_curve_rows_plan_create(int64_t n, int32_t batch, int kind, const int64_t* knot_ptr, const double* xp,
                               const double* fp, const double* left, const double* right,
                               wfk_curve_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (const int rc = curve_check(n, batch, kind, knot_ptr, xp, fp)) return rc;
  // the spans a workgroup walks: the copy of a row's tables (28 or 32 bytes a knot, from L2) against the 32 KiB a span
  // streams -- one span per 4 KiB of tables (DESIGN.md has the measurement), while the grid keeps >= 2048 workgroups
  const int V = 16 / (int)wfk_elem_size(kind);
  const int64_t span = (int64_t)V * kThreads * kSlots;
  const bool use_buckets = env_int("WFK_CURVE_BUCKETS", 1) != 0;
  const CurveTables ct = curve_build(batch, knot_ptr, xp, fp, left, right, use_buckets, (size_t)-1);
  const int max_k = ct.max_k;
  const size_t lds_bytes = 64 + ct.lds_bytes();
  int spans = (int)std::min<size_t>(kMaxSpans, std::max<size_t>(1, (lds_bytes - 64 + 4095) / 4096));
  const int64_t row_spans = n / span + 1;
  while (spans > 1 && (row_spans + spans - 1) / spans * batch < 2048) --spans;
  spans = std::min(kMaxSpans, std::max(1, env_int("WFK_CURVE_SPANS", spans)));
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("curve rows plan", n, span * spans, V - 1, batch, &bpr)) return rc;

  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_curve_rows_plan> p(new wfk_curve_rows_plan());
  p->n = n; p->batch = batch; p->kind = kind;
  p->blocks_per_row = bpr;
  p->spans = spans;
  p->lds_knots = max_k;
  p->lds_bytes = lds_bytes;
  DevTables tab;
  p->rows_off = tab.add(ct.rows);
  p->knots_off = tab.add(ct.knots);
  p->buckets_off = tab.add(ct.buckets);
  if (const int rc = wfk_upload_tables("curve rows plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the curve rows plan");
}

int wfk_curve_rows_spans(const wfk_curve_rows_plan* p) { return p ? p->spans : 0; }

int wfk_curve_rows_apply(wfk_curve_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                         int64_t out_stride, int64_t* counts_dev, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, p->batch, 3};
  // nothing to look up (the pointers of empty rows may be null); the report is still zeroed
  if (p->n == 0) return wfk_zero_report("curve rows", report, s);
  const size_t es = wfk_elem_size(p->kind);
  // exactly in place -- the same rows on both sides -- or two extents that do not meet
  const bool in_place = in_dev == out_dev && in_stride == out_stride;
  if (const int rc = wfk_row_rule("curve rows", {{"in", in_dev, p->batch, in_stride, p->n, es}},
                                  {"out", out_dev, p->batch, out_stride, p->n, es},
                                  kRowsAligned | (in_place ? 0u : kRowsDisjoint), wfk_fail, report))
    return rc;
  if (const int rc = wfk_zero_report("curve rows", report, s)) return rc;
  if (p->kind == WFK_OUT_F32)
    curve_launch<float>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  else
    curve_launch<double>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "curve rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
