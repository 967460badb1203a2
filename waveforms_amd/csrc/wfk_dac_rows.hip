// wfk_dac_rows.hip -- volts to DAC codes for a batch of rows, every input row its own gain (LSB per unit of the
// signal) and offset (LSB): the last step before an upload to an AWG.  Per sample, in double,
//   v = fl(fl(x * gain) + offset)        (two roundings, no fused multiply-add: what NumPy's x * g + o computes)
//   q = rint(v)                          (round half to even)
//   c = 0 if v is NaN, lo if q < lo, hi if q > hi, q otherwise;   lo = -2^(bits - 1), hi = 2^(bits - 1) - 1
//   word = c * 2^shift as int16          (left-justifies a 12/14-bit converter in its 16-bit word)
// clamped in double before the conversion to an integer.  interleave = k in {1, 2}: output row g holds the input
// rows g k .. g k + k - 1 sample-interleaved, out[g, i k + j] = word[g k + j, i] (k = 2: I0 Q0 I1 Q1 ...).  An
// optional report counts, per INPUT row, the samples below lo, above hi and NaN.
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) over the OUTPUT rows; a slot is one 16-byte store of 8 codes,
// laid out from the 16-byte boundary at or before the output row's first code, so a workgroup spans 8192 codes.
// Under k = 2 the parity of an output position inside its slot is that of the row's lead: which input row feeds the
// even and which the odd elements of a slot is decided once per workgroup, and so are their gains and offsets (they
// arrive by scalar loads from the row table).  A slot reads one run of 8 consecutive samples (k = 1) or two runs of 4
// (k = 2); whether a run's address is 16-byte aligned is the same for every slot of a row, and where it is the run is
// taken with 16-byte loads, element loads otherwise and in the partial slots at the two ends of a row.
// Counting (the dac_rows_count kernels; dac_rows does none of it): the lane masks of the three comparisons are
// counted per wave, the waves' counts summed through LDS, and one thread per counter adds a non-zero sum to the
// row's int64 counter with one atomic add.  Integer sums: the report does not depend on the order of arrival.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)   // a rounded product and a rounded sum, as the host formula

namespace {

constexpr int kCodes = 8;   // int16 codes per 16-byte slot

// one INPUT row as the device reads it
struct DacRow {
  double gain, offset;
};

// what a workgroup's even (a) and odd (b) slot elements read and how they are scaled; k = 1: only a
template <typename T>
struct DacSide {
  const T* x;
  double gain, offset;
};

// M consecutive samples at p, widened; `vec`: p is 16-byte aligned
template <typename T, int M>
__device__ __forceinline__ void load_run(const T* __restrict__ p, bool vec, double (&r)[M]) {
  constexpr int per = 16 / sizeof(T);
  if (vec) {
    typedef typename Slot<T>::type Q;
#pragma unroll
    for (int q = 0; q < M / per; ++q) {
      const Q v = reinterpret_cast<const Q*>(p)[q];
      if constexpr (per == 2) {
        r[2 * q] = v.x; r[2 * q + 1] = v.y;
      } else {
        r[4 * q] = (double)v.x; r[4 * q + 1] = (double)v.y; r[4 * q + 2] = (double)v.z; r[4 * q + 3] = (double)v.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < M; ++e) r[e] = (double)p[e];
  }
}

// the 8 codes of the slot that starts at output position i0 of the row y[0 .. nout)
__device__ __forceinline__ void store_codes(int16_t* __restrict__ y, int64_t nout, int64_t i0,
                                            const int (&w)[kCodes]) {
  if (i0 >= 0 && i0 + kCodes <= nout) {
    uint4 q;
    q.x = (uint32_t)(w[0] & 0xffff) | ((uint32_t)w[1] << 16);
    q.y = (uint32_t)(w[2] & 0xffff) | ((uint32_t)w[3] << 16);
    q.z = (uint32_t)(w[4] & 0xffff) | ((uint32_t)w[5] << 16);
    q.w = (uint32_t)(w[6] & 0xffff) | ((uint32_t)w[7] << 16);
    *reinterpret_cast<uint4*>(y + i0) = q;
  } else {
#pragma unroll
    for (int e = 0; e < kCodes; ++e)
      if (i0 + e >= 0 && i0 + e < nout) y[i0 + e] = (int16_t)w[e];
  }
}

// One workgroup's share of output row `row`.  in: [out rows * K] rows of n samples; out: rows of K n codes.
template <typename T, int K, bool COUNT>
__device__ __forceinline__ void dac_block(const T* __restrict__ in, int64_t in_stride, int16_t* __restrict__ out,
                                          int64_t out_stride, const DacRow* __restrict__ tab,
                                          unsigned long long* __restrict__ counts, int64_t n, uint32_t row,
                                          uint32_t blk, double lo, double hi, int shift) {
  constexpr int64_t span = (int64_t)kSlots * kThreads * kCodes;
  __shared__ unsigned wave_counts[kThreads / 64][2 * 3];
  const int64_t nout = n * K;
  int16_t* __restrict__ y = out + (int64_t)row * out_stride;
  const int64_t lead = row_lead(y);
  const int64_t first = (int64_t)blk * span - lead;   // the block's first output position
  if (first >= nout) return;
  // the input rows of the even and the odd elements of every slot of this row, and the first sample each side
  // reads in the block (k = 2: position j is sample j >> 1 of row j & 1, and i0 = -lead modulo 8)
  const int64_t r0 = (int64_t)row * K;
  const int odd = K == 2 ? (int)(lead & 1) : 0;
  const int64_t ra = r0 + odd, rb = r0 + (K - 1 - odd);
  const DacSide<T> a{in + ra * in_stride, tab[ra].gain, tab[ra].offset};
  const DacSide<T> b{in + rb * in_stride, tab[rb].gain, tab[rb].offset};
  const int64_t sa = K == 2 ? first >> 1 : first, sb = (first + 1) >> 1;
  const bool vec_a = (((uintptr_t)a.x + (uintptr_t)(sa * (int64_t)sizeof(T))) & 15) == 0;
  const bool vec_b = (((uintptr_t)b.x + (uintptr_t)(sb * (int64_t)sizeof(T))) & 15) == 0;
  const bool vec = K == 2 ? vec_a && vec_b : vec_a;
  unsigned cnt[2][3] = {{0, 0, 0}, {0, 0, 0}};   // [even / odd elements][below, above, nan] of this wave
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int64_t base = first + (int64_t)u * kThreads * kCodes;
    if (base >= nout) break;   // (the same for every thread: what follows is converged)
    const int64_t i0 = base + (int64_t)threadIdx.x * kCodes;
    const bool whole = i0 >= 0 && i0 + kCodes <= nout;
    double x[kCodes];
    if (whole) {
      if constexpr (K == 1) {
        load_run<T, kCodes>(a.x + i0, vec, x);
      } else {
        double xa[kCodes / 2], xb[kCodes / 2];
        load_run<T, kCodes / 2>(a.x + (i0 >> 1), vec, xa);
        load_run<T, kCodes / 2>(b.x + ((i0 + 1) >> 1), vec, xb);
#pragma unroll
        for (int e = 0; e < kCodes / 2; ++e) { x[2 * e] = xa[e]; x[2 * e + 1] = xb[e]; }
      }
    } else {
#pragma unroll
      for (int e = 0; e < kCodes; ++e) {
        const int64_t j = i0 + e;
        const T* __restrict__ src = (K == 2 && (e & 1)) ? b.x : a.x;
        x[e] = (j >= 0 && j < nout) ? (double)src[K == 2 ? j >> 1 : j] : 0.0;
      }
    }
    int w[kCodes];
#pragma unroll
    for (int e = 0; e < kCodes; ++e) {
      const bool second = K == 2 && (e & 1);
      const double v = x[e] * (second ? b.gain : a.gain) + (second ? b.offset : a.offset);
      const double q = rint(v);
      const bool nan = v != v, below = q < lo, above = q > hi;
      const double c = nan ? 0.0 : below ? lo : above ? hi : q;
      w[e] = (int)c * (1 << shift);
      if constexpr (COUNT) {
        const bool live = whole || (i0 + e >= 0 && i0 + e < nout);
        cnt[second][0] += (unsigned)__popcll(__ballot(live && below));
        cnt[second][1] += (unsigned)__popcll(__ballot(live && above));
        cnt[second][2] += (unsigned)__popcll(__ballot(live && nan));
        // A lane mask is a pair of scalar registers, and left alone the compiler keeps all 96 of a thread's until
        // after the last slot (they spill).  The empty statements make the three sums exist here, in scalar registers.
#pragma unroll
        for (int c = 0; c < 3; ++c) asm volatile("" : "+s"(cnt[second][c]));
      }
    }
    if (i0 < nout) store_codes(y, nout, i0, w);
  }
  if constexpr (COUNT) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int s = 0; s < K; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) wave_counts[wave][3 * s + c] = cnt[s][c];
    }
    __syncthreads();
    if (threadIdx.x < 3 * K) {
      unsigned sum = 0;
#pragma unroll
      for (int wv = 0; wv < kThreads / 64; ++wv) sum += wave_counts[wv][threadIdx.x];
      const int64_t r = threadIdx.x < 3 ? ra : rb;
      if (sum) atomicAdd(counts + r * 3 + (threadIdx.x % 3), (unsigned long long)sum);
    }
  }
}

// in: [batch] rows of n samples; out: [batch / k] rows of k n codes that share no memory with them; counts (the
// _count kernel): [batch][3], zeroed before the launch.  Row strides in elements of their own side.
template <typename T>
__global__ void __launch_bounds__(kThreads)
    dac_rows(const T* __restrict__ in, int64_t in_stride, int16_t* __restrict__ out, int64_t out_stride,
             const DacRow* __restrict__ tab, int64_t n, uint32_t blocks_per_row, double lo, double hi, int shift,
             int k) {
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    dac_block<T, 2, false>(in, in_stride, out, out_stride, tab, nullptr, n, row, blk, lo, hi, shift);
  else
    dac_block<T, 1, false>(in, in_stride, out, out_stride, tab, nullptr, n, row, blk, lo, hi, shift);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    dac_rows_count(const T* __restrict__ in, int64_t in_stride, int16_t* __restrict__ out, int64_t out_stride,
                   const DacRow* __restrict__ tab, unsigned long long* __restrict__ counts, int64_t n,
                   uint32_t blocks_per_row, double lo, double hi, int shift, int k) {
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    dac_block<T, 2, true>(in, in_stride, out, out_stride, tab, counts, n, row, blk, lo, hi, shift);
  else
    dac_block<T, 1, true>(in, in_stride, out, out_stride, tab, counts, n, row, blk, lo, hi, shift);
}

}  // namespace

struct wfk_dac_rows_plan {
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  int bits = 0, shift = 0, k = 0;
  uint32_t blocks_per_row = 0;
  size_t rows_off = 0;
  DevBuf<char> tables;   // DacRow [batch]
};

namespace {

template <typename T>
void dac_launch(const wfk_dac_rows_plan* p, const void* in, int64_t in_stride, int16_t* out, int64_t out_stride,
                int64_t* counts, hipStream_t s) {
  const dim3 grid(p->blocks_per_row * (uint32_t)(p->batch / p->k));
  const DacRow* tab = DevTables::at<const DacRow>(p->tables.get(), p->rows_off);
  const double lo = -(double)(1 << (p->bits - 1)), hi = (double)((1 << (p->bits - 1)) - 1);
  if (counts)
    hipLaunchKernelGGL(dac_rows_count<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride, out, out_stride, tab,
                       (unsigned long long*)counts, p->n, p->blocks_per_row, lo, hi, p->shift, p->k);
  else
    hipLaunchKernelGGL(dac_rows<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride, out, out_stride, tab, p->n,
                       p->blocks_per_row, lo, hi, p->shift, p->k);
}

}  // namespace

extern "C" {

int wfk_dac_rows_plan_destroy(wfk_dac_rows_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_dac_rows_kernel_name(const wfk_dac_rows_plan* p, int with_counts) {
  if (!p) return "";
  if (with_counts) return p->kind == WFK_OUT_F32 ? "dac_rows_count<float>" : "dac_rows_count<double>";
  return p->kind == WFK_OUT_F32 ? "dac_rows<float>" : "dac_rows<double>";
}

// the converter side of a plan's arguments: the format, the interleave, one finite gain and offset per row
int wfk_internal_dac_check(int32_t batch, const double* gain_host, const double* offset_host, int bits, int shift,
                           int interleave) {
  if (bits < 2 || bits > 16) return wfk_fail(WFK_EINVAL, "dac rows plan: bits must lie in [2, 16]");
  if (shift < 0 || shift > 16 - bits) return wfk_fail(WFK_EINVAL, "dac rows plan: shift must lie in [0, 16 - bits]");
  if (interleave != 1 && interleave != 2) return wfk_fail(WFK_EINVAL, "dac rows plan: interleave must be 1 or 2");
  if (batch % interleave)
    return wfk_fail(WFK_EINVAL, "dac rows plan: " + std::to_string(batch) + " rows are no multiple of the interleave");
  for (int32_t r = 0; r < batch; ++r) {
    if (!std::isfinite(gain_host[r])) return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": gain is not finite");
    if (!std::isfinite(offset_host[r]))
      return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": offset is not finite");
  }
  return WFK_OK;
}

int wfk_dac_rows_plan_create(int64_t n, int32_t batch, int kind, const double* gain_host, const double* offset_host,
                             int bits, int shift, int interleave, wfk_dac_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 0 || batch < 1 || !gain_host || !offset_host) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  if (const int rc = wfk_check_kind(kind)) return rc;
  if (const int rc = wfk_internal_dac_check(batch, gain_host, offset_host, bits, shift, interleave)) return rc;
  if (n > INT64_MAX / interleave) return wfk_fail(WFK_EINVAL, "dac rows plan: batch * n too large for one launch");
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("dac rows plan", interleave * n, (int64_t)kCodes * kThreads * kSlots, kCodes - 1,
                                    batch / interleave, &bpr))
    return rc;
  std::vector<DacRow> rows((size_t)batch);
  for (int32_t r = 0; r < batch; ++r) rows[r] = DacRow{gain_host[r], offset_host[r]};
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_dac_rows_plan> p(new wfk_dac_rows_plan());
  p->n = n; p->batch = batch; p->kind = kind;
  p->bits = bits; p->shift = shift; p->k = interleave;
  p->blocks_per_row = bpr;
  DevTables tab;
  p->rows_off = tab.add(rows);
  if (const int rc = wfk_upload_tables("dac rows plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the dac rows plan");
}

int wfk_dac_rows_apply(wfk_dac_rows_plan* p, const void* in_dev, int64_t in_stride, int16_t* out_dev,
                       int64_t out_stride, int64_t* counts_dev, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, p->batch, 3};
  // nothing to quantise (the pointers of empty rows may be null); the report is still zeroed
  if (p->n == 0) return wfk_zero_report("dac rows", report, s);
  // a lone output row's stride is not read
  if (const int rc = wfk_row_rule("dac rows", {{"in", in_dev, p->batch, in_stride, p->n, wfk_elem_size(p->kind)}},
                                  {"out", out_dev, p->batch / p->k, out_stride, p->k * p->n, sizeof(int16_t), false},
                                  kRowsAligned | kRowsDisjoint, wfk_fail, report))
    return rc;
  if (const int rc = wfk_zero_report("dac rows", report, s)) return rc;
  if (p->kind == WFK_OUT_F32)
    dac_launch<float>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  else
    dac_launch<double>(p, in_dev, in_stride, out_dev, out_stride, counts_dev, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "dac rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
