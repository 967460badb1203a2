// wfk_marker_rows.hip -- gate markers for a batch of sampled rows: the marker line of an AWG channel, high from `lead`
// samples before a pulse to `trail` samples after it, as bytes or written into one bit of the int16 DAC codes that
// wfk_dac_rows.hip produced.  group = k in {1, 2}: marker row g is driven by the input rows g k .. g k + k - 1 (k = 2:
// the I and Q of a pair, as the DAC stage's interleave pairs them).  Per marker row g, exact and in integers:
//   active[g, i] = any_j  fabs((double)x[g k + j, i]) > threshold[g]      (NaN inactive, +-inf active)
//   m[g, i]      = any    active[g, j]  for j in [i - trail[g], i + lead[g]], clipped to [0, n)
// bytes:  out[g, i] = m[g, i];   codes (in place):  codes[g, p] = (codes[g, p] & ~(1 << bit)) | (m[g, p / k] << bit).
// An optional report counts, per marker row, [high, pulses]: the samples with m = 1 and the rising edges of m (a
// marker that is high at i = 0 counts as one).
//
// Execution form.  A row-slot kernel (wfk_rows_dev.h) over the OUTPUT row; a slot is one 16-byte access: 16 markers,
// or 8 codes (8 samples at k = 1, 4 at k = 2), so a workgroup spans 16384, 8192 or 4096 samples.  A workgroup works
// on a bitmap in LDS, one bit per sample, over its span and a halo of trail (+ 1 with counts: m of the sample before
// the span decides whether the span starts with a rising edge) samples before and lead samples after it, clipped to
// the row.  The bitmap's first bit is a sample whose address in the (first) input row is 16-byte aligned, so
// 1. every thread reads runs of 8 consecutive samples, with 16-byte loads (element loads for a second row of another
//    alignment and where a run crosses a row end), and writes their 8 comparison bits as ONE BYTE of the bitmap;
// 2. the waves collect which bitmap words are not zero (one bit per word, by ballot);
// 3. every bitmap word is dilated on its own: the bits of the word smeared in the word by shift-doubling, and the
//    carry from outside it taken from the nearest set bit before and after the word, found through the map of step 2
//    -- the cost is per word, whatever lead and trail are -- and the result is clipped to the row;
// 4. every thread stores its slots: 16 bits of the dilated bitmap spread to 16 bytes, or 8 codes loaded, one bit of
//    each replaced and stored; element by element in the partial slots at the two ends of a row.
// Counting (the _count kernels; the others do none of it): popcounts of the dilated words restricted to the samples
// the workgroup owns (those whose first output position lies in its span), summed per wave by shuffles and across
// the waves through LDS; one thread per counter adds a non-zero sum to the row's int64 counter with one atomic add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

namespace {

constexpr int kMarkers = 16;   // uint8 markers per 16-byte slot
constexpr int kCodes = 8;      // int16 codes per 16-byte slot
constexpr int kRun = 8;        // samples per run: one byte of the bitmap
// bitmap words: up to 3 (alignment) + 4096 + 1 bits before the span, 16384 in it, 4096 after it, and one word more so
// that a 64-bit window may start at any bit of the last word in use
constexpr int kWords = 392;
constexpr int kMapWords = (kWords + 63) / 64;   // words of the non-zero map
static_assert(3 + WFK_MARKER_MAX_EDGE + 1 + kSlots * kThreads * kMarkers + WFK_MARKER_MAX_EDGE <= (kWords - 1) * 64,
              "the bitmap does not hold a span and its halo");
static_assert(kWords <= 2 * kThreads, "a thread dilates two words");

// a workgroup's LDS: the comparison bits, the dilated bits, which words of the first are not zero, the waves' counts
struct MarkerLds {
  uint64_t act[kWords], mark[kWords], nonzero[kMapWords];
  unsigned wave_counts[kThreads / 64][2];
};

// one MARKER row as the device reads it
struct MarkRow {
  double threshold;
  int32_t lead, trail;
};

// the comparison bits of the 8 samples at p; `vec`: p is 16-byte aligned
template <typename T>
__device__ __forceinline__ unsigned run_mask(const T* __restrict__ p, bool vec, double thr) {
  constexpr int per = 16 / sizeof(T);
  unsigned m = 0;
  if (vec) {
    typedef typename Slot<T>::type Q;
#pragma unroll
    for (int q = 0; q < kRun / per; ++q) {
      const Q v = reinterpret_cast<const Q*>(p)[q];
      if constexpr (per == 2) {
        m |= (unsigned)(fabs(v.x) > thr) << (2 * q) | (unsigned)(fabs(v.y) > thr) << (2 * q + 1);
      } else {
        m |= (unsigned)(fabs((double)v.x) > thr) << (4 * q) | (unsigned)(fabs((double)v.y) > thr) << (4 * q + 1) |
             (unsigned)(fabs((double)v.z) > thr) << (4 * q + 2) | (unsigned)(fabs((double)v.w) > thr) << (4 * q + 3);
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) m |= (unsigned)(fabs((double)p[e]) > thr) << e;
  }
  return m;
}

// the bits [lo, hi) of the bitmap that fall into the word whose first bit is w0
__device__ __forceinline__ uint64_t word_range(int64_t w0, int64_t lo, int64_t hi) {
  const int64_t a = lo - w0 > 0 ? lo - w0 : 0, b = hi - w0 < 64 ? hi - w0 : 64;
  if (a >= b) return 0;
  return (b == 64 ? ~0ull : (1ull << b) - 1) & (~0ull << a);
}

// 64 bits of the bitmap from bit q on (the word after q's is read too: kWords leaves one for it)
__device__ __forceinline__ uint64_t window(const uint64_t* map, int64_t q) {
  const int w = (int)(q >> 6), s = (int)(q & 63);
  const uint64_t lo = map[w], hi = map[w + 1];
  return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// One workgroup's share of marker row `row`.  in: [rows * K] rows of n samples; out: rows of n bytes (CODES: of K n
// codes, read and written).
template <typename T, int K, bool CODES, bool COUNT>
__device__ __forceinline__ void marker_block(MarkerLds& lds, const T* __restrict__ in, int64_t in_stride,
                                             void* out, int64_t out_stride, const MarkRow* __restrict__ tab,
                                             unsigned long long* __restrict__ counts, int64_t n, uint32_t row,
                                             uint32_t blk, int bit) {
  typedef typename std::conditional<CODES, uint16_t, uint8_t>::type O;
  constexpr int E = CODES ? kCodes : kMarkers;             // output elements per slot
  constexpr int sh = CODES && K == 2 ? 1 : 0;              // output position p holds sample p >> sh
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t span = (int64_t)kSlots * kThreads * E;
  uint64_t* act = lds.act;
  uint64_t* mark = lds.mark;
  uint64_t* nonzero = lds.nonzero;
  const int tid = threadIdx.x;
  const int64_t nout = n << sh;
  O* y = static_cast<O*>(out) + (int64_t)row * out_stride;
  const int64_t first = (int64_t)blk * span - row_lead(y);   // the block's first output position
  if (first >= nout) return;
  const double thr = tab[row].threshold;
  const int lead = tab[row].lead, trail = tab[row].trail;
  // samples: the span is [fs, s_hi], what the block owns [c_lo, c_hi), what the dilation reads [ld_lo, ld_hi]
  const int64_t fs = first >> sh;
  const int64_t s_hi = ((first + span - 1) >> sh) < n - 1 ? (first + span - 1) >> sh : n - 1;
  const int64_t need_lo = fs - (COUNT ? 1 : 0) - trail;
  const int64_t ld_lo = need_lo > 0 ? need_lo : 0, ld_hi = s_hi + lead < n - 1 ? s_hi + lead : n - 1;
  const T* __restrict__ xa = in + (int64_t)row * K * in_stride;
  const T* __restrict__ xb = xa + (K - 1) * in_stride;
  // bit 0 of the bitmap: the sample at or before need_lo whose address in row a is 16-byte aligned
  const int64_t lin = row_lead(xa);
  const int64_t b0 = ((need_lo + lin) & ~(int64_t)(V - 1)) - lin;
  const bool vec_b = K == 1 || row_lead(xb) == lin;
  const int words = (int)((ld_hi - b0) >> 6) + 2;   // <= kWords; the last one is there for window()

  // 1. the comparison bits, a byte per run of 8 samples
  unsigned char* act_bytes = reinterpret_cast<unsigned char*>(act);
#pragma unroll 4
  for (int r = tid; r < words * 8; r += kThreads) {
    const int64_t j0 = b0 + (int64_t)r * kRun;
    unsigned m = 0;
    if (j0 + kRun > ld_lo && j0 <= ld_hi) {
      if (j0 >= 0 && j0 + kRun <= n) {
        m = run_mask<T>(xa + j0, true, thr);
        if constexpr (K == 2) m |= run_mask<T>(xb + j0, vec_b, thr);
      } else {
#pragma unroll
        for (int e = 0; e < kRun; ++e) {
          const int64_t j = j0 + e;
          if (j >= 0 && j < n) {
            bool a = fabs((double)xa[j]) > thr;
            if constexpr (K == 2) a = a || fabs((double)xb[j]) > thr;
            m |= (unsigned)a << e;
          }
        }
      }
    }
    act_bytes[r] = (unsigned char)m;
  }
  __syncthreads();

  // 2. which words are not zero
#pragma unroll
  for (int w = tid; w < kMapWords * 64; w += kThreads) {
    const uint64_t nz = __ballot(w < words && act[w] != 0);
    if ((tid & 63) == 0) nonzero[w >> 6] = nz;
  }
  __syncthreads();

  // 3. dilation, word by word
  const int up = trail < 63 ? trail : 63, down = lead < 63 ? lead : 63;
  const int64_t row_lo = -b0 > 0 ? -b0 : 0, row_hi = n - b0;   // the bits of the samples of the row
  for (int w = tid; w < words; w += kThreads) {
    const uint64_t a = act[w];
    uint64_t m = a, s = a;
    for (int c = 0; c < up;) {   // towards later samples, by `up`
      const int step = c + 1 < up - c ? c + 1 : up - c;
      s |= s << step;
      c += step;
    }
    m |= s;
    s = a;
    for (int c = 0; c < down;) {   // towards earlier samples, by `down`
      const int step = c + 1 < down - c ? c + 1 : down - c;
      s |= s >> step;
      c += step;
    }
    m |= s;
    if (trail) {   // the nearest set bit before the word reaches into it from below
      int j = w >> 6;
      uint64_t nz = nonzero[j] & ((1ull << (w & 63)) - 1);
      while (!nz && j > 0) nz = nonzero[--j];
      if (nz) {
        const int hw = 64 * j + 63 - __builtin_clzll(nz);
        // the last bit it sets, counted from the word's first
        const int reach = 64 * hw + 63 - __builtin_clzll(act[hw]) + trail - 64 * w;
        if (reach >= 0) m |= reach >= 63 ? ~0ull : (2ull << reach) - 1;
      }
    }
    if (lead) {   // the nearest set bit after the word reaches into it from above
      int j = w >> 6;
      uint64_t nz = nonzero[j] & ~((2ull << (w & 63)) - 1);
      while (!nz && j < kMapWords - 1) nz = nonzero[++j];
      if (nz) {
        const int lw = 64 * j + __builtin_ctzll(nz);
        // the first bit it sets, counted from the word's first
        const int reach = 64 * lw + __builtin_ctzll(act[lw]) - lead - 64 * w;
        if (reach <= 63) m |= reach <= 0 ? ~0ull : ~0ull << reach;
      }
    }
    mark[w] = m & word_range((int64_t)w * 64, row_lo, row_hi);
  }
  __syncthreads();

  // 4. the slots
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int64_t base = first + (int64_t)u * kThreads * E;
    if (base >= nout) break;   // (the same for every thread)
    const int64_t i0 = base + (int64_t)tid * E;
    if (i0 >= nout) continue;
    const int64_t s0 = i0 >> sh;
    const uint64_t bits = window(mark, s0 - b0);
    const bool whole = i0 >= 0 && i0 + E <= nout;
    if constexpr (!CODES) {
      if (whole) {
        uint4 q;   // bit j of a nibble to bit 8 j of a word
        q.x = ((unsigned)(bits & 15) * 0x00204081u) & 0x01010101u;
        q.y = ((unsigned)((bits >> 4) & 15) * 0x00204081u) & 0x01010101u;
        q.z = ((unsigned)((bits >> 8) & 15) * 0x00204081u) & 0x01010101u;
        q.w = ((unsigned)((bits >> 12) & 15) * 0x00204081u) & 0x01010101u;
        *reinterpret_cast<uint4*>(y + i0) = q;
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (i0 + e >= 0 && i0 + e < nout) y[i0 + e] = (uint8_t)((bits >> e) & 1);
      }
    } else {
      const unsigned keep = ~(1u << bit) & 0xffffu;
      const int odd = (int)(i0 & sh);   // k = 2: code e of the slot holds sample s0 + ((e + odd) >> 1)
      if (whole) {
        uint4 q = *reinterpret_cast<const uint4*>(y + i0);
        unsigned* d = reinterpret_cast<unsigned*>(&q);
#pragma unroll
        for (int e = 0; e < E; e += 2) {
          const unsigned m0 = (unsigned)(bits >> ((e + odd) >> sh)) & 1;
          const unsigned m1 = (unsigned)(bits >> ((e + 1 + odd) >> sh)) & 1;
          d[e / 2] = (d[e / 2] & (keep | keep << 16)) | m0 << bit | m1 << (bit + 16);
        }
        *reinterpret_cast<uint4*>(y + i0) = q;
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (i0 + e >= 0 && i0 + e < nout)
            y[i0 + e] = (uint16_t)((y[i0 + e] & keep) | ((unsigned)(bits >> ((e + odd) >> sh)) & 1) << bit);
      }
    }
  }

  if constexpr (COUNT) {
    // the samples whose first output position lies in the span, as bits
    const int64_t c_lo = ((first + (1 << sh) - 1) >> sh) > 0 ? (first + (1 << sh) - 1) >> sh : 0;
    const int64_t c_hi = ((first + span + (1 << sh) - 1) >> sh) < n ? (first + span + (1 << sh) - 1) >> sh : n;
    unsigned high = 0, pulses = 0;
    for (int w = tid; w < words; w += kThreads) {
      const uint64_t own = word_range((int64_t)w * 64, c_lo - b0, c_hi - b0);
      const uint64_t m = mark[w], before = m << 1 | (w ? mark[w - 1] >> 63 : 0);
      high += (unsigned)__popcll(m & own);
      pulses += (unsigned)__popcll(m & ~before & own);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      high += __shfl_xor(high, d);
      pulses += __shfl_xor(pulses, d);
    }
    if ((tid & 63) == 0) {
      lds.wave_counts[tid >> 6][0] = high;
      lds.wave_counts[tid >> 6][1] = pulses;
    }
    __syncthreads();
    if (tid < 2) {
      unsigned sum = 0;
#pragma unroll
      for (int wv = 0; wv < kThreads / 64; ++wv) sum += lds.wave_counts[wv][tid];
      if (sum) atomicAdd(counts + (int64_t)row * 2 + tid, (unsigned long long)sum);
    }
  }
}

// in: [rows * k] rows of n samples; out: [rows] rows of n bytes that share no memory with them; counts (the _count
// kernels): [rows][2], zeroed before the launch.  Row strides in elements of their own side.
template <typename T>
__global__ void __launch_bounds__(kThreads)
    marker_rows(const T* __restrict__ in, int64_t in_stride, uint8_t* __restrict__ out, int64_t out_stride,
                const MarkRow* __restrict__ tab, int64_t n, uint32_t blocks_per_row, int k) {
  __shared__ MarkerLds lds;
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    marker_block<T, 2, false, false>(lds, in, in_stride, out, out_stride, tab, nullptr, n, row, blk, 0);
  else
    marker_block<T, 1, false, false>(lds, in, in_stride, out, out_stride, tab, nullptr, n, row, blk, 0);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    marker_rows_count(const T* __restrict__ in, int64_t in_stride, uint8_t* __restrict__ out, int64_t out_stride,
                      const MarkRow* __restrict__ tab, unsigned long long* __restrict__ counts, int64_t n,
                      uint32_t blocks_per_row, int k) {
  __shared__ MarkerLds lds;
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    marker_block<T, 2, false, true>(lds, in, in_stride, out, out_stride, tab, counts, n, row, blk, 0);
  else
    marker_block<T, 1, false, true>(lds, in, in_stride, out, out_stride, tab, counts, n, row, blk, 0);
}

// codes: [rows] rows of k n int16 codes, one bit of each replaced
template <typename T>
__global__ void __launch_bounds__(kThreads)
    marker_rows_codes(const T* __restrict__ in, int64_t in_stride, int16_t* codes, int64_t codes_stride,
                      const MarkRow* __restrict__ tab, int64_t n, uint32_t blocks_per_row, int k, int bit) {
  __shared__ MarkerLds lds;
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    marker_block<T, 2, true, false>(lds, in, in_stride, codes, codes_stride, tab, nullptr, n, row, blk, bit);
  else
    marker_block<T, 1, true, false>(lds, in, in_stride, codes, codes_stride, tab, nullptr, n, row, blk, bit);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    marker_rows_codes_count(const T* __restrict__ in, int64_t in_stride, int16_t* codes, int64_t codes_stride,
                            const MarkRow* __restrict__ tab, unsigned long long* __restrict__ counts, int64_t n,
                            uint32_t blocks_per_row, int k, int bit) {
  __shared__ MarkerLds lds;
  const auto [row, blk] = row_block(blocks_per_row);
  if (k == 2)
    marker_block<T, 2, true, true>(lds, in, in_stride, codes, codes_stride, tab, counts, n, row, blk, bit);
  else
    marker_block<T, 1, true, true>(lds, in, in_stride, codes, codes_stride, tab, counts, n, row, blk, bit);
}

}  // namespace

struct wfk_marker_rows_plan {
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  int k = 0;
  uint32_t blocks_per_row[2] = {0, 0};   // [bytes, into codes]
  size_t rows_off = 0;
  DevBuf<char> tables;   // MarkRow [batch / k]
};

namespace {

template <typename T>
void marker_launch(const wfk_marker_rows_plan* p, const void* in, int64_t in_stride, void* out, int64_t out_stride,
                   bool into_codes, int bit, int64_t* counts, hipStream_t s) {
  const uint32_t bpr = p->blocks_per_row[into_codes];
  const dim3 grid(bpr * (uint32_t)(p->batch / p->k));
  const MarkRow* tab = DevTables::at<const MarkRow>(p->tables.get(), p->rows_off);
  unsigned long long* c = (unsigned long long*)counts;
  if (into_codes) {
    if (counts)
      hipLaunchKernelGGL(marker_rows_codes_count<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride,
                         (int16_t*)out, out_stride, tab, c, p->n, bpr, p->k, bit);
    else
      hipLaunchKernelGGL(marker_rows_codes<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride, (int16_t*)out,
                         out_stride, tab, p->n, bpr, p->k, bit);
  } else {
    if (counts)
      hipLaunchKernelGGL(marker_rows_count<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride, (uint8_t*)out,
                         out_stride, tab, c, p->n, bpr, p->k);
    else
      hipLaunchKernelGGL(marker_rows<T>, grid, dim3(kThreads), 0, s, (const T*)in, in_stride, (uint8_t*)out,
                         out_stride, tab, p->n, bpr, p->k);
  }
}

// both applies: `out` is rows of out_n elements of out_es bytes
int marker_apply(wfk_marker_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev, int64_t out_stride,
                 bool into_codes, int bit, int64_t* counts_dev, hipStream_t s) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (bit < 0 || bit > 15) return wfk_fail(WFK_EINVAL, "marker rows: bit must lie in [0, 15]");
  const int64_t rows = p->batch / p->k;
  const RowReport report{counts_dev, rows, 2};
  // nothing to mark (the pointers of empty rows may be null); the report is still zeroed
  if (p->n == 0) return wfk_zero_report("marker rows", report, s);
  // a lone output row's stride is not read
  const RowSide out = into_codes ? RowSide{"codes", out_dev, rows, out_stride, p->k * p->n, sizeof(int16_t), false}
                                 : RowSide{"out", out_dev, rows, out_stride, p->n, sizeof(uint8_t), false};
  if (const int rc = wfk_row_rule("marker rows", {{"in", in_dev, p->batch, in_stride, p->n, wfk_elem_size(p->kind)}},
                                  out, kRowsAligned | kRowsDisjoint, wfk_fail, report))
    return rc;
  if (const int rc = wfk_zero_report("marker rows", report, s)) return rc;
  if (p->kind == WFK_OUT_F32)
    marker_launch<float>(p, in_dev, in_stride, out_dev, out_stride, into_codes, bit, counts_dev, s);
  else
    marker_launch<double>(p, in_dev, in_stride, out_dev, out_stride, into_codes, bit, counts_dev, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "marker rows kernel launch failed");
  return WFK_OK;
}

}  // namespace

extern "C" {

int wfk_marker_rows_plan_destroy(wfk_marker_rows_plan* p) {
  delete p;
  return WFK_OK;
}

int64_t wfk_marker_rows_span(const wfk_marker_rows_plan* p, int into_codes) {
  if (!p) return 0;
  return (int64_t)kSlots * kThreads * (into_codes ? kCodes / p->k : kMarkers);
}

const char* wfk_marker_rows_kernel_name(const wfk_marker_rows_plan* p, int into_codes, int with_counts) {
  if (!p) return "";
  const bool f32 = p->kind == WFK_OUT_F32;
  if (into_codes) {
    if (with_counts) return f32 ? "marker_rows_codes_count<float>" : "marker_rows_codes_count<double>";
    return f32 ? "marker_rows_codes<float>" : "marker_rows_codes<double>";
  }
  if (with_counts) return f32 ? "marker_rows_count<float>" : "marker_rows_count<double>";
  return f32 ? "marker_rows<float>" : "marker_rows<double>";
}

int wfk_marker_rows_plan_create(int64_t n, int32_t batch, int kind, int group, const double* threshold_host,
                                const int32_t* lead_host, const int32_t* trail_host,
                                wfk_marker_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (batch < 1 || !threshold_host || !lead_host || !trail_host)
    return wfk_fail(WFK_EINVAL, "bad marker rows plan arguments");
  if (n < 0) return wfk_fail(WFK_EINVAL, "marker rows plan: n must not be negative");
  if (const int rc = wfk_check_kind(kind)) return rc;
  if (group != 1 && group != 2) return wfk_fail(WFK_EINVAL, "marker rows plan: group must be 1 or 2");
  if (batch % group)
    return wfk_fail(WFK_EINVAL, "marker rows plan: " + std::to_string(batch) + " rows are no multiple of the group");
  const int32_t rows = batch / group;
  std::vector<MarkRow> tab_rows((size_t)rows);
  for (int32_t r = 0; r < rows; ++r) {
    const std::string who = "row " + std::to_string(r) + ": ";
    if (!std::isfinite(threshold_host[r])) return wfk_fail(WFK_EINVAL, who + "threshold is not finite");
    if (threshold_host[r] < 0.0) return wfk_fail(WFK_EINVAL, who + "threshold is negative");
    const int32_t edges[2] = {lead_host[r], trail_host[r]};
    for (int e = 0; e < 2; ++e) {
      if (edges[e] < 0) return wfk_fail(WFK_EINVAL, who + (e ? "trail" : "lead") + " is negative");
      if (edges[e] > WFK_MARKER_MAX_EDGE)
        return wfk_fail(WFK_EINVAL, who + (e ? "trail" : "lead") + " exceeds " + std::to_string(WFK_MARKER_MAX_EDGE));
    }
    tab_rows[r] = MarkRow{threshold_host[r], lead_host[r], trail_host[r]};
  }
  if (n > INT64_MAX / group) return wfk_fail(WFK_EINVAL, "marker rows plan: batch * n too large for one launch");
  uint32_t bpr[2] = {0, 0};
  if (const int rc = wfk_row_blocks("marker rows plan", n, (int64_t)kMarkers * kThreads * kSlots, kMarkers - 1, rows,
                                    &bpr[0]))
    return rc;
  if (const int rc = wfk_row_blocks("marker rows plan", group * n, (int64_t)kCodes * kThreads * kSlots, kCodes - 1,
                                    rows, &bpr[1]))
    return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_marker_rows_plan> p(new wfk_marker_rows_plan());
  p->n = n; p->batch = batch; p->kind = kind; p->k = group;
  p->blocks_per_row[0] = bpr[0]; p->blocks_per_row[1] = bpr[1];
  DevTables tab;
  p->rows_off = tab.add(tab_rows);
  if (const int rc = wfk_upload_tables("marker rows plan", tab, p->tables)) return rc;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the marker rows plan");
}

int wfk_marker_rows_apply(wfk_marker_rows_plan* p, const void* in_dev, int64_t in_stride, uint8_t* out_dev,
                          int64_t out_stride, int64_t* counts_dev, void* hip_stream) {
  return marker_apply(p, in_dev, in_stride, out_dev, out_stride, false, 0, counts_dev, (hipStream_t)hip_stream);
}

int wfk_marker_rows_apply_codes(wfk_marker_rows_plan* p, const void* in_dev, int64_t in_stride, int16_t* codes_dev,
                                int64_t codes_stride, int bit, int64_t* counts_dev, void* hip_stream) {
  return marker_apply(p, in_dev, in_stride, codes_dev, codes_stride, true, bit, counts_dev, (hipStream_t)hip_stream);
}

}  // extern "C"
