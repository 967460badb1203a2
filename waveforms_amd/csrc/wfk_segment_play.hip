// wfk_segment_play.hip -- play a segment table back into rows of int16 DAC codes: what a sequencer plays from a table
// (wfk_segment_rows' table, wfk_segment_library's plays, or one the user wrote) and a waveform memory (packed, library),
// with an optional comparison against the rows the table was cut from.  Per good row, sample i holds the k codes at
// k (offset_j + i - start_j) of packed where start_j <= i < start_j + length_j, and idle elsewhere; the report is
// [played, differ, stray, first].  It reads table, packed, used and expect and never writes them.
//
// A row is GOOD when 0 <= count <= max_segments, every entry j < count has length > 0, start >= 0, start + length <=
// n, offset >= 0, offset + length <= capacity (formed in 64 bits), and start_j >= start_(j-1) + length_(j-1): the
// entries are ascending and disjoint.  Any other row gets the report [-1, -1, -1, -1] and nothing else of it is written.
//
// Execution form.  Two launches on the stream (one in the checking pass and for n = 0).
// 1. segplay_check: one wave per row walks the count entries 64 at a time (the loads of four such rounds issued
//    together): the per-entry conditions and the neighbour condition (the end of the entry before through __shfl_up,
//    carried between rounds) by __ballot, played by a wave reduction.  It writes the row's verdict into the plan's workspace and the row's report, [played, 0, 0, -1] or all
//    -1: the launch that initialises the report, so there is no zeroing launch.
// 2. segplay_fill<K, OUT, EXPECT>: a workgroup owns the samples [b S, (b + 1) S) of its row, S = kSpan.  A bad row
//    returns at once.  A binary search on `start` finds the first entry that meets the block; the entries from there are
//    staged through LDS in tiles of kTile, a tile standing for the samples up to the start of the next tile's first
//    entry (the last tile: to the block's end), so a block that meets S one-sample plays loops over tiles.  A thread
//    owns chunks of 8 codes of the destination, counted from the row's first code; a chunk finds the first play that
//    ends after its first sample by a binary search in the tile.  A whole chunk inside one play, or in a gap, whose out
//    row is 16-byte aligned: one 16-byte store, the source being one aligned 16-byte load or two and a funnel shift by
//    the source's phase (2 k (offset - start) mod 16 plus the packed row's own: every value is legal); where the two
//    aligned loads would leave the packed row, element loads.  Every other chunk -- one that straddles a play's edge,
//    a tile's edge or the row's end, every chunk of an unaligned out row -- goes element by element.  The idle pattern
//    is by code index in the row, so an out row that starts at an odd code still has the I idle code on I positions.
//    With EXPECT a thread counts its samples in registers, the block reduces them and adds once to the report with
//    64-bit atomic adds, first by an atomic min (on the unsigned value: -1 is above every sample): all integers, so
//    nothing depends on the order of arrival.  With OUT = false nothing but the report is stored.
// No element outside [0, k capacity) of a packed row or [0, k n) of an expect row is read, and only rows whose every
// entry the check found inside those are followed.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

namespace {

constexpr int kSpan = 8192;                      // samples per block: wfk_segment_rows_span at align 1
constexpr int kTile = kThreads;                  // entries staged at a time: a thread loads one
constexpr int kWaves = kThreads / 64;
constexpr int kCheckRounds = 4;                // rounds of 64 entries whose loads the check issues together
constexpr int64_t kMaxSegments = 1ll << 30;      // as the library's
constexpr uint32_t kNone = 0xffffffffu;          // no sample counted: above every sample index

struct PlayGeom {
  int64_t n, max_segments, capacity;
  uint32_t blocks_per_row;
};

// one wave per row; bad: [rows], report: [rows][4]
__global__ void __launch_bounds__(64)
    segplay_check(const int32_t* __restrict__ table, int64_t table_stride, const int64_t* __restrict__ used,
                  int32_t* __restrict__ bad_of, int64_t* __restrict__ report, PlayGeom geo) {
  const uint32_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t count = used[(int64_t)row * 2];
  bool bad = count < 0 || count > geo.max_segments;
  const int32_t* t = table + (int64_t)row * table_stride;
  long long played = 0, end_c = 0;   // the end of the last entry of the rounds before
  for (int64_t base = 0; !bad && base < count; base += 64 * kCheckRounds) {
    // the loads of kCheckRounds rounds of 64 entries first, so that a long table does not wait for each in turn
    int32_t start[kCheckRounds], length[kCheckRounds], offset[kCheckRounds];
#pragma unroll
    for (int u = 0; u < kCheckRounds; ++u) {
      const int64_t j = base + u * 64 + lane;
      start[u] = length[u] = offset[u] = 0;
      if (j < count) {
        start[u] = t[j * 3];
        length[u] = t[j * 3 + 1];
        offset[u] = t[j * 3 + 2];
      }
    }
    bool wrong = false;
#pragma unroll
    for (int u = 0; u < kCheckRounds; ++u) {
      const bool valid = base + u * 64 + lane < count;
      const long long end = (long long)start[u] + length[u];   // (64 bits: the sums of two int32 do not wrap)
      long long before = __shfl_up(end, 1);
      if (lane == 0) before = end_c;
      wrong = wrong || (valid && (length[u] <= 0 || start[u] < 0 || end > geo.n || offset[u] < 0 ||
                                  (long long)offset[u] + length[u] > geo.capacity || start[u] < before));
      played += length[u];
      end_c = __shfl(end, 63);   // (of a round that is not full: read by no valid entry)
    }
    bad = __ballot(wrong) != 0;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) played += __shfl_xor(played, d);
  if (lane == 0) bad_of[row] = bad;
  if (lane < 4) report[(int64_t)row * 4 + lane] = bad ? -1 : lane == 0 ? played : lane == 3 ? -1 : 0;
}

// The 8 codes [e, e + 8) of the row x[0 .. ne), all of them in it, from wherever they start: one aligned 16-byte load,
// or the two aligned 16 bytes that hold them shifted down by the phase; element loads where those two would leave the
// row.
__device__ __forceinline__ uint4 load_codes8(const uint16_t* __restrict__ x, int64_t e, int64_t ne) {
  const uint16_t* src = x + e;
  const int phase = (int)((reinterpret_cast<uintptr_t>(src) >> 1) & 7);   // codes from the 16-byte boundary to src
  if (!phase) return *reinterpret_cast<const uint4*>(src);
  uint4 v;
  if (e >= phase && e - phase + 16 <= ne) {
    const uint4* a = reinterpret_cast<const uint4*>(src - phase);
    const uint4 lo = a[0], hi = a[1];
    const uint64_t w0 = lo.x | (uint64_t)lo.y << 32, w1 = lo.z | (uint64_t)lo.w << 32;
    const uint64_t w2 = hi.x | (uint64_t)hi.y << 32, w3 = hi.z | (uint64_t)hi.w << 32;
    const bool up = phase >= 4;                          // a whole 64-bit word, then 0 .. 3 codes
    const int rs = 16 * (phase & 3);
    const uint64_t f0 = up ? w1 : w0, f1 = up ? w2 : w1, f2 = up ? w3 : w2;
    const uint64_t o0 = rs ? f0 >> rs | f1 << (64 - rs) : f0, o1 = rs ? f1 >> rs | f2 << (64 - rs) : f1;
    v.x = (unsigned)o0; v.y = (unsigned)(o0 >> 32);
    v.z = (unsigned)o1; v.w = (unsigned)(o1 >> 32);
  } else {
    v.x = src[0] | (unsigned)src[1] << 16;
    v.y = src[2] | (unsigned)src[3] << 16;
    v.z = src[4] | (unsigned)src[5] << 16;
    v.w = src[6] | (unsigned)src[7] << 16;
  }
  return v;
}

// the samples of a chunk (first sample s0) in which a and b differ in any of their K codes
template <int K>
__device__ __forceinline__ void count_samples(const uint4& a, const uint4& b, int64_t s0, uint32_t& counter,
                                              uint32_t& first) {
  const unsigned x[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
#pragma unroll
  for (int s = 0; s < 8 / K; ++s) {
    const bool d = K == 2 ? x[s] != 0 : ((x[s / 2] >> (16 * (s & 1))) & 0xffffu) != 0;
    if (d) {
      ++counter;
      if ((uint32_t)(s0 + s) < first) first = (uint32_t)(s0 + s);
    }
  }
}

// out: [rows] rows of K n int16 (OUT), expect: the same (EXPECT), report: [rows][4], initialised by segplay_check
template <int K, bool OUT, bool EXPECT>
__global__ void __launch_bounds__(kThreads)
    segplay_fill(const int32_t* __restrict__ table, int64_t table_stride, const uint16_t* __restrict__ packed,
                 int64_t packed_stride, const int64_t* __restrict__ used, const int32_t* __restrict__ bad_of,
                 uint32_t idle, uint16_t* __restrict__ out, int64_t out_stride, const uint16_t* __restrict__ expect,
                 int64_t expect_stride, int64_t* __restrict__ report, PlayGeom geo) {
  __shared__ int32_t st[kTile], en[kTile], delta[kTile];   // start, end, offset - start of the staged entries
  __shared__ uint32_t red[3][kWaves];
  const auto [row, blk] = row_block(geo.blocks_per_row);
  if (bad_of[row]) return;
  const int tid = threadIdx.x;
  const int64_t n = geo.n, count = used[(int64_t)row * 2];
  const int64_t s_lo = (int64_t)blk * kSpan, s_hi = s_lo + kSpan < n ? s_lo + kSpan : n;
  const int32_t* __restrict__ t = table + (int64_t)row * table_stride;
  const uint16_t* __restrict__ y = packed + (int64_t)row * packed_stride;
  uint16_t* __restrict__ o = OUT ? out + (int64_t)row * out_stride : nullptr;
  const uint16_t* __restrict__ ex = EXPECT ? expect + (int64_t)row * expect_stride : nullptr;
  const int64_t y_codes = geo.capacity * K, row_codes = n * K;
  const bool vdst = !OUT || !(reinterpret_cast<uintptr_t>(o) & 15);
  const uint16_t idle_i = (uint16_t)(idle & 0xffffu), idle_q = K == 2 ? (uint16_t)(idle >> 16) : idle_i;
  const unsigned idle2 = idle_i | (unsigned)idle_q << 16;   // code index 8 c is even: I comes first
  const uint4 idle8 = make_uint4(idle2, idle2, idle2, idle2);
  constexpr int cps = 8 / K;   // samples per chunk

  // the first entry that meets the block: the one before the first with start > s_lo where it ends after s_lo
  int64_t j_base;
  {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (t[mid * 3] > s_lo) hi = mid;
      else lo = mid + 1;
    }
    j_base = lo > 0 && (int64_t)t[(lo - 1) * 3] + t[(lo - 1) * 3 + 1] > s_lo ? lo - 1 : lo;
  }

  uint32_t differ = 0, stray = 0, first = kNone;
  for (int64_t lo_t = s_lo;; j_base += kTile) {
    const int m = (int)(count - j_base < kTile ? count - j_base : kTile);   // >= 0
    if (tid < m) {
      const int64_t j = j_base + tid;
      const int32_t start = t[j * 3];
      st[tid] = start;
      en[tid] = start + t[j * 3 + 1];
      delta[tid] = t[j * 3 + 2] - start;
    }
    // the tile stands for [lo_t, hi_t): up to the start of the next tile's first entry, or the block's end
    const int64_t next = j_base + kTile < count ? (int64_t)t[(j_base + kTile) * 3] : s_hi;
    const bool last = next >= s_hi;
    const int64_t hi_t = last ? s_hi : next;
    __syncthreads();
    for (int64_t c = lo_t / cps + tid; c * cps < hi_t; c += kThreads) {
      const int64_t sa = c * cps, sb = sa + cps;
      const int64_t a = sa > lo_t ? sa : lo_t, b = sb < hi_t ? sb : hi_t;
      int idx = 0;   // the first staged entry that ends after a
      for (int len = m; len > 0;) {
        const int half = len >> 1;
        if (en[idx + half] <= a) {
          idx += half + 1;
          len -= half + 1;
        } else {
          len = half;
        }
      }
      const bool inside = idx < m && st[idx] <= a && en[idx] >= b, gap = idx == m || st[idx] >= b;
      if (vdst && a == sa && b == sb && (inside || gap)) {
        const uint4 v = inside ? load_codes8(y, ((int64_t)delta[idx] + sa) * K, y_codes) : idle8;
        if constexpr (OUT) *reinterpret_cast<uint4*>(o + c * 8) = v;
        if constexpr (EXPECT) {
          uint32_t counted = 0;
          count_samples<K>(v, load_codes8(ex, c * 8, row_codes), sa, counted, first);
          differ += inside ? counted : 0;
          stray += inside ? 0 : counted;
        }
      } else {
        for (int64_t i = a; i < b; ++i) {
          while (idx < m && en[idx] <= i) ++idx;
          const bool in = idx < m && st[idx] <= i;
          bool d = false;
#pragma unroll
          for (int q = 0; q < K; ++q) {
            const uint16_t code = in ? y[((int64_t)delta[idx] + i) * K + q] : q ? idle_q : idle_i;
            if constexpr (OUT) o[i * K + q] = code;
            if constexpr (EXPECT) d = d || ex[i * K + q] != code;
          }
          if (d) {
            differ += in;
            stray += !in;
            if ((uint32_t)i < first) first = (uint32_t)i;
          }
        }
      }
    }
    if (last) break;
    lo_t = hi_t;
    __syncthreads();   // the tile is read no more
  }

  if constexpr (EXPECT) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      differ += __shfl_xor(differ, d);
      stray += __shfl_xor(stray, d);
      const uint32_t f = __shfl_xor(first, d);
      first = f < first ? f : first;
    }
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = differ;
      red[1][tid >> 6] = stray;
      red[2][tid >> 6] = first;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t dsum = 0, ssum = 0, f = kNone;
      for (int w = 0; w < kWaves; ++w) {
        dsum += red[0][w];
        ssum += red[1][w];
        f = red[2][w] < f ? red[2][w] : f;
      }
      unsigned long long* r = reinterpret_cast<unsigned long long*>(report + (int64_t)row * 4);
      if (dsum) atomicAdd(r + 1, (unsigned long long)dsum);
      if (ssum) atomicAdd(r + 2, (unsigned long long)ssum);
      if (f != kNone) atomicMin(r + 3, (unsigned long long)f);
    }
  }
}

}  // namespace

struct wfk_segment_play_plan {
  int64_t n = 0, max_segments = 0, capacity = 0;
  int32_t rows = 0;
  int k = 0;
  uint32_t blocks_per_row = 0;
  DevBuf<int32_t> bad;   // [rows]  the row's verdict, by the check
};

namespace {

template <int K, bool OUT, bool EXPECT>
void play_launch(const wfk_segment_play_plan* p, const PlayGeom& geo, const int32_t* table, int64_t table_stride,
                 const int16_t* packed, int64_t packed_stride, const int64_t* used, uint32_t idle, int16_t* out,
                 int64_t out_stride, const int16_t* expect, int64_t expect_stride, int64_t* report, hipStream_t s) {
  hipLaunchKernelGGL((segplay_fill<K, OUT, EXPECT>), dim3(p->blocks_per_row * (uint32_t)p->rows), dim3(kThreads), 0, s,
                     table, table_stride, (const uint16_t*)packed, packed_stride, used, (const int32_t*)p->bad.get(),
                     idle, (uint16_t*)out, out_stride, (const uint16_t*)expect, expect_stride, report, geo);
}

template <int K>
void play_launch_k(const wfk_segment_play_plan* p, const PlayGeom& geo, const int32_t* table, int64_t table_stride,
                   const int16_t* packed, int64_t packed_stride, const int64_t* used, uint32_t idle, int16_t* out,
                   int64_t out_stride, const int16_t* expect, int64_t expect_stride, int64_t* report, hipStream_t s) {
  if (out && expect)
    play_launch<K, true, true>(p, geo, table, table_stride, packed, packed_stride, used, idle, out, out_stride, expect,
                               expect_stride, report, s);
  else if (out)
    play_launch<K, true, false>(p, geo, table, table_stride, packed, packed_stride, used, idle, out, out_stride,
                                nullptr, 0, report, s);
  else
    play_launch<K, false, true>(p, geo, table, table_stride, packed, packed_stride, used, idle, nullptr, 0, expect,
                                expect_stride, report, s);
}

}  // namespace

extern "C" {

int wfk_segment_play_plan_destroy(wfk_segment_play_plan* p) {
  delete p;
  return WFK_OK;
}

int64_t wfk_segment_play_span(const wfk_segment_play_plan* p) { return p ? kSpan : 0; }

const char* wfk_segment_play_kernel_name(const wfk_segment_play_plan* p, int launch) {
  if (!p) return "";
  const bool two = p->k == 2;
  switch (launch) {
    case 0: return "segplay_check";
    case 1: return two ? "segplay_fill<2, true, false>" : "segplay_fill<1, true, false>";
    case 2: return two ? "segplay_fill<2, false, true>" : "segplay_fill<1, false, true>";
    case 3: return two ? "segplay_fill<2, true, true>" : "segplay_fill<1, true, true>";
    default: return "";
  }
}

int wfk_segment_play_plan_create(int64_t n, int32_t rows, int width, int64_t max_segments, int64_t capacity,
                                 wfk_segment_play_plan** out) try {
  const std::string who = "segment play plan: ";
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 0 || n > 0x7fffffffLL) return wfk_fail(WFK_EINVAL, who + "n must lie in [0, 2^31 - 1]");
  if (rows < 1) return wfk_fail(WFK_EINVAL, who + "rows must be at least 1");
  if (width != 1 && width != 2) return wfk_fail(WFK_EINVAL, who + "width must be 1 or 2");
  if (max_segments < 0) return wfk_fail(WFK_EINVAL, who + "max_segments must not be negative");
  if (max_segments > kMaxSegments) return wfk_fail(WFK_EINVAL, who + "max_segments must not exceed 2^30");
  if (capacity < 0 || capacity > 0x7fffffffLL) return wfk_fail(WFK_EINVAL, who + "capacity must lie in [0, 2^31 - 1]");
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("segment play plan", n, kSpan, 0, rows, &bpr)) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_segment_play_plan> p(new wfk_segment_play_plan());
  p->n = n; p->rows = rows; p->k = width; p->max_segments = max_segments; p->capacity = capacity;
  p->blocks_per_row = bpr;
  if (!p->bad.alloc((size_t)rows * sizeof(int32_t))) {
    (void)hipGetLastError();
    return wfk_fail(WFK_EHIP, who + "workspace allocation failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the segment play plan");
}

int wfk_segment_play_apply(wfk_segment_play_plan* p, const int32_t* table, int64_t table_stride, const int16_t* packed,
                           int64_t packed_stride, const int64_t* used, int16_t idle0, int16_t idle1, int16_t* out,
                           int64_t out_stride, const int16_t* expect, int64_t expect_stride, int64_t* report,
                           void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (!report) return wfk_fail(WFK_EINVAL, "segment play: report is null");
  if (!used) return wfk_fail(WFK_EINVAL, "segment play: used is null");
  if (const int rc = wfk_segment_play_row_rule(SegmentPlayShape{p->rows, p->n, p->k, p->max_segments, p->capacity},
                                               table, table_stride, packed, packed_stride, used, out, out_stride,
                                               expect, expect_stride, report, wfk_fail))
    return rc;
  // a side that holds nothing is not written or read: the kernels are not given it
  if (!p->n) {
    out = nullptr;
    expect = nullptr;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  const PlayGeom geo{p->n, p->max_segments, p->capacity, p->blocks_per_row};
  const uint32_t idle = (uint16_t)idle0 | (uint32_t)(uint16_t)idle1 << 16;
  hipLaunchKernelGGL(segplay_check, dim3((uint32_t)p->rows), dim3(64), 0, s, table, table_stride, used, p->bad.get(),
                     report, geo);
  if (p->blocks_per_row && (out || expect)) {
    if (p->k == 2)
      play_launch_k<2>(p, geo, table, table_stride, packed, packed_stride, used, idle, out, out_stride, expect,
                       expect_stride, report, s);
    else
      play_launch_k<1>(p, geo, table, table_stride, packed, packed_stride, used, idle, out, out_stride, expect,
                       expect_stride, report, s);
  }
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "segment play kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
