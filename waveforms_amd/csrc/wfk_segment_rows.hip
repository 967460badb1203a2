// wfk_segment_rows.hip -- cut rows of int16 DAC codes at their marker: per row a segment table (play this stretch of
// the row, from here), the kept codes packed back to back, and the two totals, so that only the stretches around the
// pulses cross to the host.  width = k in {1, 2} codes per sample (k = 2: the interleaved I/Q of wfk_dac_rows), the
// marker either one bit of the codes (any of the k codes of a sample) or a row of bytes (wfk_marker_rows_apply).
// align = A, a power of two: the row is cut in granules of A samples, granule q is kept when any of its samples is
// marked, and a segment is a maximal run of kept granules [q0, q1):
//   start = q0 A,   length = min(q1 A, n) - start,   offset = the lengths before it,   kept = all lengths.
//
// Execution form.  Three launches on the stream; a workgroup owns the samples [b S, (b + 1) S) of its row, S =
// max(8192, 64 A), so a block's granules fill whole 64-bit words.
// 1. segment_count: the block's bitmap in LDS, one bit per sample.  A row that is aligned (16 bytes of codes, 8 of
//    marks): a byte per run of 8 samples, from one 16-byte load per 8 codes or one 8-byte load of marks.  Any other row:
//    the aligned chunks from the one that holds the block's first element on, each chunk's bits OR-ed into the zeroed
//    bitmap at the samples of its elements.  Element loads in the run or chunk that crosses an end of the row.  Folded
//    to one bit per granule.  One partial per (row, block) in the plan's workspace:
//    [kept samples, rising edges of the granule bits counted as if nothing came before the block, first | last << 1
//    granule bit, the last of those edges as a sample or -1].
// 2. segment_scan: one wave per row walks the row's partials, 64 at a time, and turns them IN PLACE into
//    [kept before, segments started before, the start of the segment open at the block's first sample or -1, kept in
//    the block]; an edge at a block's first granule is no start where the block before ended kept.  It writes
//    used[row] = [count, kept].
// 3. segment_pack: the bitmap and granule bits again (a block that keeps nothing and has no segment open returns at
//    once), ranks of the kept granules by popcount over the granule words plus the block's prefix, the kept codes
//    copied 16 bytes at a time where A k >= 8 and the packed row is aligned (the load: one aligned 16 bytes, or two
//    and a funnel shift where the code row is not aligned; element by element otherwise, at the capacity cut and at the
//    row's end); table entries: the block in which a segment starts writes start and offset,
//    the block in which it ends (a falling edge of the granule bits, or the row's end) writes length from the last
//    start before it, carried across blocks by the scan.
// No atomics on global memory, no zeroing launch: the result is a pure function of the inputs.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

namespace {

constexpr int kMinSpan = 8192;                 // samples per block where 64 A is not more
constexpr int kRun = 8;                        // samples per run: one byte of the bitmap
constexpr int kGWords = kMinSpan / 64;         // the most granule words a block has (A = 1)
constexpr int kPartial = 4;                    // int64 per (row, block) in the workspace
static_assert(kGWords <= kThreads, "a thread per granule word");

// a block's LDS next to the bitmap: the granule bits; for the pack: kept granules / starts before each word, and the
// last start at or before each word's end (a sample, carried from the blocks before; -1: none)
struct SegLds {
  uint64_t g[kGWords];
  int64_t lstart[kGWords];
  uint32_t grank[kGWords], srank[kGWords];
  int acc[3];
};

// what a launch is given besides the rows
struct SegGeom {
  int64_t n, span;          // samples per row, per block
  uint32_t blocks_per_row;
  int ash, bit;             // A = 1 << ash
};

// The block's granule bits into lds.g: granule q of the block is bit q.  bm: span / 64 words of LDS.
template <int K, bool MARKS>
__device__ __forceinline__ void granule_bits(uint64_t* bm, SegLds& lds, const uint16_t* __restrict__ codes,
                                             const uint8_t* __restrict__ marks, const SegGeom& geo, int64_t s_lo) {
  const int tid = threadIdx.x;
  const int64_t n = geo.n;
  const int runs = (int)(geo.span / kRun);
  unsigned char* bytes = reinterpret_cast<unsigned char*>(bm);
  const bool vec = MARKS ? !(reinterpret_cast<uintptr_t>(marks) & 7) : !(reinterpret_cast<uintptr_t>(codes) & 15);
  if (!vec) {
    // The row is not aligned: the aligned chunks of 8 elements (16 bytes of codes, 8 of marks) from the one that holds
    // the block's first element on; a chunk's bits go to the samples of its elements -- element e of the row belongs to
    // sample e / KE -- by an OR into the zeroed bitmap, so a pair that straddles two chunks needs nothing special.
    constexpr int KE = MARKS ? 1 : K;   // elements per sample
    constexpr int sh = KE - 1;
    uint32_t* bw = reinterpret_cast<uint32_t*>(bm);
    for (int i = tid; i < (int)(geo.span / 32); i += kThreads) bw[i] = 0;
    __syncthreads();
    const int64_t ne = n * KE, span = geo.span;
    const int lead = MARKS ? (int)(reinterpret_cast<uintptr_t>(marks) & 7)
                           : (int)((reinterpret_cast<uintptr_t>(codes) >> 1) & 7);
    const int chunks = (int)(span * KE / 8) + 1;
    for (int r = tid; r < chunks; r += kThreads) {
      const int64_t e0 = s_lo * KE + (int64_t)r * 8 - lead;   // the chunk's first element, in the row (>= -7)
      if (e0 >= ne) break;
      unsigned m8 = 0;                                        // bit e: element e0 + e is marked
      if (e0 >= 0 && e0 + 8 <= ne) {
        if constexpr (MARKS) {
          const uint2 v = *reinterpret_cast<const uint2*>(marks + e0);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            m8 |= (unsigned)(((v.x >> (8 * e)) & 0xffu) != 0) << e | (unsigned)(((v.y >> (8 * e)) & 0xffu) != 0) << (4 + e);
        } else {
          const uint4 v = *reinterpret_cast<const uint4*>(codes + e0);
          const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) m8 |= ((d[e / 2] >> (16 * (e & 1) + geo.bit)) & 1u) << e;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e0 + e >= 0 && e0 + e < ne) {
            if constexpr (MARKS) m8 |= (unsigned)(marks[e0 + e] != 0) << e;
            else m8 |= (((unsigned)codes[e0 + e] >> geo.bit) & 1u) << e;
          }
      }
      if (!m8) continue;
      const int64_t p0 = e0 >> sh;                            // the sample of the chunk's first element (floor)
      unsigned mask = 0;                                      // bit j: sample p0 + j
#pragma unroll
      for (int e = 0; e < 8; ++e) mask |= ((m8 >> e) & 1u) << (int)(((e0 + e) >> sh) - p0);
      int64_t pos = p0 - s_lo;                                // the bitmap bit of sample p0 (>= -7)
      if (pos < 0) {
        mask >>= (int)-pos;
        pos = 0;
      }
      if (pos >= span) continue;
      if (span - pos < 16) mask &= (1u << (int)(span - pos)) - 1;
      const uint64_t v = (uint64_t)mask << (pos & 31);
      if ((uint32_t)v) atomicOr(&bw[pos >> 5], (uint32_t)v);
      if (v >> 32) atomicOr(&bw[(pos >> 5) + 1], (uint32_t)(v >> 32));
    }
  }
  for (int r = vec ? tid : runs; r < runs; r += kThreads) {
    const int64_t j0 = s_lo + (int64_t)r * kRun;
    unsigned m = 0;
    if (j0 < n) {
      if constexpr (MARKS) {
        const uint8_t* p = marks + j0;
        if (vec && j0 + kRun <= n) {
          const uint2 v = *reinterpret_cast<const uint2*>(p);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            m |= (unsigned)(((v.x >> (8 * e)) & 0xffu) != 0) << e | (unsigned)(((v.y >> (8 * e)) & 0xffu) != 0) << (4 + e);
        } else {
#pragma unroll
          for (int e = 0; e < kRun; ++e)
            if (j0 + e < n) m |= (unsigned)(p[e] != 0) << e;
        }
      } else {
        const uint16_t* p = codes + j0 * K;
        if (vec && j0 + kRun <= n) {
#pragma unroll
          for (int q = 0; q < K; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[q];
            const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e)   // code 8 q + e of the run belongs to sample (8 q + e) / K
              m |= ((d[e / 2] >> (16 * (e & 1) + geo.bit)) & 1u) << ((8 * q + e) / K);
          }
        } else {
#pragma unroll
          for (int e = 0; e < kRun; ++e)
            if (j0 + e < n) {
#pragma unroll
              for (int j = 0; j < K; ++j) m |= (((unsigned)p[e * K + j] >> geo.bit) & 1u) << e;
            }
        }
      }
    }
    bytes[r] = (unsigned char)m;
  }
  __syncthreads();
  const int ash = geo.ash;
  const int gran = (int)(geo.span >> ash);   // granules per block: a multiple of 64, at most 64 kGWords
  if (ash < 6) {                             // a thread per granule word
    if (tid < gran / 64) {
      uint64_t g = 0;
      if (ash == 0) {
        g = bm[tid];
      } else {
        const uint64_t mask = (1ull << (1 << ash)) - 1;
        for (int b = 0; b < 64; ++b) {
          const int s = (tid * 64 + b) << ash;   // < span <= 8192 here
          g |= (uint64_t)(((bm[s >> 6] >> (s & 63)) & mask) != 0) << b;
        }
      }
      lds.g[tid] = g;
    }
  } else {                                   // a thread per granule (at most 128 of them), a ballot per word
    const int wpg = 1 << (ash - 6);
    bool on = false;
    if (tid < gran)
      for (int i = 0; i < wpg; ++i) on = on || bm[tid * wpg + i] != 0;
    const uint64_t b = __ballot(on);
    if ((tid & 63) == 0 && tid < gran) lds.g[tid >> 6] = b;
  }
  __syncthreads();
}

// codes: [rows] rows of K n int16; marks (MARKS): [rows] rows of n bytes; ws: [rows][blocks_per_row][kPartial]
template <int K, bool MARKS>
__global__ void __launch_bounds__(kThreads)
    segment_count(const uint16_t* __restrict__ codes, int64_t codes_stride, const uint8_t* __restrict__ marks,
                  int64_t marks_stride, int64_t* __restrict__ ws, SegGeom geo) {
  extern __shared__ uint64_t bm[];
  __shared__ SegLds lds;
  const auto [row, blk] = row_block(geo.blocks_per_row);
  const int tid = threadIdx.x;
  const int64_t s_lo = (int64_t)blk * geo.span;
  if (tid < 3) lds.acc[tid] = tid == 2 ? -1 : 0;
  granule_bits<K, MARKS>(bm, lds, codes + (int64_t)row * codes_stride,
                         MARKS ? marks + (int64_t)row * marks_stride : nullptr, geo, s_lo);
  const int gwords = (int)(geo.span >> geo.ash) / 64;
  if (tid < gwords) {
    const uint64_t g = lds.g[tid];
    const uint64_t rise = g & ~(g << 1 | (tid ? lds.g[tid - 1] >> 63 : 0));
    if (g) atomicAdd(&lds.acc[0], __popcll(g));
    if (rise) {
      atomicAdd(&lds.acc[1], __popcll(rise));
      atomicMax(&lds.acc[2], tid * 64 + 63 - __builtin_clzll(rise));
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int64_t q_first = s_lo >> geo.ash, q_last = ((geo.n - 1) >> geo.ash) - q_first;   // the row's last granule
    int64_t kept = (int64_t)lds.acc[0] << geo.ash;
    if (q_last < (int64_t)gwords * 64 && ((lds.g[q_last >> 6] >> (q_last & 63)) & 1))
      kept -= ((q_first + q_last + 1) << geo.ash) - geo.n;                                  // it may be partial
    int64_t* w = ws + ((int64_t)row * geo.blocks_per_row + blk) * kPartial;
    w[0] = kept;
    w[1] = lds.acc[1];
    w[2] = (int64_t)(lds.g[0] & 1) | (int64_t)(lds.g[gwords - 1] >> 63) << 1;
    w[3] = lds.acc[2] < 0 ? -1 : (q_first + lds.acc[2]) << geo.ash;
  }
}

// one wave per row; used: [rows][2]
__global__ void __launch_bounds__(64)
    segment_scan(int64_t* __restrict__ ws, int64_t* __restrict__ used, uint32_t blocks_per_row) {
  const int lane = threadIdx.x;
  int64_t* w = ws + (int64_t)blockIdx.x * blocks_per_row * kPartial;
  long long kept_c = 0, starts_c = 0, last_c = -1;   // over the blocks before this round of 64
  int last_flag_c = 0;
  for (uint32_t base = 0; base < blocks_per_row; base += 64) {
    const uint32_t b = base + lane;
    const bool valid = b < blocks_per_row;
    long long kept = 0, st = 0, fl = 0, ls = -1;
    if (valid) {
      kept = w[(int64_t)b * kPartial];
      st = w[(int64_t)b * kPartial + 1];
      fl = w[(int64_t)b * kPartial + 2];
      ls = w[(int64_t)b * kPartial + 3];
    }
    const int last_bit = (int)(fl >> 1) & 1;
    int prev_last = __shfl_up(last_bit, 1);
    if (lane == 0) prev_last = last_flag_c;
    const long long joined = (fl & 1) & prev_last;   // the block's first granule continues a segment
    const long long own_st = st - joined;
    long long kept_i = kept, st_i = own_st, ls_i = own_st > 0 ? ls : -1;   // inclusive over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long a = __shfl_up(kept_i, d), s = __shfl_up(st_i, d), l = __shfl_up(ls_i, d);
      if (lane >= d) {
        kept_i += a;
        st_i += s;
        ls_i = l > ls_i ? l : ls_i;
      }
    }
    long long ls_before = __shfl_up(ls_i, 1);
    if (lane == 0) ls_before = -1;
    if (last_c > ls_before) ls_before = last_c;
    if (valid) {
      w[(int64_t)b * kPartial] = kept_c + kept_i - kept;
      w[(int64_t)b * kPartial + 1] = starts_c + st_i - own_st;
      w[(int64_t)b * kPartial + 2] = prev_last ? ls_before : -1;
      w[(int64_t)b * kPartial + 3] = kept;
    }
    kept_c += __shfl(kept_i, 63);
    starts_c += __shfl(st_i, 63);
    const long long l63 = __shfl(ls_i, 63);
    last_c = l63 > last_c ? l63 : last_c;
    last_flag_c = __shfl(last_bit, 63);
  }
  if (lane == 0) {
    used[(int64_t)blockIdx.x * 2] = starts_c;
    used[(int64_t)blockIdx.x * 2 + 1] = kept_c;
  }
}

// table: [rows] rows of 3 max_segments int32, packed: [rows] rows of K capacity int16 (either may hold nothing)
template <int K, bool MARKS>
__global__ void __launch_bounds__(kThreads)
    segment_pack(const uint16_t* __restrict__ codes, int64_t codes_stride, const uint8_t* __restrict__ marks,
                 int64_t marks_stride, const int64_t* __restrict__ ws, int32_t* __restrict__ table,
                 int64_t table_stride, int64_t max_segments, uint16_t* __restrict__ packed, int64_t packed_stride,
                 int64_t capacity, SegGeom geo) {
  extern __shared__ uint64_t bm[];
  __shared__ SegLds lds;
  const auto [row, blk] = row_block(geo.blocks_per_row);
  const int tid = threadIdx.x;
  const int64_t* w = ws + ((int64_t)row * geo.blocks_per_row + blk) * kPartial;
  const int64_t kept_before = w[0], starts_before = w[1], open_start = w[2];
  if (w[3] == 0 && open_start < 0) return;   // nothing kept, nothing to close (the same for every thread)
  const int64_t n = geo.n, s_lo = (int64_t)blk * geo.span;
  const int ash = geo.ash;
  const uint16_t* __restrict__ x = codes + (int64_t)row * codes_stride;
  granule_bits<K, MARKS>(bm, lds, x, MARKS ? marks + (int64_t)row * marks_stride : nullptr, geo, s_lo);
  const int gwords = (int)(geo.span >> ash) / 64;
  const uint64_t open = open_start >= 0;
  if (tid == 0) {   // the prefixes over the granule words
    uint32_t gr = 0, sr = 0;
    int64_t last = open_start;
    uint64_t prev = open;
    for (int i = 0; i < gwords; ++i) {
      const uint64_t g = lds.g[i], rise = g & ~(g << 1 | prev);
      lds.grank[i] = gr;
      lds.srank[i] = sr;
      gr += __popcll(g);
      sr += __popcll(rise);
      if (rise) last = s_lo + ((int64_t)(i * 64 + 63 - __builtin_clzll(rise)) << ash);
      lds.lstart[i] = last;
      prev = g >> 63;
    }
  }
  __syncthreads();

  // the kept codes, in chunks of 8 codes of the row
  if (capacity > 0) {
    constexpr int cps = 8 / K;   // samples per chunk
    uint16_t* __restrict__ y = packed + (int64_t)row * packed_stride;
    const int chunks = (int)(geo.span / cps);
    const bool vsrc = !(reinterpret_cast<uintptr_t>(x) & 15);
    const int src_lead = (int)((reinterpret_cast<uintptr_t>(x) >> 1) & 7);   // codes from the 16-byte boundary to the row
    const bool vdst = !(reinterpret_cast<uintptr_t>(y) & 15) && (K << ash) >= 8;
    for (int c = tid; c < chunks; c += kThreads) {
      const int64_t ls = (int64_t)c * cps;   // the chunk's first sample, in the block
      const int64_t s0 = s_lo + ls;
      if (s0 >= n) break;
      if ((K << ash) >= 8) {   // the chunk lies in one granule
        const int q = (int)(ls >> ash);
        const uint64_t gw = lds.g[q >> 6];
        if (!((gw >> (q & 63)) & 1)) continue;
        const int64_t rank = lds.grank[q >> 6] + __popcll(gw & ((1ull << (q & 63)) - 1));
        const int64_t p0 = kept_before + (rank << ash) + (ls - ((int64_t)q << ash));
        if (p0 >= capacity) continue;
        const uint16_t* src = x + s0 * K;
        uint16_t* dst = y + p0 * K;
        if (vdst && s0 + cps <= n && p0 + cps <= capacity) {
          uint4 v;
          if (vsrc) {
            v = *reinterpret_cast<const uint4*>(src);
          } else if (s0 * K >= src_lead && s0 * K - src_lead + 16 <= n * K) {
            // the two aligned chunks that hold the 8 codes lie in the row: 32 bytes, shifted down by 2 src_lead
            const uint4* a = reinterpret_cast<const uint4*>(src - src_lead);
            const uint4 lo = a[0], hi = a[1];
            const uint64_t w0 = lo.x | (uint64_t)lo.y << 32, w1 = lo.z | (uint64_t)lo.w << 32;
            const uint64_t w2 = hi.x | (uint64_t)hi.y << 32, w3 = hi.z | (uint64_t)hi.w << 32;
            const bool up = src_lead >= 4;                     // a whole 64-bit word, then 0 .. 3 codes
            const int rs = 16 * (src_lead & 3);
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
          *reinterpret_cast<uint4*>(dst) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (s0 + e / K < n && p0 + e / K < capacity) dst[e] = src[e];
        }
      } else {                 // granules shorter than the chunk: sample by sample
#pragma unroll
        for (int e = 0; e < cps; ++e) {
          const int64_t ss = ls + e;
          if (s_lo + ss >= n) break;
          const int q = (int)(ss >> ash);
          const uint64_t gw = lds.g[q >> 6];
          if (!((gw >> (q & 63)) & 1)) continue;
          const int64_t rank = lds.grank[q >> 6] + __popcll(gw & ((1ull << (q & 63)) - 1));
          const int64_t p = kept_before + (rank << ash) + (ss - ((int64_t)q << ash));
          if (p >= capacity) continue;
#pragma unroll
          for (int j = 0; j < K; ++j) y[p * K + j] = x[(s_lo + ss) * K + j];
        }
      }
    }
  }

  // the table: a thread per granule word
  if (max_segments > 0 && tid < gwords) {
    int32_t* __restrict__ t = table + (int64_t)row * table_stride;
    const uint64_t g = lds.g[tid], before = g << 1 | (tid ? lds.g[tid - 1] >> 63 : open);
    const uint64_t rise = g & ~before;
    uint64_t fall = ~g & before;
    const int64_t w_lo = s_lo + ((int64_t)tid * 64 << ash);   // the word's first sample
    int idx = 0;
    for (uint64_t r = rise; r; r &= r - 1, ++idx) {
      const int b = __builtin_ctzll(r);
      const int64_t j = starts_before + lds.srank[tid] + idx;
      if (j < max_segments) {
        t[j * 3] = (int32_t)(w_lo + ((int64_t)b << ash));
        t[j * 3 + 2] = (int32_t)(kept_before + ((int64_t)(lds.grank[tid] + __popcll(g & ((1ull << b) - 1))) << ash));
      }
    }
    for (; fall; fall &= fall - 1) {
      const int b = __builtin_ctzll(fall);
      const uint64_t below = rise & ((1ull << b) - 1);
      const int64_t j = starts_before + lds.srank[tid] + __popcll(below) - 1;
      const int64_t start = below ? w_lo + ((int64_t)(63 - __builtin_clzll(below)) << ash)
                                  : (tid ? lds.lstart[tid - 1] : open_start);
      const int64_t end = w_lo + ((int64_t)b << ash) < n ? w_lo + ((int64_t)b << ash) : n;
      if (j >= 0 && j < max_segments) t[j * 3 + 1] = (int32_t)(end - start);
    }
    // the row ends kept in the block's last granule: no falling edge follows in this block
    if (tid == gwords - 1 && (g >> 63) && s_lo + geo.span >= n) {
      const int64_t j = starts_before + lds.srank[tid] + __popcll(rise) - 1;
      if (j >= 0 && j < max_segments) t[j * 3 + 1] = (int32_t)(n - lds.lstart[tid]);
    }
  }
}

}  // namespace

struct wfk_segment_rows_plan {
  int64_t n = 0, span = 0, max_segments = 0, capacity = 0;
  int32_t rows = 0;
  int k = 0, ash = 0;
  uint32_t blocks_per_row = 0;
  DevBuf<int64_t> workspace;   // [rows][blocks_per_row][kPartial]
};

namespace {

int64_t segment_span(int64_t align) { return 64 * align > kMinSpan ? 64 * align : kMinSpan; }

template <int K, bool MARKS>
void segment_launch(const wfk_segment_rows_plan* p, const SegGeom& geo, const int16_t* codes, int64_t codes_stride,
                    const uint8_t* marks, int64_t marks_stride, int32_t* table, int64_t table_stride, int16_t* packed,
                    int64_t packed_stride, int64_t* used, bool pack, hipStream_t s) {
  const dim3 grid(p->blocks_per_row * (uint32_t)p->rows);
  const size_t lds = (size_t)(p->span / 8);
  int64_t* ws = p->workspace.get();
  hipLaunchKernelGGL((segment_count<K, MARKS>), grid, dim3(kThreads), lds, s, (const uint16_t*)codes, codes_stride,
                     marks, marks_stride, ws, geo);
  hipLaunchKernelGGL(segment_scan, dim3((uint32_t)p->rows), dim3(64), 0, s, ws, used, p->blocks_per_row);
  if (pack)
    hipLaunchKernelGGL((segment_pack<K, MARKS>), grid, dim3(kThreads), lds, s, (const uint16_t*)codes, codes_stride,
                       marks, marks_stride, (const int64_t*)ws, table, table_stride, p->max_segments,
                       (uint16_t*)packed, packed_stride, p->capacity, geo);
}

int segment_apply(wfk_segment_rows_plan* p, const int16_t* codes, int64_t codes_stride, const uint8_t* marks,
                  int64_t marks_stride, bool use_marks, int bit, int32_t* table, int64_t table_stride, int16_t* packed,
                  int64_t packed_stride, int64_t* used, hipStream_t s) {
  const char* stage = "segment rows";
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (bit < 0 || bit > 15) return wfk_fail(WFK_EINVAL, "segment rows: bit must lie in [0, 15]");
  if (!used) return wfk_fail(WFK_EINVAL, "segment rows: used is null");
  // the sizing pass gives neither; a side that holds nothing (max_segments = 0, capacity = 0) is not looked at
  const bool sizing = !table && !packed;
  const bool has_table = !sizing && p->max_segments > 0, has_packed = !sizing && p->capacity > 0;
  if (has_table && !table) return wfk_fail(WFK_EINVAL, "segment rows: null table with a packed buffer");
  if (has_packed && !packed) return wfk_fail(WFK_EINVAL, "segment rows: null packed with a table buffer");
  const int64_t rows = p->rows;
  const RowReport report{used, rows, 2};
  if (p->n == 0) return wfk_zero_report(stage, report, s);
  if (use_marks && !marks) return wfk_fail(WFK_EINVAL, "segment rows: null marks buffer");
  if (const int rc = wfk_segment_row_rule(SegmentShape{rows, p->n, p->k, p->max_segments, p->capacity}, codes,
                                          codes_stride, use_marks ? marks : nullptr, marks_stride, table, table_stride,
                                          packed, packed_stride, used, wfk_fail))
    return rc;
  const SegGeom geo{p->n, p->span, p->blocks_per_row, p->ash, bit};
  const bool pack = has_table || has_packed;
  if (p->k == 2) {
    if (use_marks)
      segment_launch<2, true>(p, geo, codes, codes_stride, marks, marks_stride, table, table_stride, packed,
                              packed_stride, used, pack, s);
    else
      segment_launch<2, false>(p, geo, codes, codes_stride, nullptr, 0, table, table_stride, packed, packed_stride,
                               used, pack, s);
  } else {
    if (use_marks)
      segment_launch<1, true>(p, geo, codes, codes_stride, marks, marks_stride, table, table_stride, packed,
                              packed_stride, used, pack, s);
    else
      segment_launch<1, false>(p, geo, codes, codes_stride, nullptr, 0, table, table_stride, packed, packed_stride,
                               used, pack, s);
  }
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "segment rows kernel launch failed");
  return WFK_OK;
}

}  // namespace

extern "C" {

int wfk_segment_rows_plan_destroy(wfk_segment_rows_plan* p) {
  delete p;
  return WFK_OK;
}

int64_t wfk_segment_rows_span(const wfk_segment_rows_plan* p) { return p ? p->span : 0; }

const char* wfk_segment_rows_kernel_name(const wfk_segment_rows_plan* p, int launch, int with_marks) {
  if (!p) return "";
  if (launch == 1) return "segment_scan";
  if (launch == 0) {
    if (p->k == 2) return with_marks ? "segment_count<2, true>" : "segment_count<2, false>";
    return with_marks ? "segment_count<1, true>" : "segment_count<1, false>";
  }
  if (launch == 2) {
    if (p->k == 2) return with_marks ? "segment_pack<2, true>" : "segment_pack<2, false>";
    return with_marks ? "segment_pack<1, true>" : "segment_pack<1, false>";
  }
  return "";
}

int wfk_segment_rows_plan_create(int64_t n, int32_t rows, int width, int64_t align, int64_t max_segments,
                                 int64_t capacity, wfk_segment_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 0 || n > 0x7fffffffLL) return wfk_fail(WFK_EINVAL, "segment rows plan: n must lie in [0, 2^31 - 1]");
  if (rows < 1) return wfk_fail(WFK_EINVAL, "segment rows plan: rows must be at least 1");
  if (width != 1 && width != 2) return wfk_fail(WFK_EINVAL, "segment rows plan: width must be 1 or 2");
  if (align < 1 || align > WFK_SEGMENT_MAX_ALIGN || (align & (align - 1)))
    return wfk_fail(WFK_EINVAL, "segment rows plan: align must be a power of two in [1, " +
                                    std::to_string(WFK_SEGMENT_MAX_ALIGN) + "]");
  if (max_segments < 0) return wfk_fail(WFK_EINVAL, "segment rows plan: max_segments must not be negative");
  if (capacity < 0 || capacity > n) return wfk_fail(WFK_EINVAL, "segment rows plan: capacity must lie in [0, n]");
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("segment rows plan", n, segment_span(align), 0, rows, &bpr)) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_segment_rows_plan> p(new wfk_segment_rows_plan());
  p->n = n; p->rows = rows; p->k = width; p->max_segments = max_segments; p->capacity = capacity;
  p->span = segment_span(align);
  p->blocks_per_row = bpr;
  while ((1ll << p->ash) < align) ++p->ash;
  if (bpr && !p->workspace.alloc((size_t)rows * bpr * kPartial * sizeof(int64_t))) {
    (void)hipGetLastError();
    return wfk_fail(WFK_EHIP, "segment rows plan: workspace allocation failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the segment rows plan");
}

int wfk_segment_rows_apply_bit(wfk_segment_rows_plan* p, const int16_t* codes_dev, int64_t codes_stride, int bit,
                               int32_t* table_dev, int64_t table_stride, int16_t* packed_dev, int64_t packed_stride,
                               int64_t* used_dev, void* hip_stream) {
  return segment_apply(p, codes_dev, codes_stride, nullptr, 0, false, bit, table_dev, table_stride, packed_dev,
                       packed_stride, used_dev, (hipStream_t)hip_stream);
}

int wfk_segment_rows_apply_marks(wfk_segment_rows_plan* p, const int16_t* codes_dev, int64_t codes_stride,
                                 const uint8_t* marks_dev, int64_t marks_stride, int32_t* table_dev,
                                 int64_t table_stride, int16_t* packed_dev, int64_t packed_stride, int64_t* used_dev,
                                 void* hip_stream) {
  return segment_apply(p, codes_dev, codes_stride, marks_dev, marks_stride, true, 0, table_dev, table_stride,
                       packed_dev, packed_stride, used_dev, (hipStream_t)hip_stream);
}

}  // extern "C"
