// wfk_segment_library.hip -- the waveform library of a segment stage's rows: the segments of a row whose codes are
// equal share one slot of the row's library, so that what crosses to the host, and what the waveform memory holds,
// scales with the distinct pulses of a channel and not with the pulses played.  It reads what wfk_segment_rows wrote
// (table, packed, used) and never writes it.  Two segments of a row are equal when their lengths and their k length
// codes are; among equal segments the one with the lowest j is the FIRST; the firsts in ascending j are the slots
// u = 0, 1, ...:  lib_offset_u = the lengths of the slots before it, unique = the slots, lib_kept = their lengths.
//
// Execution form.  Four launches on the stream (three in the sizing pass); a wave owns a segment, a workgroup
// kSegsPerBlock consecutive segments of its row.  The row's hash table is tab[0 .. T_row), T_row = the power of two
// >= max(64, 2 count): it is sized by the row's count, so an apply costs what the row holds and not what the plan
// allows.  A slot of it holds kEmpty or the lowest segment id that has joined it so far.
// 0. seglib_hash:  the workgroups that own segments clear tab[0 .. T_row) between them; a wave validates its entry and
//    forms the 64-bit hash of (length, codes) as a wrapping SUM over the code positions p of a term of (p, code): the
//    order of the additions, and so the load path and the segment's alignment, cannot change it.
// 1. seglib_match: the wave probes from hash & (T_row - 1), at most T_row slots.  An empty slot: compare-and-swap of
//    its id; a slot that holds v: hash, length, then the codes of v against its own, 16 bytes a lane; equal: atomicMin
//    of its id onto the slot (left out where v is already lower: the slot only goes down); different: the next slot.
//    Whatever id a slot holds is a member of the slot's class, so the comparison may be made against any value read.
//    A failed compare-and-swap compares with what it found: nothing waits.  The slot goes to slot_of[j].
// 2. seglib_scan:  one wave per row, 64 segments at a time: first_j = (tab[slot_of[j]] == j), exclusive sums of first
//    and of first * length into the workspace, the row's verdict, lib_used.
// 3. seglib_copy:  segment j writes plays[j] and slots[j] from the sums of its first; a first copies its codes to the
//    library up to the cut: element stores up to the library's first 16-byte boundary, at the end and at the cut, 16
//    bytes a lane between.
// The codes of a segment start wherever offset puts them, so they are loaded through a 2-byte aligned 16-byte type:
// gfx950 takes such a load as one instruction, and no code before or after the segment is read.
// Every index that comes out of table / used is validated before it is used: an entry that would reach outside the
// packed row is never followed, and its row is reported [-1, -1].
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <new>
#include <string>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rows_dev.h"

namespace {

constexpr int kWaves = kThreads / 64;            // a wave per segment
constexpr int kPerWave = 4;                      // segments a wave takes in turn
constexpr int kSegsPerBlock = kWaves * kPerWave;
constexpr int32_t kEmpty = 0x7fffffff;           // above every segment id, so atomicMin keeps the lowest
constexpr int64_t kMaxSegments = 1ll << 30;      // segment ids are int32, and T = 2 max_segments fits a uint32

// the plan's workspace, all of it rewritten by every apply before it is read
struct LibWs {
  uint64_t* hash;      // [rows][M]  hash of segment j
  int64_t* uoff;       // [rows][M]  lengths of the firsts before j
  int32_t* tab;        // [rows][T]  the hash table
  int32_t* slot_of;    // [rows][M]  the slot of tab that segment j joined, or -1
  int32_t* uidx;       // [rows][M]  firsts before j
  int32_t* bad;        // [rows]     the row's verdict, by the scan
};

struct LibGeom {
  int64_t max_segments, capacity, lib_capacity;
  int64_t table_slots;        // T
  uint64_t hash_mask;
  uint32_t blocks_per_row;
  int k;
};

// 16 bytes of codes from an address that is a multiple of 2
struct __attribute__((packed, aligned(2))) Codes8 { uint32_t w[4]; };
__device__ __forceinline__ uint4 load_codes8(const uint16_t* p) {
  const Codes8 v = *reinterpret_cast<const Codes8*>(p);
  return make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
}

// the row's count where used[row] can be believed, -1 where not
__device__ __forceinline__ int64_t row_count(const int64_t* __restrict__ used, uint32_t row, const LibGeom& geo) {
  const int64_t count = used[(int64_t)row * 2], kept = used[(int64_t)row * 2 + 1];
  return count < 0 || count > geo.max_segments || kept < 0 || kept > geo.capacity ? -1 : count;
}

// the slots of a row's hash table: a power of two, >= 64, >= 2 count, <= T (count <= max_segments)
__device__ __forceinline__ uint32_t row_slots(int64_t count) {
  return count <= 32 ? 64u : 1u << (64 - __builtin_clzll((uint64_t)(2 * count - 1)));
}

struct Entry {
  int64_t start, length, offset;
  bool ok;   // its codes lie in the packed row
};
__device__ __forceinline__ Entry read_entry(const int32_t* __restrict__ t, int64_t j, int64_t capacity) {
  Entry e{t[j * 3], t[j * 3 + 1], t[j * 3 + 2], false};
  e.ok = e.length > 0 && e.offset >= 0 && e.offset + e.length <= capacity;
  return e;
}

__device__ __forceinline__ void add_term(uint32_t& a, uint32_t& b, uint32_t code, uint32_t p) {
  uint32_t t = code + p * 0x9E3779B1u;
  t *= 0x85EBCA6Bu;
  t ^= t >> 13;
  t *= 0xC2B2AE35u;
  t ^= t >> 16;
  a += t;
  b += (t >> 5 | t << 27) * 0x27D4EB2Fu + p;
}

// the hash of ne codes at c and of the length, the same in every lane of the wave
__device__ __forceinline__ uint64_t wave_hash(const uint16_t* __restrict__ c, int64_t ne, int64_t length, int lane) {
  uint32_t a = 0, b = 0;
  const int64_t nch = ne >> 3;
  for (int64_t q = lane; q < nch; q += 64) {
    const uint4 v = load_codes8(c + q * 8);
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) add_term(a, b, (d[e / 2] >> (16 * (e & 1))) & 0xffffu, (uint32_t)(q * 8 + e));
  }
  const int64_t p = nch * 8 + lane;
  if (p < ne) add_term(a, b, c[p], (uint32_t)p);
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    a += __shfl_xor(a, d);
    b += __shfl_xor(b, d);
  }
  uint64_t h = ((uint64_t)b << 32 | a) ^ (uint64_t)length * 0x9E3779B97F4A7C15ull;
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  return h;
}

// are the ne codes at a and at b equal (the same answer in every lane)
__device__ __forceinline__ bool wave_equal(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b, int64_t ne,
                                           int lane) {
  const int64_t nch = ne >> 3;
  for (int64_t base = 0; base < nch; base += 64) {
    const int64_t q = base + lane;
    bool diff = false;
    if (q < nch) {
      const uint4 x = load_codes8(a + q * 8), y = load_codes8(b + q * 8);
      diff = x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    }
    if (__any(diff)) return false;
  }
  const int64_t p = nch * 8 + lane;
  return !__any(p < ne && a[p] != b[p]);
}

__global__ void __launch_bounds__(kThreads)
    seglib_hash(const int32_t* __restrict__ table, int64_t table_stride, const uint16_t* __restrict__ packed,
                int64_t packed_stride, const int64_t* __restrict__ used, LibWs ws, LibGeom geo) {
  const auto [row, blk] = row_block(geo.blocks_per_row);
  const int64_t count = row_count(used, row, geo);
  const int64_t owners = (count + kSegsPerBlock - 1) / kSegsPerBlock;   // the workgroups of the row that own segments
  if (blk >= owners) return;                                            // (a bad row: owners = 0)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t T = row_slots(count), per = (T + owners - 1) / owners;
  int32_t* tab = ws.tab + (int64_t)row * geo.table_slots;
  const int64_t hi = (blk + 1) * per < T ? (blk + 1) * per : T;
  for (int64_t i = blk * per + tid; i < hi; i += kThreads) tab[i] = kEmpty;
  const int32_t* t = table + (int64_t)row * table_stride;
  const uint16_t* y = packed + (int64_t)row * packed_stride;
  uint64_t* hash = ws.hash + (int64_t)row * geo.max_segments;
  for (int i = 0; i < kPerWave; ++i) {
    const int64_t j = (int64_t)blk * kSegsPerBlock + i * kWaves + wave;
    if (j >= count) break;
    const Entry e = read_entry(t, j, geo.capacity);
    uint64_t h = 0;
    if (e.ok) h = wave_hash(y + e.offset * geo.k, e.length * geo.k, e.length, lane) & geo.hash_mask;
    if (lane == 0) hash[j] = h;
  }
}

__global__ void __launch_bounds__(kThreads)
    seglib_match(const int32_t* __restrict__ table, int64_t table_stride, const uint16_t* __restrict__ packed,
                 int64_t packed_stride, const int64_t* __restrict__ used, LibWs ws, LibGeom geo) {
  const auto [row, blk] = row_block(geo.blocks_per_row);
  const int64_t count = row_count(used, row, geo);
  if ((int64_t)blk * kSegsPerBlock >= count) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t T = row_slots(count);
  int32_t* tab = ws.tab + (int64_t)row * geo.table_slots;
  const int32_t* t = table + (int64_t)row * table_stride;
  const uint16_t* y = packed + (int64_t)row * packed_stride;
  const uint64_t* hash = ws.hash + (int64_t)row * geo.max_segments;
  int32_t* slot_of = ws.slot_of + (int64_t)row * geo.max_segments;
  for (int i = 0; i < kPerWave; ++i) {
    const int64_t j = (int64_t)blk * kSegsPerBlock + i * kWaves + wave;
    if (j >= count) break;
    const Entry e = read_entry(t, j, geo.capacity);
    int32_t found = -1;
    if (e.ok) {
      const uint64_t h = hash[j];
      const uint16_t* a = y + e.offset * geo.k;
      uint32_t s = (uint32_t)h & (T - 1);
      for (uint32_t step = 0; step < T; ++step, s = (s + 1) & (T - 1)) {
        int32_t v = 0;
        if (lane == 0) {
          v = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (v == kEmpty) {
            const int32_t old = atomicCAS(&tab[s], kEmpty, (int32_t)j);
            v = old == kEmpty ? (int32_t)j : old;
          }
        }
        v = __shfl(v, 0);
        if (v == (int32_t)j) {   // claimed: ids are unique, nobody else writes this one
          found = (int32_t)s;
          break;
        }
        if (v < 0 || v >= count || hash[v] != h) continue;   // (only ids of the row are ever put there)
        const Entry o = read_entry(t, v, geo.capacity);
        if (!o.ok || o.length != e.length || !wave_equal(a, y + o.offset * geo.k, e.length * geo.k, lane)) continue;
        if (lane == 0 && v > (int32_t)j) atomicMin(&tab[s], (int32_t)j);   // (the slot only ever goes down)
        found = (int32_t)s;
        break;
      }
    }
    if (lane == 0) slot_of[j] = found;
  }
}

// one wave per row; lib_used: [rows][2]
__global__ void __launch_bounds__(64)
    seglib_scan(const int32_t* __restrict__ table, int64_t table_stride, const int64_t* __restrict__ used, LibWs ws,
                int64_t* __restrict__ lib_used, LibGeom geo) {
  const uint32_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t count = row_count(used, row, geo);
  const int32_t* t = table + (int64_t)row * table_stride;
  const int32_t* tab = ws.tab + (int64_t)row * geo.table_slots;
  const int32_t* slot_of = ws.slot_of + (int64_t)row * geo.max_segments;
  int32_t* uidx = ws.uidx + (int64_t)row * geo.max_segments;
  int64_t* uoff = ws.uoff + (int64_t)row * geo.max_segments;
  const uint32_t T = row_slots(count < 0 ? 0 : count);
  long long uniq_c = 0, kept_c = 0;
  bool bad = count < 0;
  for (int64_t base = 0; base < count; base += 64) {
    const int64_t j = base + lane;
    long long f = 0, len = 0;
    bool wrong = false;
    if (j < count) {
      const Entry e = read_entry(t, j, geo.capacity);
      const int32_t s = slot_of[j];
      wrong = !e.ok || s < 0 || (uint32_t)s >= T;
      if (!wrong && tab[s] == (int32_t)j) {
        f = 1;
        len = e.length;
      }
    }
    bad = bad || __any(wrong);
    long long f_i = f, len_i = len;   // inclusive over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long a = __shfl_up(f_i, d), b = __shfl_up(len_i, d);
      if (lane >= d) {
        f_i += a;
        len_i += b;
      }
    }
    if (j < count) {
      uidx[j] = (int32_t)(uniq_c + f_i - f);
      uoff[j] = kept_c + len_i - len;
    }
    uniq_c += __shfl(f_i, 63);
    kept_c += __shfl(len_i, 63);
  }
  if (lane == 0) {
    lib_used[(int64_t)row * 2] = bad ? -1 : uniq_c;
    lib_used[(int64_t)row * 2 + 1] = bad ? -1 : kept_c;
    ws.bad[row] = bad;
  }
}

// plays: [rows] rows of 3 M int32, slots: [rows] rows of M int32, library: [rows] rows of k lib_capacity int16; any of
// them may be null
__global__ void __launch_bounds__(kThreads)
    seglib_copy(const int32_t* __restrict__ table, int64_t table_stride, const uint16_t* __restrict__ packed,
                int64_t packed_stride, const int64_t* __restrict__ used, LibWs ws, int32_t* __restrict__ plays,
                int64_t plays_stride, int32_t* __restrict__ slots, int64_t slots_stride, uint16_t* __restrict__ library,
                int64_t library_stride, LibGeom geo) {
  const auto [row, blk] = row_block(geo.blocks_per_row);
  const int64_t count = row_count(used, row, geo);
  if ((int64_t)blk * kSegsPerBlock >= count || ws.bad[row]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* t = table + (int64_t)row * table_stride;
  const int32_t* tab = ws.tab + (int64_t)row * geo.table_slots;
  const int32_t* slot_of = ws.slot_of + (int64_t)row * geo.max_segments;
  const int32_t* uidx = ws.uidx + (int64_t)row * geo.max_segments;
  const int64_t* uoff = ws.uoff + (int64_t)row * geo.max_segments;
  for (int i = 0; i < kPerWave; ++i) {
    const int64_t j = (int64_t)blk * kSegsPerBlock + i * kWaves + wave;
    if (j >= count) break;
    const Entry e = read_entry(t, j, geo.capacity);   // ok, and slot_of[j] a slot: the scan found the row good
    const int64_t first = tab[slot_of[j]];
    const int64_t off = uoff[first];
    if (lane == 0) {
      if (plays) {
        int32_t* p = plays + (int64_t)row * plays_stride + j * 3;
        p[0] = (int32_t)e.start;
        p[1] = (int32_t)e.length;
        p[2] = (int32_t)off;
      }
      if (slots) slots[(int64_t)row * slots_stride + j] = uidx[first];
    }
    if (!library || first != j || off >= geo.lib_capacity) continue;
    const int64_t room = geo.lib_capacity - off;
    const int64_t ne = (e.length < room ? e.length : room) * geo.k;   // the cut is by position
    const uint16_t* __restrict__ src = packed + (int64_t)row * packed_stride + e.offset * geo.k;
    uint16_t* __restrict__ dst = library + (int64_t)row * library_stride + off * geo.k;
    int64_t head = (8 - (int64_t)((reinterpret_cast<uintptr_t>(dst) >> 1) & 7)) & 7;   // codes to dst's 16-byte boundary
    if (head > ne) head = ne;
    if (lane < head) dst[lane] = src[lane];
    const int64_t nch = (ne - head) >> 3;
    for (int64_t q = lane; q < nch; q += 64)
      *reinterpret_cast<uint4*>(dst + head + q * 8) = load_codes8(src + head + q * 8);
    const int64_t p = head + nch * 8 + lane;
    if (p < ne) dst[p] = src[p];
  }
}

}  // namespace

struct wfk_segment_library_plan {
  int64_t max_segments = 0, capacity = 0, lib_capacity = 0, table_slots = 0;
  int32_t rows = 0;
  int k = 0, hash_bits = 64;
  uint32_t blocks_per_row = 0;
  DevBuf<uint64_t> hash;
  DevBuf<int64_t> uoff;
  DevBuf<int32_t> tab, slot_of, uidx, bad;
  std::string names[4];
};

extern "C" {

int wfk_segment_library_plan_destroy(wfk_segment_library_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_segment_library_kernel_name(const wfk_segment_library_plan* p, int launch) {
  return p && launch >= 0 && launch < 4 ? p->names[launch].c_str() : "";
}

int wfk_segment_library_plan_create(int32_t rows, int width, int64_t max_segments, int64_t capacity,
                                    int64_t lib_capacity, wfk_segment_library_plan** out) try {
  const std::string who = "segment library plan: ";
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (rows < 1) return wfk_fail(WFK_EINVAL, who + "rows must be at least 1");
  if (width != 1 && width != 2) return wfk_fail(WFK_EINVAL, who + "width must be 1 or 2");
  if (max_segments < 0) return wfk_fail(WFK_EINVAL, who + "max_segments must not be negative");
  if (max_segments > kMaxSegments) return wfk_fail(WFK_EINVAL, who + "max_segments must not exceed 2^30");
  if (capacity < 0 || capacity > 0x7fffffffLL) return wfk_fail(WFK_EINVAL, who + "capacity must lie in [0, 2^31 - 1]");
  if (lib_capacity < 0 || lib_capacity > capacity)
    return wfk_fail(WFK_EINVAL, who + "lib_capacity must lie in [0, capacity]");
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("segment library plan", max_segments, kSegsPerBlock, 0, rows, &bpr)) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_segment_library_plan> p(new wfk_segment_library_plan());
  p->rows = rows; p->k = width; p->max_segments = max_segments; p->capacity = capacity; p->lib_capacity = lib_capacity;
  p->blocks_per_row = bpr;
  p->table_slots = 64;
  while (p->table_slots < 2 * max_segments) p->table_slots <<= 1;
  if (const char* bits = std::getenv("WFK_SEGLIB_HASH_BITS")) {
    char* end = nullptr;
    const long b = std::strtol(bits, &end, 10);
    if (end != bits && !*end && b >= 0 && b <= 64) p->hash_bits = (int)b;
  }
  const std::string kept = p->hash_bits < 64 ? " [hash bits " + std::to_string(p->hash_bits) + "]" : "";
  p->names[0] = "seglib_hash" + kept;
  p->names[1] = "seglib_match" + kept;
  p->names[2] = "seglib_scan";
  p->names[3] = "seglib_copy";
  const size_t r = (size_t)rows, m = (size_t)max_segments;
  const bool got = p->bad.alloc(r * sizeof(int32_t)) && p->tab.alloc(r * (size_t)p->table_slots * sizeof(int32_t)) &&
                   (!m || (p->hash.alloc(r * m * sizeof(uint64_t)) && p->uoff.alloc(r * m * sizeof(int64_t)) &&
                           p->slot_of.alloc(r * m * sizeof(int32_t)) && p->uidx.alloc(r * m * sizeof(int32_t))));
  if (!got) {
    (void)hipGetLastError();
    return wfk_fail(WFK_EHIP, who + "workspace allocation failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the segment library plan");
}

int wfk_segment_library_apply(wfk_segment_library_plan* p, const int32_t* table, int64_t table_stride,
                              const int16_t* packed, int64_t packed_stride, const int64_t* used, int32_t* plays,
                              int64_t plays_stride, int32_t* slots, int64_t slots_stride, int16_t* library,
                              int64_t library_stride, int64_t* lib_used, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (!lib_used) return wfk_fail(WFK_EINVAL, "segment library: lib_used is null");
  if (!used) return wfk_fail(WFK_EINVAL, "segment library: used is null");
  if (const int rc = wfk_segment_library_row_rule(
          SegmentLibraryShape{p->rows, p->k, p->max_segments, p->capacity, p->lib_capacity}, table, table_stride, packed,
          packed_stride, used, plays, plays_stride, slots, slots_stride, library, library_stride, lib_used, wfk_fail))
    return rc;
  // an output that holds nothing is not written: the kernels are not given it
  if (!p->max_segments) plays = slots = nullptr;
  if (!p->lib_capacity) library = nullptr;
  hipStream_t s = (hipStream_t)hip_stream;
  const LibWs ws{p->hash.get(), p->uoff.get(), p->tab.get(), p->slot_of.get(), p->uidx.get(), p->bad.get()};
  uint64_t mask = p->hash_bits >= 64 ? ~0ull : (1ull << p->hash_bits) - 1;
  const LibGeom geo{p->max_segments, p->capacity, p->lib_capacity, p->table_slots, mask, p->blocks_per_row, p->k};
  const dim3 grid(p->blocks_per_row * (uint32_t)p->rows);
  const uint16_t* y = (const uint16_t*)packed;
  if (p->blocks_per_row) {
    hipLaunchKernelGGL(seglib_hash, grid, dim3(kThreads), 0, s, table, table_stride, y, packed_stride, used, ws, geo);
    hipLaunchKernelGGL(seglib_match, grid, dim3(kThreads), 0, s, table, table_stride, y, packed_stride, used, ws, geo);
  }
  hipLaunchKernelGGL(seglib_scan, dim3((uint32_t)p->rows), dim3(64), 0, s, table, table_stride, used, ws, lib_used, geo);
  if (p->blocks_per_row && (plays || slots || library))
    hipLaunchKernelGGL(seglib_copy, grid, dim3(kThreads), 0, s, table, table_stride, y, packed_stride, used, ws, plays,
                       plays_stride, slots, slots_stride, (uint16_t*)library, library_stride, geo);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "segment library kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
