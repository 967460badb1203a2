// wfk_avg.hip -- per-step shot sums of digitiser traces: the reduction over SHOTS that goes with the demodulator's
// reduction over time.  A block of S traces of N samples (int16 ADC codes, float32 or float64; row stride >= N) was
// taken while the sequence cycled through G steps; `first` shots came before the block, so
//   shot s of the block belongs to step (first + s) mod G
// and the apply forms, per step g and column c, over the block's shots of that step,
//   sum[g, c] = SUM x[s, c]        sumsq[g, c] = SUM x[s, c]^2       (sumsq optional)
// in int64 for codes (exact) and in fp64 for floats (a float32 sample is widened first, so its square is exact).
// accumulate = 0 overwrites both outputs (a step without a shot gets 0); accumulate = 1 adds the block's sums to what
// is there, one add per element, and leaves a step without a shot in the block bit for bit as it was.
//
// avg_tile<T, SQ>: lanes own columns.  A lane reads 16 bytes of a row (8 codes / 4 floats / 2 doubles), a workgroup
// of 256 lanes a column tile of 256 such vectors; it owns ONE step and a range of that step's shots and walks its rows
// G rows apart, kRows of them loaded before the first is added, so that many 16-byte loads per lane are in flight.
// Nothing is reused and nothing is shared: no LDS, no barrier, every input byte is read once.  A row that does not
// start on a 16-byte boundary (rows are windows at any element, at any stride) and the vector that crosses column N
// are read element by element.  Every row offset is 64-bit.
// Codes: 64-bit adds are two instructions here, so a run of rows is added in 32 bits and widened once.
//   a sum of R codes is at most R * 32768 in magnitude, below 2^31 for every R <= 65535: the run is the kRowsI16 = 6
//     rows of one batch, far inside that;
//   a square is at most 2^30: uint32 holds 3 of them (3 * 2^30 < 2^32) and not 4 (4 * 2^30 = 2^32); the run is 3 rows,
//     two runs per batch, added modulo 2^32 and read back as unsigned.
// Floats: one fp64 accumulator per column, rows added in ascending shot order (the square by one fused multiply-add).
//
// Few column tiles (N = 4096 codes are two) cannot fill the chip, so the shots of a step are split over `splits`
// workgroups; the split rule is splits_for() below, a function of (S, G, N, dtype) alone.  splits == 1 writes the
// outputs directly.  Otherwise each workgroup stores its partial sums into its own slot of the plan's workspace
// ([split][step][tile] slots of 256 vectors) and avg_reduce adds the slots of every output element in a fixed order
// (16 threads per element, each every 16th split in ascending order, their sums in ascending order through LDS) and
// then does the one accumulate add.  No atomics anywhere: the order of every float addition is a fixed
// function of (S, G, N, first mod G, dtype), two applies of the same call agree to the bit, and a NaN or Inf reaches
// its own (step, column) only.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <type_traits>

#include "wfk.h"
#include "wfk_host.h"

namespace {

constexpr int kThreads = 256;    // lanes of a workgroup: 16-byte vectors of a column tile
constexpr int kTarget = 1024;    // workgroups a split launch aims at (4 per CU); the workspace has this many slots
constexpr int kMinRows = 32;     // a split keeps at least this many shots of its step
constexpr int kRowsI16 = 6;      // rows of a batch: loads in flight per lane; two runs of 3 squares (see above)
constexpr int kRowsF = 8;        // (12 / 16 rows and 2048 workgroups measured no faster: DESIGN.md 3.18)
constexpr int kRedLanes = 16;    // avg_reduce: threads that share the splits of one output
constexpr int kRedCols = kThreads / kRedLanes;
static_assert(kRowsI16 % 3 == 0, "a batch of code rows is whole runs of 3 squares");

template <typename T>
using acc_t = std::conditional_t<std::is_same_v<T, int16_t>, long long, double>;

// 16 bytes of a row from column c on, zeros past N (demodulator's load_seg)
template <typename T>
__device__ __forceinline__ uint4 load_vec(const T* __restrict__ p, int64_t c, int64_t N) {
  constexpr int E = 16 / sizeof(T);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  if (c + E <= N && ((uintptr_t)p & 15) == 0) {   // read once and never again: a non-temporal load
    const u32x4 q = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(q.x, q.y, q.z, q.w);
  }
  union {
    uint4 v;
    T e[E];
  } u;
#pragma unroll
  for (int i = 0; i < E; ++i) u.e[i] = c + i < N ? p[i] : (T)0;
  return u.v;
}

__device__ __forceinline__ int code_of(const uint4 v, int e) {
  const unsigned w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return (e & 1) ? (int)w >> 16 : (int)(short)(w & 0xffffu);
}

template <typename T>
__device__ __forceinline__ double real_of(const uint4 v, int e);
template <>
__device__ __forceinline__ double real_of<float>(const uint4 v, int e) {
  return (double)__uint_as_float(e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w);
}
template <>
__device__ __forceinline__ double real_of<double>(const uint4 v, int e) {
  return e == 0 ? __hiloint2double((int)v.y, (int)v.x) : __hiloint2double((int)v.w, (int)v.z);
}

// the first shot of step g in a block that `phase` = first mod G shots of the cycle precede, and how many of the
// block's S shots the step has
__device__ __forceinline__ int64_t step_start(int64_t g, int64_t phase, int64_t G) {
  const int64_t s0 = g - phase;
  return s0 < 0 ? s0 + G : s0;
}
__device__ __forceinline__ int64_t step_shots(int64_t s0, int64_t S, int64_t G) {
  return s0 < S ? (S - s0 - 1) / G + 1 : 0;
}

// X: S rows of >= N samples, ldx apart.  Grid: tiles * G * splits workgroups, block b = (split * G + step) * tiles +
// tile; split k takes shots [k * chunk, (k + 1) * chunk) of its step's list.  part / partq null: splits == 1, the
// sums go to sum / sq (rows ld_sum / ld_sq apart), added to what is there when `accumulate`; else into slot b.
template <typename T, bool SQ>
__global__ void __launch_bounds__(kThreads)
    avg_tile(const T* __restrict__ X, int64_t S, int64_t N, int64_t ldx, int64_t G, int64_t phase, int64_t tiles,
             int64_t chunk, acc_t<T>* __restrict__ sum, int64_t ld_sum, acc_t<T>* __restrict__ sq, int64_t ld_sq,
             acc_t<T>* __restrict__ part, acc_t<T>* __restrict__ partq, int accumulate) {
  constexpr int E = 16 / sizeof(T);
  using A = acc_t<T>;
  const int64_t b = blockIdx.x;
  const int64_t tile = b % tiles, g = (b / tiles) % G, k = b / (tiles * G);
  const int64_t c0 = (tile * kThreads + threadIdx.x) * E;
  if (c0 >= N) return;
  const int64_t s0 = step_start(g, phase, G);
  const int64_t m = step_shots(s0, S, G);
  if (m == 0 && accumulate && !part) return;   // a step without a shot keeps its bits
  const int64_t i0 = min(m, k * chunk), i1 = min(m, i0 + chunk);
  const T* __restrict__ x = X + c0;
  const int64_t hop = G * ldx;
  const T* __restrict__ row = x + (s0 + i0 * G) * ldx;

  A acc[E], accq[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = accq[e] = 0;

  int64_t i = i0;
  if constexpr (std::is_same_v<T, int16_t>) {
    for (; i + kRowsI16 <= i1; i += kRowsI16, row += kRowsI16 * hop) {
      uint4 v[kRowsI16];
#pragma unroll
      for (int j = 0; j < kRowsI16; ++j) v[j] = load_vec<T>(row + j * hop, c0, N);
      int s32[E];
#pragma unroll
      for (int e = 0; e < E; ++e) s32[e] = 0;
#pragma unroll
      for (int j0 = 0; j0 < kRowsI16; j0 += 3) {
        unsigned q32[E];
#pragma unroll
        for (int e = 0; e < E; ++e) q32[e] = 0;
#pragma unroll
        for (int j = j0; j < j0 + 3; ++j)
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int c = code_of(v[j], e);
            s32[e] += c;
            if (SQ) q32[e] += (unsigned)(c * c);
          }
        if (SQ) {
#pragma unroll
          for (int e = 0; e < E; ++e) accq[e] += (long long)q32[e];
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] += (long long)s32[e];
    }
    for (; i < i1; ++i, row += hop) {
      const uint4 v = load_vec<T>(row, c0, N);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = code_of(v, e);
        acc[e] += (long long)c;
        if (SQ) accq[e] += (long long)(c * c);
      }
    }
  } else {
    for (; i + kRowsF <= i1; i += kRowsF, row += kRowsF * hop) {
      uint4 v[kRowsF];
#pragma unroll
      for (int j = 0; j < kRowsF; ++j) v[j] = load_vec<T>(row + j * hop, c0, N);
#pragma unroll
      for (int j = 0; j < kRowsF; ++j)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double r = real_of<T>(v[j], e);
          acc[e] += r;
          if (SQ) accq[e] = fma(r, r, accq[e]);
        }
    }
    for (; i < i1; ++i, row += hop) {
      const uint4 v = load_vec<T>(row, c0, N);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double r = real_of<T>(v, e);
        acc[e] += r;
        if (SQ) accq[e] = fma(r, r, accq[e]);
      }
    }
  }

  if (part) {   // slot b of the workspace: kThreads vectors, a lane's E sums side by side
    A* dst = part + (b * kThreads + threadIdx.x) * E;
#pragma unroll
    for (int e = 0; e < E; ++e) dst[e] = acc[e];
    if (SQ) {
      A* dstq = partq + (b * kThreads + threadIdx.x) * E;
#pragma unroll
      for (int e = 0; e < E; ++e) dstq[e] = accq[e];
    }
    return;
  }
  A* dst = sum + g * ld_sum + c0;
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (c0 + e < N) dst[e] = accumulate ? dst[e] + acc[e] : acc[e];
  if (SQ) {
    A* dstq = sq + g * ld_sq + c0;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (c0 + e < N) dstq[e] = accumulate ? dstq[e] + accq[e] : accq[e];
  }
}

// sum[g, c] (and sq[g, c] when partq is there) = the slots of (step g, the tile of c) added up, then -- `accumulate`
// -- added to what is there.  A workgroup takes kRedCols consecutive outputs (g, c), kRedLanes threads each: thread j
// of an output adds the splits j, j + kRedLanes, ... in ascending order, the kRedLanes sums meet in LDS and thread 0
// adds them in ascending j.  tile_elems = kThreads * E columns per tile.
template <typename A>
__global__ void __launch_bounds__(kThreads)
    avg_reduce(const A* __restrict__ part, const A* __restrict__ partq, int64_t splits, int64_t S, int64_t N, int64_t G,
               int64_t phase, int64_t tiles, int64_t tile_elems, A* __restrict__ sum, int64_t ld_sum,
               A* __restrict__ sq, int64_t ld_sq, int accumulate) {
  __shared__ A red[2][kThreads];
  const int j = threadIdx.x / kRedCols, lc = threadIdx.x % kRedCols;
  const int64_t o = (int64_t)blockIdx.x * kRedCols + lc;
  const bool live = o < G * N;
  const int64_t g = live ? o / N : 0, c = live ? o % N : 0;
  const int64_t slot = (g * tiles + c / tile_elems) * tile_elems + c % tile_elems, hop = G * tiles * tile_elems;
  A t = 0, tq = 0;
  if (live) {
#pragma unroll 4
    for (int64_t k = j; k < splits; k += kRedLanes) {
      t += part[slot + k * hop];
      if (partq) tq += partq[slot + k * hop];
    }
  }
  red[0][threadIdx.x] = t;
  red[1][threadIdx.x] = tq;
  __syncthreads();
  if (j != 0 || !live) return;
  if (accumulate && step_shots(step_start(g, phase, G), S, G) == 0) return;   // a step without a shot keeps its bits
  for (int jj = 1; jj < kRedLanes && jj < splits; ++jj) {
    t += red[0][jj * kRedCols + lc];
    tq += red[1][jj * kRedCols + lc];
  }
  A* dst = sum + g * ld_sum + c;
  *dst = accumulate ? *dst + t : t;
  if (partq) {
    A* dstq = sq + g * ld_sq + c;
    *dstq = accumulate ? *dstq + tq : tq;
  }
}

int elem_bytes(int kind) { return kind == WFK_IN_F64 ? 8 : kind == WFK_IN_F32 ? 4 : 2; }

const char* type_name(int kind) { return kind == WFK_IN_F64 ? "double" : kind == WFK_IN_F32 ? "float" : "short"; }

}  // namespace

struct wfk_avg_plan {
  int64_t n = 0, steps = 0, tiles = 0;
  int kind = 0;
  int forced = 0;           // WFK_AVG_SPLITS when the plan was made (an experiment's and the tests' switch); 0: the rule
  DevBuf<char> ws;          // 2 x kTarget slots of kThreads x E 8-byte sums: the sums, then the squares
  std::string name;
};

namespace {

// How many workgroups share the shots of one step, for a block of S shots.  One when the column tiles times the
// steps already give kTarget workgroups; else as many as reach kTarget, while a split keeps kMinRows shots of its
// step (the longest step has ceil(S / G)).  splits * steps * tiles <= kTarget, the slots of the workspace.
// WFK_AVG_SPLITS = k asks for k splits instead, under the same cap.
int64_t splits_for(const wfk_avg_plan* p, int64_t S) {
  if (S <= 0) return 1;
  const int64_t cap = kTarget / p->tiles / p->steps;   // (each division first: no product to overflow)
  const int64_t longest = (S - 1) / p->steps + 1;
  int64_t ks = p->forced > 0 ? p->forced : longest / kMinRows;
  if (ks > cap) ks = cap;
  return ks > 1 ? ks : 1;
}

template <typename T>
void launch_t(const wfk_avg_plan* p, hipStream_t st, const void* X, int64_t S, int64_t ldx, int64_t phase, void* sum,
              int64_t ld_sum, void* sq, int64_t ld_sq, int accumulate, int64_t ks) {
  using A = acc_t<T>;
  constexpr int E = 16 / sizeof(T);
  const int64_t longest = (S - 1) / p->steps + 1, chunk = (longest - 1) / ks + 1;
  A* part = ks > 1 ? (A*)p->ws.get() : nullptr;
  A* partq = ks > 1 && sq ? part + (size_t)kTarget * kThreads * E : nullptr;
  const dim3 grid((unsigned)(p->tiles * p->steps * ks));
  if (sq)
    hipLaunchKernelGGL((avg_tile<T, true>), grid, dim3(kThreads), 0, st, (const T*)X, S, p->n, ldx, p->steps, phase,
                       p->tiles, chunk, (A*)sum, ld_sum, (A*)sq, ld_sq, part, partq, accumulate);
  else
    hipLaunchKernelGGL((avg_tile<T, false>), grid, dim3(kThreads), 0, st, (const T*)X, S, p->n, ldx, p->steps, phase,
                       p->tiles, chunk, (A*)sum, ld_sum, (A*)nullptr, ld_sq, part, partq, accumulate);
  if (ks > 1) {
    const int64_t blocks = (p->steps * p->n - 1) / kRedCols + 1;
    hipLaunchKernelGGL(avg_reduce<A>, dim3((unsigned)blocks), dim3(kThreads), 0, st, (const A*)part, (const A*)partq,
                       ks, S, p->n, p->steps, phase, p->tiles, (int64_t)kThreads * E, (A*)sum, ld_sum, (A*)sq, ld_sq,
                       accumulate);
  }
}

}  // namespace

extern "C" {

int wfk_avg_plan_destroy(wfk_avg_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_avg_plan_create(int64_t n_points, int64_t steps, int in_kind, wfk_avg_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n_points < 1) return wfk_fail(WFK_EINVAL, "trace averager plan: n_points < 1");
  if (steps < 1) return wfk_fail(WFK_EINVAL, "trace averager plan: steps < 1");
  if (in_kind != WFK_IN_F64 && in_kind != WFK_IN_F32 && in_kind != WFK_IN_I16)
    return wfk_fail(WFK_EINVAL, "trace averager plan: in_kind must be WFK_IN_F64, WFK_IN_F32 or WFK_IN_I16");
  const int64_t tile_elems = (int64_t)kThreads * (16 / elem_bytes(in_kind));
  const int64_t tiles = (n_points - 1) / tile_elems + 1;
  // one launch: tiles * steps workgroups (times the splits, which keep it under kTarget then)
  if (tiles > 0x7fffffffLL / steps)
    return wfk_fail(WFK_EINVAL, "trace averager plan: steps * n_points too large for one launch");
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_avg_plan> p(new wfk_avg_plan());
  p->n = n_points;
  p->steps = steps;
  p->kind = in_kind;
  p->tiles = tiles;
  const char* forced = std::getenv("WFK_AVG_SPLITS");
  p->forced = forced && *forced ? std::atoi(forced) : 0;
  // the workspace, where a block can split at all: sums and squares, 8 bytes per column of every slot
  if (kTarget / tiles / steps >= 2 && !p->ws.alloc((size_t)2 * kTarget * tile_elems * 8)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "trace averager plan: device allocation failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the trace averager plan");
}

int64_t wfk_avg_splits(const wfk_avg_plan* p, int64_t n_shots, int64_t first) {
  (void)first;   // the longest step of a block has ceil(n_shots / steps) shots wherever the block starts
  return p ? splits_for(p, n_shots) : 0;
}

int wfk_avg_apply(wfk_avg_plan* p, const void* traces_dev, int64_t n_shots, int64_t trace_stride, int64_t first,
                  void* sum_dev, int64_t sum_stride, void* sumsq_dev, int64_t sumsq_stride, int accumulate,
                  void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (n_shots < 0) return wfk_fail(WFK_EINVAL, "trace averager: n_shots < 0");
  if (first < 0) return wfk_fail(WFK_EINVAL, "trace averager: first < 0");
  const char* stage = "trace averager";
  const size_t es = (size_t)elem_bytes(p->kind);
  const RowSide sum{"sum", sum_dev, p->steps, sum_stride, p->n, 8};
  const RowSide sumsq{"sumsq", sumsq_dev, p->steps, sumsq_stride, p->n, 8};
  const RowSide traces{"traces", traces_dev, n_shots, trace_stride, p->n, es};
  // a block of no shots has no traces to hold to the rule: the outputs stand in for them
  if (n_shots == 0) {
    if (const int rc = wfk_row_rule(stage, {sum}, sum, kRowsAligned, wfk_fail)) return rc;
    if (sumsq_dev)
      if (const int rc = wfk_row_rule(stage, {sum}, sumsq, kRowsAligned | kRowsDisjoint, wfk_fail)) return rc;
  } else {
    if (const int rc = wfk_row_rule(stage, {traces}, sum, kRowsAligned | kRowsDisjoint, wfk_fail)) return rc;
    if (sumsq_dev)
      if (const int rc = wfk_row_rule(stage, {traces, sum}, sumsq, kRowsAligned | kRowsDisjoint, wfk_fail)) return rc;
  }
  if (n_shots == 0 && accumulate) return WFK_OK;   // nothing to add
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t ks = splits_for(p, n_shots);
  const int64_t phase = first % p->steps;
  // (a block of no shots runs the direct kernel: every step is without a shot and is zeroed)
  if (p->kind == WFK_IN_F64)
    launch_t<double>(p, st, traces_dev, n_shots, trace_stride, phase, sum_dev, sum_stride, sumsq_dev, sumsq_stride,
                     accumulate, ks);
  else if (p->kind == WFK_IN_F32)
    launch_t<float>(p, st, traces_dev, n_shots, trace_stride, phase, sum_dev, sum_stride, sumsq_dev, sumsq_stride,
                    accumulate, ks);
  else
    launch_t<int16_t>(p, st, traces_dev, n_shots, trace_stride, phase, sum_dev, sum_stride, sumsq_dev, sumsq_stride,
                      accumulate, ks);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "trace averager launch failed");
  return WFK_OK;
}

const char* wfk_avg_kernel_name(const wfk_avg_plan* p, int64_t n_shots, int with_sumsq) {
  if (!p) return "";
  wfk_avg_plan* q = const_cast<wfk_avg_plan*>(p);
  q->name = std::string("avg_tile<") + type_name(p->kind) + (with_sumsq ? ",sumsq>" : ">");
  if (splits_for(p, n_shots) > 1) q->name += " + avg_reduce";
  return q->name.c_str();
}

}  // extern "C"
