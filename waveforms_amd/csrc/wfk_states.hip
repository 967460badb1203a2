// wfk_states.hip -- IQ points to qubit states and per-step counts: the last link of the readout chain, behind the
// demodulator.  points: S rows of nf complex128 IQ points (row stride >= nf); centres: nf x K complex128, 2 <= K <= 8,
// a tone with fewer states pads its row with NaN.  Per shot s, tone j, state k, in double, every operation rounded on
// its own (no fused multiply-add: the bits of NumPy's dr * dr + di * di):
//   dr = re(p) - re(c),  di = im(p) - im(c),  d2 = fl(fl(dr * dr) + fl(di * di))
//   label = the first k of 0 .. K - 1 with d2 < best, best starting at +inf (strict: ties go to the lowest k, a NaN or
//           infinite d2 never wins), 255 when no centre wins
// and from the labels, all optional:
//   labels[s, j]  uint8
//   words[s]      int64, tone j in bits [j b, (j + 1) b), b = 1 / 2 / 3 for K = 2 / <= 4 / <= 8; -1 when a tone is invalid
//   counts[g, j, k]  int64 (steps, nf, K + 1): the block's shots of step g = (first + s) mod steps whose tone j got state
//                    k; column K counts the invalid ones
//   joint[g, w]   int64 (steps, 2^(nf b) + 1): the shots of step g whose word is w; the last bin those with word -1
// accumulate = 0 overwrites counts and joint (zeroed by a kernel on the stream, then added to), accumulate = 1 adds.
//
// states_block<KT>, KT = K rounded up to 2 / 4 / 8 (padded NaN centres never win).  A workgroup of 256 lanes owns a
// block of consecutive shots, tile_for() points of them at most; lanes own consecutive (shot, tone) points, 256 apart,
// and walk (shot, tone, step) by additions -- the divisions are done once per lane.  A point is one 16-byte
// non-temporal load (it is never read again), kBatch of them in flight per lane; with a row stride of nf the block is
// one contiguous stream, otherwise contiguous per row.  Label bytes of consecutive lanes are consecutive.  Every row
// offset is 64-bit.  The K centres of a tone are read through the cache (the table is nf * KT * 16 bytes, 128 KB at most).
// Words: the block's labels are kept in LDS; after a barrier one lane per shot packs its tones.  No second pass over
// the points.
// Counters, one routine for both tables: a table of at most kLdsEntries entries is counted in a per-workgroup LDS
// histogram of 32-bit counters (a block has far fewer than 2^32 points) and flushed with one 64-bit global atomic add
// per non-zero entry; a larger one is hit about once per entry and block, so there is nothing to merge and it is
// counted by 64-bit global atomic adds directly.  Integer sums: the tables do not depend on the order of arrival.
// The flush is what a hot table costs: every workgroup adds to the SAME few addresses, and adds to one address are
// served one after the other.  So a launch that keeps a histogram has at most kTarget workgroups, each walking every
// kTarget-th block with its histogram kept across them and flushed once; a launch without one has a workgroup per block.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"

#pragma clang fp contract(off)   // rounded products and a rounded sum, as the host formula

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;          // points of a workgroup's block, at most (16 per lane)
constexpr int kMinTile = 1024;       // ... and at least, where the block is made smaller to fill the chip
constexpr int kTarget = 1024;        // workgroups a launch aims at (4 per CU)
constexpr int kBatch = 4;            // 16-byte loads in flight per lane
constexpr int kLdsEntries = 4096;    // a table of at most this many entries is counted in LDS
constexpr int kInvalid = 255;

typedef double dvec2 __attribute__((ext_vector_type(2)));

struct StatesArgs {
  const dvec2* pts;             // S rows of nf points, ldp apart
  int64_t S, ldp, blocks;       // blocks: of `shots` shots each, the last one shorter
  const dvec2* centres;         // [nf][KT], NaN padded
  uint8_t* labels;              // null: none
  int64_t ldl;
  long long* words;             // null: none
  unsigned long long* counts;   // null: none
  unsigned long long* joint;    // null: none
  int64_t phase;                // first mod steps
  unsigned steps, bins;         // bins of joint per step, 2^(nf b) + 1
  unsigned nc, nj;              // entries of counts / joint kept in LDS (0: counted in global memory)
  int nf, K, bits, shots;       // shots: of a workgroup's block
};

// one more of table entry `idx`: in the LDS histogram where there is one, else in the caller's table
__device__ __forceinline__ void count_one(unsigned* __restrict__ hist, unsigned in_lds,
                                          unsigned long long* __restrict__ table, unsigned idx) {
  if (in_lds)
    atomicAdd(hist + idx, 1u);
  else
    atomicAdd(table + idx, 1ull);
}

__device__ __forceinline__ void flush(const unsigned* __restrict__ hist, unsigned entries,
                                      unsigned long long* __restrict__ table) {
  for (unsigned e = threadIdx.x; e < entries; e += kThreads) {
    const unsigned v = hist[e];
    if (v) atomicAdd(table + e, (unsigned long long)v);
  }
}

template <int KT>
__global__ void __launch_bounds__(kThreads) states_block(const StatesArgs a) {
  extern __shared__ unsigned lds[];   // [nc] counts, [nj] joint, then the block's labels (bytes) when words are formed
  unsigned* __restrict__ hc = lds;
  unsigned* __restrict__ hj = lds + a.nc;
  uint8_t* __restrict__ lab = reinterpret_cast<uint8_t*>(lds + a.nc + a.nj);
  const bool packed = a.words || a.joint;
  const unsigned hist = a.nc + a.nj;
  for (unsigned e = threadIdx.x; e < hist; e += kThreads) lds[e] = 0;
  if (hist) __syncthreads();
  const unsigned steps = a.steps;
  const int nf = a.nf, dq = kThreads / nf, dr = kThreads % nf;
  const unsigned dg = (unsigned)dq % steps;
  // A workgroup walks the blocks b, b + gridDim.x, ... and keeps its histograms across them: they are flushed once,
  // so a hot table entry takes one global atomic per WORKGROUP (at most kTarget of them), not one per block.
  for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
    const int64_t s0 = b * a.shots;
    const int shots = (int)min((int64_t)a.shots, a.S - s0);
    const int npts = shots * nf;
    const unsigned g0 = (unsigned)((a.phase + s0) % (int64_t)steps);   // the step of the block's first shot

    // the lane's point p = threadIdx.x + i * 256 as (shot, tone) and its step, advanced by additions
    int shot = (int)threadIdx.x / nf, tone = (int)threadIdx.x % nf;
    unsigned g = (g0 + (unsigned)shot) % steps;
    for (int p = threadIdx.x; p < npts; p += kBatch * kThreads) {
      dvec2 v[kBatch];
      int sh[kBatch], tn[kBatch];
      unsigned gs[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        sh[u] = shot; tn[u] = tone; gs[u] = g;
        if (p + u * kThreads < npts)
          v[u] = __builtin_nontemporal_load(a.pts + (s0 + shot) * a.ldp + tone);
        else
          v[u] = dvec2{0.0, 0.0};
        shot += dq; tone += dr; g += dg;
        if (tone >= nf) { tone -= nf; ++shot; ++g; }
        if (g >= steps) g -= steps;   // (g and dg are below steps: one subtraction)
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int pu = p + u * kThreads;
        if (pu >= npts) break;
        const dvec2* __restrict__ c = a.centres + (size_t)tn[u] * KT;
        double best = std::numeric_limits<double>::infinity();
        int w = kInvalid;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const dvec2 ck = c[k];
          const double re = v[u].x - ck.x, im = v[u].y - ck.y;
          const double d2 = re * re + im * im;
          if (d2 < best) { best = d2; w = k; }
        }
        if (a.labels) a.labels[(s0 + sh[u]) * a.ldl + tn[u]] = (uint8_t)w;
        if (packed) lab[pu] = (uint8_t)w;
        if (a.counts)
          count_one(hc, a.nc, a.counts, (gs[u] * (unsigned)nf + (unsigned)tn[u]) * (unsigned)(a.K + 1) +
                                            (unsigned)(w == kInvalid ? a.K : w));
      }
    }

    if (packed) {   // one lane per shot packs the labels the block has just produced
      __syncthreads();
      for (int t = threadIdx.x; t < shots; t += kThreads) {
        long long word = 0;
        bool bad = false;
        for (int j = 0; j < nf; ++j) {
          const unsigned l = lab[t * nf + j];
          bad = bad || l == kInvalid;
          word |= (long long)l << (j * a.bits);
        }
        if (a.words) a.words[s0 + t] = bad ? -1LL : word;
        if (a.joint)
          count_one(hj, a.nj, a.joint, ((g0 + (unsigned)t) % steps) * a.bins + (bad ? a.bins - 1u : (unsigned)word));
      }
      __syncthreads();   // (the next block writes its labels over these)
    }
  }
  if (hist) {
    __syncthreads();
    flush(hc, a.nc, a.counts);
    flush(hj, a.nj, a.joint);
  }
}

int bits_of(int K) { return K <= 2 ? 1 : K <= 4 ? 2 : 3; }

}  // namespace

struct wfk_states_plan {
  int nf = 0, K = 0, KT = 0, bits = 0;
  int64_t steps = 0;
  int forced = 0;               // WFK_STATES_COUNTERS when the plan was made: 1 lds, 2 global; 0: the rule
  DevBuf<char> centres;         // dvec2 [nf][KT]
  std::string name;
};

namespace {

// entries of counts and of joint (0: the plan has no joint table, nf b > 16)
int64_t counts_entries(const wfk_states_plan* p) { return p->steps * p->nf * (p->K + 1); }
int64_t joint_bins(const wfk_states_plan* p) { return p->nf * p->bits <= 16 ? (1LL << (p->nf * p->bits)) + 1 : 0; }

// The counter rule, a function of the plan's shape alone: how many of a table's entries live in LDS -- all of them
// when there are at most kLdsEntries, none otherwise.  WFK_STATES_COUNTERS = global takes every table to global
// memory; = lds asks for what the rule gives (a larger table has no room there).
unsigned lds_entries(const wfk_states_plan* p, int64_t entries) {
  return p->forced != 2 && entries > 0 && entries <= kLdsEntries ? (unsigned)entries : 0u;
}

// points of a workgroup's block for n_shots: kTile, halved down to kMinTile while the launch has fewer than kTarget
// workgroups
int tile_for(const wfk_states_plan* p, int64_t S) {
  if (S >= (int64_t)kTarget * kTile) return kTile;   // (so that the product below is small)
  int tile = kTile;
  while (tile > kMinTile && S * p->nf / tile < kTarget) tile /= 2;
  return tile;
}

}  // namespace

extern "C" {

int wfk_states_plan_destroy(wfk_states_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_states_plan_create(const double* centres_host, int32_t n_tones, int32_t n_states, int64_t steps,
                           wfk_states_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!centres_host) return wfk_fail(WFK_EINVAL, "state discriminator plan: null centres");
  if (n_tones < 1 || n_tones > WFK_STATES_MAX_TONES)
    return wfk_fail(WFK_EINVAL, "state discriminator plan: n_tones must lie in [1, 1024]");
  if (n_states < 2 || n_states > WFK_STATES_MAX_STATES)
    return wfk_fail(WFK_EINVAL, "state discriminator plan: n_states must lie in [2, 8]");
  if (steps < 1) return wfk_fail(WFK_EINVAL, "state discriminator plan: steps < 1");
  if (steps > 0x7fffffffLL / (n_tones * (n_states + 1)))
    return wfk_fail(WFK_EINVAL, "state discriminator plan: steps * n_tones * (n_states + 1) too large");
  const int KT = n_states <= 2 ? 2 : n_states <= 4 ? 4 : 8;
  std::vector<double> tab((size_t)n_tones * KT * 2, std::numeric_limits<double>::quiet_NaN());
  for (int32_t j = 0; j < n_tones; ++j) {
    bool any = false;
    for (int32_t k = 0; k < n_states; ++k) {
      const double re = centres_host[((size_t)j * n_states + k) * 2], im = centres_host[((size_t)j * n_states + k) * 2 + 1];
      tab[((size_t)j * KT + k) * 2] = re;
      tab[((size_t)j * KT + k) * 2 + 1] = im;
      any = any || (std::isfinite(re) && std::isfinite(im));
    }
    if (!any) return wfk_fail(WFK_EINVAL, "tone " + std::to_string(j) + ": no finite centre");
  }
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_states_plan> p(new wfk_states_plan());
  p->nf = n_tones; p->K = n_states; p->KT = KT; p->bits = bits_of(n_states);
  p->steps = steps;
  const char* forced = std::getenv("WFK_STATES_COUNTERS");
  p->forced = !forced ? 0 : !std::strcmp(forced, "lds") ? 1 : !std::strcmp(forced, "global") ? 2 : 0;
  if (!p->centres.upload(tab.data(), tab.size() * sizeof(double))) {
    (void)hipGetLastError();
    return wfk_fail(WFK_EHIP, "state discriminator plan: table upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the state discriminator plan");
}

int wfk_states_apply(wfk_states_plan* p, const void* points_dev, int64_t n_shots, int64_t points_stride, int64_t first,
                     uint8_t* labels_dev, int64_t labels_stride, int64_t* words_dev, int64_t* counts_dev,
                     int64_t* joint_dev, int accumulate, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  const char* stage = "state discriminator";
  if (n_shots < 0) return wfk_fail(WFK_EINVAL, "state discriminator: n_shots < 0");
  if (first < 0) return wfk_fail(WFK_EINVAL, "state discriminator: first < 0");
  if (!labels_dev && !words_dev && !counts_dev && !joint_dev)
    return wfk_fail(WFK_EINVAL, "state discriminator: no output (labels, words, counts and joint are all null)");
  if (words_dev && p->nf * p->bits > 62)
    return wfk_fail(WFK_EINVAL, "state discriminator: words need n_tones * bits <= 62, the plan has " +
                                    std::to_string(p->nf * p->bits));
  const int64_t bins = joint_bins(p);
  if (joint_dev && !bins)
    return wfk_fail(WFK_EINVAL, "state discriminator: joint needs n_tones * bits <= 16, the plan has " +
                                    std::to_string(p->nf * p->bits));
  if (joint_dev && p->steps > 0x7fffffffLL / bins)
    return wfk_fail(WFK_EINVAL, "state discriminator: steps * joint bins too large");
  if (n_shots > INT64_MAX / WFK_STATES_MAX_TONES) return wfk_fail(WFK_EINVAL, "state discriminator: n_shots too large");
  const int64_t nc = counts_entries(p), nj = p->steps * bins;
  // the sides there are, in the order of the call: each is held to the row rule against every one before it.  A block
  // of no shots has no points, labels or words to hold to it.
  RowSide sides[5];
  int n_sides = 0;
  if (n_shots > 0) {
    sides[n_sides++] = RowSide{"points", points_dev, n_shots, points_stride, p->nf, 16};
    if (labels_dev) sides[n_sides++] = RowSide{"labels", labels_dev, n_shots, labels_stride, p->nf, 1};
    if (words_dev) sides[n_sides++] = RowSide{"words", words_dev, 1, n_shots, n_shots, 8};
  }
  if (counts_dev) sides[n_sides++] = RowSide{"counts", counts_dev, 1, nc, nc, 8};
  if (joint_dev) sides[n_sides++] = RowSide{"joint", joint_dev, 1, nj, nj, 8};
  if (n_sides == 1)   // (one side alone stands in for its own input)
    if (const int rc = wfk_row_rule(stage, {sides[0]}, sides[0], kRowsAligned, wfk_fail)) return rc;
  for (int o = 1; o < n_sides; ++o)
    for (int i = 0; i < o; ++i)
      if (const int rc = wfk_row_rule(stage, {sides[i]}, sides[o], kRowsAligned | kRowsDisjoint, wfk_fail)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  if (!accumulate) {   // by a kernel on the stream: a captured memset node replays with another fill value
    if ((counts_dev && wfk_internal_zero_async(counts_dev, (size_t)nc * 8, st) != WFK_OK) ||
        (joint_dev && wfk_internal_zero_async(joint_dev, (size_t)nj * 8, st) != WFK_OK))
      return wfk_fail(WFK_EHIP, "state discriminator: zeroing the counts failed");
  }
  if (n_shots == 0) return WFK_OK;
  const int tile = tile_for(p, n_shots);
  StatesArgs a;
  a.pts = (const dvec2*)points_dev; a.S = n_shots; a.ldp = points_stride;
  a.centres = (const dvec2*)p->centres.get();
  a.labels = labels_dev; a.ldl = labels_stride;
  a.words = (long long*)words_dev;
  a.counts = (unsigned long long*)counts_dev;
  a.joint = (unsigned long long*)joint_dev;
  a.phase = first % p->steps;
  a.steps = (unsigned)p->steps; a.bins = (unsigned)bins;
  a.nc = counts_dev ? lds_entries(p, nc) : 0u;
  a.nj = joint_dev ? lds_entries(p, nj) : 0u;
  a.nf = p->nf; a.K = p->K; a.bits = p->bits;
  a.shots = tile / p->nf > 1 ? tile / p->nf : 1;
  a.blocks = (n_shots - 1) / a.shots + 1;
  // a launch that keeps a histogram has at most kTarget workgroups, each walking every kTarget-th block (one flush per
  // workgroup); without one a workgroup per block
  const int64_t blocks = (a.nc || a.nj) && a.blocks > kTarget ? kTarget : a.blocks;
  if (blocks > 0x7fffffffLL) return wfk_fail(WFK_EINVAL, "state discriminator: n_shots too large for one launch");
  const bool packed = words_dev || joint_dev;
  const size_t lds = (size_t)(a.nc + a.nj) * 4 + (packed ? (((size_t)a.shots * p->nf + 3) & ~size_t(3)) : 0);
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (p->KT == 2)
    hipLaunchKernelGGL(states_block<2>, grid, block, lds, st, a);
  else if (p->KT == 4)
    hipLaunchKernelGGL(states_block<4>, grid, block, lds, st, a);
  else
    hipLaunchKernelGGL(states_block<8>, grid, block, lds, st, a);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "state discriminator launch failed");
  return WFK_OK;
}

const char* wfk_states_kernel_name(const wfk_states_plan* p, int64_t n_shots) {
  if (!p) return "";
  wfk_states_plan* q = const_cast<wfk_states_plan*>(p);
  const int64_t bins = joint_bins(p);
  q->name = "states_block<" + std::to_string(p->KT) + "> tile=" + std::to_string(tile_for(p, n_shots > 0 ? n_shots : 0)) +
            " counts:" + (lds_entries(p, counts_entries(p)) ? "lds" : "global") + " joint:" +
            (!bins ? "none" : p->steps <= 0x7fffffffLL / bins && lds_entries(p, p->steps * bins) ? "lds" : "global");
  return q->name.c_str();
}

}  // extern "C"
