// wfk_bdemod.hip -- readout demodulation per time bin: out[s, w, j] = sum over k in bin w of x[s, k] * e[k, j], bin w =
// samples [start + w bin, start + (w + 1) bin), w = 0 .. W - 1, for real traces x (shots x >= N; float64, float32 or
// int16 ADC codes) and the complex matrix e (N x nf) of getFTMatrix: the IQ trajectory of every shot.  e keeps the global
// time axis, so the phases run on from bin to bin.  fp64 throughout; the product is demod_tile's (wfk_demod.hip), what
// is new is where the sums end.
//
// The plan holds the rows [start, start + W bin) of B = e as interleaved (re, im) doubles in HBM, in column blocks of NB
// tones ([ncb][kFront + W bin + kRear][NB] complex): zero columns past nf, kFront zero rows in front and kRear behind,
// so a launch never reads outside it.  Every used entry of e is finite (refused at creation otherwise): a position the
// kernel fills with a zero sample multiplies a finite number, never 0 * inf.
//
// bdemod_tile<T, NB>: lane = shot.  A workgroup of 4 waves owns 64 shots, one column block (grid.z) and one group of
// consecutive bins (grid.y); its waves share the group's bins in four consecutive runs, each bin whole.  A bin's sums
// live in ONE wave's registers: no reduction across waves, no barrier between them, no workspace, no atomics.  A wave
// walks the samples of its run as one stream of chunks, demod_tile's walk: 128 B of each of the 64 rows (16 / 32 / 64
// samples), every lane loading 8 of the 16-B segments (8 lanes per row, coalesced), parked in the wave's own LDS tile
// (row pitch 144 B), read back by the lane that owns the row, widened and run through 2NB FMAs per sample against B's
// row, the same for all lanes (scalar loads); the next chunk's loads are in flight during the FMAs.  When the sample
// that ends a bin is done (a wave-uniform test), the lane stores its NB complex sums and clears them.
// Bin edges: the chunk grid is laid from the 16-B boundary at or below the run's first sample (of row 0; rows whose
// stride is a multiple of 16 B share it), so the segments inside the run are aligned loads whatever `start` and `bin`
// are; the samples in front of the run in the first segment and behind it in the last are zeros in the register --
// never loaded -- and those two segments, like every segment of a row off that boundary, are read element by element.
// Every row offset is 64-bit: s * ldx, s * out_stride + w * nf.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>

#include "wfk.h"
#include "wfk_host.h"

namespace {

constexpr int kWaves = 4;               // waves per workgroup
constexpr int kRows = 64;               // shots per workgroup (lane = shot)
constexpr int kRowBytes = 128;          // bytes of one trace row per chunk
constexpr int kSeg = kRowBytes / 16;    // 16-B segments per row and chunk
constexpr int kPitch = kRowBytes + 16;  // LDS row pitch
constexpr int kLoads = kRows * kSeg / 64;  // 16-B loads per lane and chunk
constexpr int kTarget = 1024;           // workgroups a launch aims at (4 per CU)
constexpr int kMinBins = 4;             // bins a group keeps where W allows (one per wave)
constexpr int kFront = 8;               // zero rows of B in front: a chunk grid starts up to 7 samples before its run
constexpr int kRear = 72;               // ... and behind: the last chunk ends less than one chunk after it

// First sample of a 16-B segment as fp64, and the segment shifted down by one sample (see wfk_demod.hip: taking the
// samples one at a time keeps the sample loop rollable).
template <typename T>
__device__ __forceinline__ double first(const uint4 v);
template <>
__device__ __forceinline__ double first<double>(const uint4 v) { return __hiloint2double((int)v.y, (int)v.x); }
template <>
__device__ __forceinline__ double first<float>(const uint4 v) { return (double)__uint_as_float(v.x); }
template <>
__device__ __forceinline__ double first<int16_t>(const uint4 v) { return (double)(int)(short)(v.x & 0xffffu); }

template <typename T>
__device__ __forceinline__ uint4 next(const uint4 v) {
  if (sizeof(T) == 8) return make_uint4(v.z, v.w, 0, 0);
  if (sizeof(T) == 4) return make_uint4(v.y, v.z, v.w, 0);
  return make_uint4(__funnelshift_r(v.x, v.y, 16), __funnelshift_r(v.y, v.z, 16),
                    __funnelshift_r(v.z, v.w, 16), v.w >> 16);
}

// The 16-B segment of one row that starts at sample k (row: the row's first sample); zeros outside [lo, hi), which are
// not read.  A segment inside [lo, hi) at a 16-B boundary is one load, any other is read element by element.
template <typename T>
__device__ __forceinline__ uint4 load_seg(const T* __restrict__ row, int64_t k, int64_t lo, int64_t hi) {
  constexpr int E = 16 / sizeof(T);
  if (k >= lo && k + E <= hi && ((uintptr_t)(row + k) & 15) == 0) return *(const uint4*)(row + k);
  union {
    uint4 v;
    T e[E];
  } u;
#pragma unroll
  for (int i = 0; i < E; ++i) u.e[i] = k + i >= lo && k + i < hi ? row[k + i] : (T)0;
  return u.v;
}

// the lanes of one wave meet: what they wrote to the wave's LDS tile is there for the others, what they read is read
// (a wave's LDS instructions run in order: this costs no instruction, it keeps the compiler from moving them)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef const __attribute__((address_space(4))) double* const_row;

template <typename T, int NB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NB <= 8 ? 4 : NB <= 16 ? 3 : 2)))
    bdemod_tile(const T* __restrict__ X, int64_t S, int64_t ldx, int phase, const double* __restrict__ B,
                int64_t brows, int64_t start, int64_t bin, int32_t W, int32_t bins_per_group,
                double* __restrict__ out, int64_t out_stride, int32_t nf) {
  constexpr int E = 16 / sizeof(T);
  constexpr int KC = kRowBytes / sizeof(T);
  constexpr int NC = 2 * NB;
  constexpr int UE = NB <= 4 ? (E < 4 ? E : 4) : 1;   // samples per unrolled step (B rows in scalar registers)
  constexpr bool kClampRows = NB >= 16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWaves * kRows * kPitch];

  // the wave index is wave-uniform: readfirstlane lets the compiler keep B's row addresses (and so B's loads), the
  // sample counter and the bin edge in scalar registers
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s0 = (int64_t)blockIdx.x * kRows;
  // the group's bins [g0, g1) and this wave's run of them [w, w_end)   (bins * nf < 2^31: 32 bits hold a bin)
  const int g0 = (int)blockIdx.y * bins_per_group, g1 = min(W, g0 + bins_per_group);
  const int per_wave = (g1 - g0 + kWaves - 1) / kWaves;
  int w = g0 + wv * per_wave;
  const int w_end = min(g1, w + per_wave);
  if (w >= w_end) return;   // a wave without a bin (W < 4): the kernel has no workgroup barrier
  // the run's samples [ka, kb); the chunk grid starts at kc <= ka, a 16-B boundary of row 0
  const int64_t ka = start + w * bin, kb = start + w_end * bin;
  int64_t kc = ka - (ka + phase) % E;
  // B's row of sample kc; it runs on from chunk to chunk (every chunk but the last is walked to its end).  Read through
  // the constant address space: the plan wrote B before any launch, and only so do the rows stay SCALAR loads -- with
  // the stores to `out` inside the loop the compiler otherwise reads them with vector loads, eight per sample and lane.
  const_row b = (const_row)(B + ((int64_t)blockIdx.z * brows + (kc - start + kFront)) * NC);
  unsigned char* tile = lds + wv * (kRows * kPitch);
  const int col0 = blockIdx.z * NB;
  const int64_t s_own = s0 + lane;

  double acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.0;

  uint4 buf[kLoads];
  auto fetch = [&](int64_t from) {   // the chunk that starts at sample `from`; nothing at or behind kb
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int idx = i * 64 + lane, r = idx / kSeg, q = idx % kSeg;
      // A row behind the last shot is not read: one lane mask per load slot, eight scalar register pairs kept across
      // the loop.  NB = 32 has no room for them next to B's rows (they spill into VGPR lanes): there such a row reads
      // the last shot's instead, and its sums are not stored.  (The narrower builds take MORE vector registers that
      // way -- int16, NB = 8 goes past 128 -- so they keep the masks.)
      const int64_t s = kClampRows ? min(s0 + r, S - 1) : s0 + r, k = from + q * E;
      buf[i] = make_uint4(0, 0, 0, 0);
      if (s < S && k < kb) buf[i] = load_seg<T>(X + s * ldx, k, ka, kb);
    }
  };

  int64_t edge = ka + bin;   // one past the last sample of bin w
  // the 1-based place in the chunk at kc of the sample that ends bin w; 0: not in this chunk (or no bin is left)
  auto place = [&]() { return w < w_end && edge - kc <= KC ? (int)(edge - kc) : 0; };
  fetch(kc);
  for (; kc < kb; kc += KC) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int idx = i * 64 + lane, r = idx / kSeg, q = idx % kSeg;
      *(uint4*)(tile + r * kPitch + q * 16) = buf[i];
    }
    wave_sync();
    fetch(kc + KC);
    const int nseg = kb - kc < KC ? (int)((kb - kc + E - 1) / E) : kSeg;
    const unsigned char* row = tile + lane * kPitch;
    int at = 0, ends = place();
    // bin w is complete (wave-uniform): the lane stores its sums and clears them
    auto finish_bin = [&]() {
      if (s_own < S) {
        double2* dst = (double2*)out + s_own * out_stride + (int64_t)w * nf + col0;
#pragma unroll
        for (int j = 0; j < NB; ++j)
          if (col0 + j < nf) dst[j] = make_double2(acc[2 * j], acc[2 * j + 1]);
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) acc[j] = 0.0;
      ++w;
      edge += bin;
      ends = place();
    };
#pragma unroll 1
    for (int q = 0; q < nseg; ++q) {
      uint4 v = *(const uint4*)(row + q * 16);
      if constexpr (UE > 1) {
        // narrow column blocks: UE samples in one straight run where no bin ends among them, so that their rows of B
        // are fetched together -- one wait per UE samples, which is what a launch of few waves is bound by
#pragma unroll
        for (int e0 = 0; e0 < E; e0 += UE) {
          if (ends == 0 || ends > at + UE) {
#pragma unroll
            for (int u = 0; u < UE; ++u) {
              const double x = first<T>(v);
              v = next<T>(v);
#pragma unroll
              for (int j = 0; j < NC; ++j) acc[j] = fma(x, b[u * NC + j], acc[j]);
            }
            b += UE * NC;
            at += UE;
          } else {
#pragma unroll 1
            for (int u = 0; u < UE; ++u, b += NC) {
              const double x = first<T>(v);
              v = next<T>(v);
#pragma unroll
              for (int j = 0; j < NC; ++j) acc[j] = fma(x, b[j], acc[j]);
              if (++at == ends) finish_bin();
            }
          }
        }
      } else {
#pragma unroll 1
        for (int e = 0; e < E; ++e, b += NC) {
          const double x = first<T>(v);
          v = next<T>(v);
#pragma unroll
          for (int j0 = 0; j0 < NC; j0 += 16) {   // 16 columns of B at a time in scalar registers
#pragma unroll
            for (int j = j0; j < j0 + 16 && j < NC; ++j) acc[j] = fma(x, b[j], acc[j]);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (++at == ends) finish_bin();
        }
      }
    }
    wave_sync();
  }
}

int bucket_of(int32_t nf) { return nf <= 4 ? 4 : nf <= 8 ? 8 : nf <= 16 ? 16 : 32; }

int elem_bytes(int kind) { return kind == WFK_IN_F64 ? 8 : kind == WFK_IN_F32 ? 4 : 2; }

const char* type_name(int kind) {
  return kind == WFK_IN_F64 ? "double" : kind == WFK_IN_F32 ? "float" : "short";
}

template <typename T>
int launch_t(int nb, dim3 grid, hipStream_t st, const T* X, int64_t S, int64_t ldx, const double* B, int64_t brows,
             int64_t start, int64_t bin, int32_t W, int32_t bpg, double* out, int64_t ostride, int32_t nf) {
  // elements from the 16-B boundary below row 0 to its first sample
  const int phase = (int)(((uintptr_t)X & 15) / sizeof(T));
  switch (nb) {
#define WFK_BDEMOD_CASE(NBV)                                                                                  \
  case NBV:                                                                                                   \
    hipLaunchKernelGGL((bdemod_tile<T, NBV>), grid, dim3(256), 0, st, X, S, ldx, phase, B, brows, start, bin, \
                       W, bpg, out, ostride, nf);                                                             \
    break;
    WFK_BDEMOD_CASE(4)
    WFK_BDEMOD_CASE(8)
    WFK_BDEMOD_CASE(16)
    WFK_BDEMOD_CASE(32)
#undef WFK_BDEMOD_CASE
    default:
      return wfk_fail(WFK_EINVAL, "binned demodulator: bad column bucket");
  }
  return WFK_OK;
}

}  // namespace

struct wfk_bdemod_plan {
  int64_t n = 0, start = 0, bin = 0, bins = 0, brows = 0;
  int32_t nf = 0, nb = 0, ncb = 0;
  int kind = 0;
  DevBuf<double> B;        // [ncb][brows][nb] complex: the rows [start, start + bins * bin) between zero rows
  std::string name;
};

extern "C" {

// The bin-group rule, a function of (n_shots, n_freq, bins) alone: with `blocks` = ceil(n_shots / 64) * column blocks,
// max(1, 1024 / blocks) groups, at most max(1, bins / 4) of them (a group keeps four bins, one per wave, where bins
// allows), and then as few as give every group ceil(bins / groups) bins but the last.
int64_t wfk_bdemod_bin_groups(int64_t n_shots, int32_t n_freq, int64_t bins) {
  if (n_shots < 1 || n_freq < 1 || bins < 1) return 0;
  const int64_t shot_blocks = (n_shots - 1) / kRows + 1;
  const int64_t ncb = (n_freq - 1) / bucket_of(n_freq) + 1;
  const int64_t want = shot_blocks >= kTarget ? 1 : kTarget / (shot_blocks * ncb) > 1 ? kTarget / (shot_blocks * ncb) : 1;
  const int64_t cap = bins / kMinBins > 1 ? bins / kMinBins : 1;
  const int64_t groups = want < cap ? want : cap;
  const int64_t per_group = (bins - 1) / groups + 1;
  return (bins - 1) / per_group + 1;
}

int wfk_bdemod_plan_destroy(wfk_bdemod_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_bdemod_plan_create(const double* e_host, int64_t n_points, int32_t n_freq, int in_kind, int64_t start,
                           int64_t bin, int64_t bins, wfk_bdemod_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!e_host) return wfk_fail(WFK_EINVAL, "binned demodulator plan: null matrix");
  if (n_points < 1 || n_freq < 1 || n_freq > 65535 * 32)
    return wfk_fail(WFK_EINVAL, "binned demodulator plan: bad shape (n_points >= 1, 1 <= n_freq <= 2097120)");
  if (bin < 1) return wfk_fail(WFK_EINVAL, "binned demodulator plan: bin < 1");
  if (bins < 1) return wfk_fail(WFK_EINVAL, "binned demodulator plan: bins < 1");
  if (start < 0) return wfk_fail(WFK_EINVAL, "binned demodulator plan: start < 0");
  if (start > n_points || bin > n_points - start || bins > (n_points - start) / bin)   // (no product: no overflow)
    return wfk_fail(WFK_EINVAL, "binned demodulator plan: start + bins * bin > n_points");
  if (bins > 0x7fffffffLL / n_freq)
    return wfk_fail(WFK_EINVAL, "binned demodulator plan: bins * n_freq exceeds 2^31 - 1");
  if (in_kind != WFK_IN_F64 && in_kind != WFK_IN_F32 && in_kind != WFK_IN_I16)
    return wfk_fail(WFK_EINVAL, "in_kind must be WFK_IN_F64, WFK_IN_F32 or WFK_IN_I16");
  const int64_t used = bins * bin;
  for (int64_t k = start; k < start + used; ++k)
    for (int32_t j = 0; j < n_freq; ++j) {
      const double* z = e_host + ((size_t)k * n_freq + j) * 2;
      if (!std::isfinite(z[0]) || !std::isfinite(z[1]))
        return wfk_fail(WFK_EINVAL, "binned demodulator plan: e[" + std::to_string(k) + ", " + std::to_string(j) +
                                        "] is not finite");
    }
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_bdemod_plan> p(new wfk_bdemod_plan());
  p->n = n_points;
  p->nf = n_freq;
  p->kind = in_kind;
  p->start = start;
  p->bin = bin;
  p->bins = bins;
  p->nb = bucket_of(n_freq);
  p->ncb = (n_freq + p->nb - 1) / p->nb;
  p->brows = kFront + used + kRear;
  const size_t block_bytes = (size_t)p->brows * p->nb * 16, bbytes = (size_t)p->ncb * block_bytes;
  bool ok = p->B.alloc(bbytes) && hipMemset(p->B.get(), 0, bbytes) == hipSuccess;
  // column block cb of the used rows of e (point-major rows of nf complex) -> rows of nb complex behind kFront zero rows
  for (int32_t cb = 0; ok && cb < p->ncb; ++cb) {
    const int32_t w = n_freq - cb * p->nb < p->nb ? n_freq - cb * p->nb : p->nb;
    ok = hipMemcpy2D((char*)p->B.get() + (size_t)cb * block_bytes + (size_t)kFront * p->nb * 16, (size_t)p->nb * 16,
                     e_host + ((size_t)start * n_freq + (size_t)cb * p->nb) * 2, (size_t)n_freq * 16, (size_t)w * 16,
                     (size_t)used, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "binned demodulator plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the binned demodulator plan");
}

int wfk_bdemod_apply(wfk_bdemod_plan* p, const void* traces_dev, int64_t n_shots, int64_t trace_stride,
                     void* out_dev, int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (n_shots < 0) return wfk_fail(WFK_EINVAL, "binned demodulator: n_shots < 0");
  if (n_shots == 0) return WFK_OK;
  // a lone trace's stride is read by no kernel
  if (const int rc = wfk_row_rule("binned demodulator",
                                  {{"traces", traces_dev, n_shots, trace_stride, p->n, (size_t)elem_bytes(p->kind), false}},
                                  {"out", out_dev, n_shots, out_stride, p->bins * p->nf, 16},
                                  kRowsAligned | kRowsDisjoint, wfk_fail))
    return rc;
  const int64_t nsb = (n_shots + kRows - 1) / kRows;
  if (nsb > 0x7fffffff) return wfk_fail(WFK_EINVAL, "binned demodulator: too many shots");
  const int64_t groups = wfk_bdemod_bin_groups(n_shots, p->nf, p->bins);
  const int64_t bpg = (p->bins + groups - 1) / groups;
  const dim3 grid((unsigned)nsb, (unsigned)groups, (unsigned)p->ncb);
  hipStream_t st = (hipStream_t)hip_stream;
  int rc;
  if (p->kind == WFK_IN_F64)
    rc = launch_t<double>(p->nb, grid, st, (const double*)traces_dev, n_shots, trace_stride, p->B.get(), p->brows,
                          p->start, p->bin, (int32_t)p->bins, (int32_t)bpg, (double*)out_dev, out_stride, p->nf);
  else if (p->kind == WFK_IN_F32)
    rc = launch_t<float>(p->nb, grid, st, (const float*)traces_dev, n_shots, trace_stride, p->B.get(), p->brows,
                         p->start, p->bin, (int32_t)p->bins, (int32_t)bpg, (double*)out_dev, out_stride, p->nf);
  else
    rc = launch_t<int16_t>(p->nb, grid, st, (const int16_t*)traces_dev, n_shots, trace_stride, p->B.get(), p->brows,
                           p->start, p->bin, (int32_t)p->bins, (int32_t)bpg, (double*)out_dev, out_stride, p->nf);
  if (rc != WFK_OK) return rc;
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "binned demodulator launch failed");
  return WFK_OK;
}

const char* wfk_bdemod_kernel_name(const wfk_bdemod_plan* p, int64_t n_shots) {
  if (!p) return "";
  wfk_bdemod_plan* q = const_cast<wfk_bdemod_plan*>(p);
  q->name = std::string("bdemod_tile<") + type_name(p->kind) + "," + std::to_string(p->nb) +
            "> groups=" + std::to_string(wfk_bdemod_bin_groups(n_shots, p->nf, p->bins));
  return q->name.c_str();
}

}  // extern "C"
