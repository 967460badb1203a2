// wfk_demod.hip -- readout demodulation: out[s, j] = sum_k x[s, k] * e[k, j]
// for real traces x (shots x N; float64, float32 or int16 ADC codes) and a complex matrix e (N x nf),
// i.e. `traces @ getFTMatrix(...)` of the reference's utils.py:35-84 as one device product.
//
// Viewed as C[S x 2nf] = X[S x N] * B[N x 2nf] with B = e as interleaved (re, im) doubles.  The plan
// holds B in HBM padded to column blocks of NB tones ([ncb][npad][NB] complex, zero columns and
// zero rows past N), so a launch never reads past B and a block's 2NB columns are compile-time.
//
// demod_tile<T, NB>: lane = shot.  A workgroup owns 64 shots and a range of chunks of N; its four
// waves take the chunks round robin.  A chunk is 128 B of every one of the 64 rows (16 / 32 / 64
// samples): each lane loads 8 of its 16-B segments (8 lanes per row, coalesced), the wave parks them
// in its own LDS tile (row pitch 144 B: the 16 lanes of a ds_read_b128 group hit 16 distinct slots),
// and each lane then reads its own row back, widens to fp64 in registers and runs 2NB fp64 FMAs per
// sample against B's row k, which is the same for every lane (scalar loads: B is read once per wave
// per sample and reused across the 64 shots).  The next chunk's global loads are in flight while the
// current one is computed.  The four waves' sums are added in a fixed order through LDS.
//
// Small S (fewer than ~512 workgroups from shots x column blocks) splits N across workgroups
// (grid.y).  Each split writes its 64 x NB partial sums into the plan's workspace and demod_reduce
// adds the splits in a fixed order (per-lane strided sums, then a fixed xor butterfly): no float
// atomics, the result is bitwise reproducible for a given shape.
#include <hip/hip_runtime.h>

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
constexpr int kTarget = 1024;           // workgroups a split launch aims at (4 per CU)

// First sample of a 16-B segment as fp64, and the segment shifted down by one sample.  Taking the
// samples one at a time keeps the sample loop rollable, so the compiler fetches B's rows a few at a
// time instead of hoisting the whole segment's rows into scalar registers (which spills them).
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

// One 16-B segment of row s starting at sample k; zeros past N.  Rows may start at any element
// (windows x[:, w0:w0+N]): unaligned or partial segments are read element by element.
template <typename T>
__device__ __forceinline__ uint4 load_seg(const T* __restrict__ p, int64_t k, int64_t N) {
  constexpr int E = 16 / sizeof(T);
  if (k + E <= N && ((uintptr_t)p & 15) == 0) return *(const uint4*)p;
  union {
    uint4 v;
    T e[E];
  } u;
#pragma unroll
  for (int i = 0; i < E; ++i) u.e[i] = k + i < N ? p[i] : (T)0;
  return u.v;
}

template <typename T, int NB>
__global__ void __launch_bounds__(256)
    demod_tile(const T* __restrict__ X, int64_t S, int64_t N, int64_t ldx,
               const double* __restrict__ B, int64_t npad, int64_t chunks_per_split,
               double* __restrict__ out, int64_t out_stride, int32_t nf,
               double* __restrict__ part, int64_t spad) {
  constexpr int E = 16 / sizeof(T);
  constexpr int KC = kRowBytes / sizeof(T);
  constexpr int NC = 2 * NB;
  constexpr int UE = NB <= 4 ? 2 : 1;   // samples per unrolled step (B rows in scalar registers)
  __shared__ __attribute__((aligned(16))) unsigned char lds[kWaves * kRows * kPitch];

  // the wave index is wave-uniform: readfirstlane lets the compiler keep B's row addresses (and so B's
  // loads) in scalar registers
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t s0 = (int64_t)blockIdx.x * kRows;
  const int64_t nch = (N + KC - 1) / KC;
  const int64_t c_begin = (int64_t)blockIdx.y * chunks_per_split;
  const int64_t c_end = min(nch, c_begin + chunks_per_split);
  const int64_t iters = c_end > c_begin ? (c_end - c_begin + kWaves - 1) / kWaves : 0;
  const double* __restrict__ Bb = B + (int64_t)blockIdx.z * npad * NC;
  unsigned char* tile = lds + w * (kRows * kPitch);

  double acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.0;

  uint4 buf[kLoads];
  auto fetch = [&](int64_t c) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int idx = i * 64 + lane, r = idx / kSeg, q = idx % kSeg;
      const int64_t s = s0 + r, k = c * KC + q * E;
      buf[i] = make_uint4(0, 0, 0, 0);
      if (c < c_end && s < S) buf[i] = load_seg<T>(X + s * ldx + k, k, N);
    }
  };

  int64_t c = c_begin + w;
  fetch(c);
  for (int64_t it = 0; it < iters; ++it, c += kWaves) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int idx = i * 64 + lane, r = idx / kSeg, q = idx % kSeg;
      *(uint4*)(tile + r * kPitch + q * 16) = buf[i];
    }
    __syncthreads();
    fetch(c + kWaves);
    if (c < c_end) {
      const unsigned char* row = tile + lane * kPitch;
      const double* __restrict__ Bc = Bb + c * KC * NC;
#pragma unroll 1
      for (int q = 0; q < kSeg; ++q) {
        uint4 v = *(const uint4*)(row + q * 16);
        const double* __restrict__ b = Bc + q * E * NC;
#pragma unroll UE
        for (int e = 0; e < E; ++e, b += NC) {
          const double x = first<T>(v);
          v = next<T>(v);
#pragma unroll
          for (int j0 = 0; j0 < NC; j0 += 16) {   // 16 columns of B at a time in scalar registers
#pragma unroll
            for (int j = j0; j < j0 + 16 && j < NC; ++j) acc[j] = fma(x, b[j], acc[j]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    __syncthreads();
  }

  // waves 1..3 hand their sums to wave 0, PC columns at a time; wave 0 adds them in wave order
  constexpr int PC = NC < 16 ? NC : 16;
  double* red = (double*)lds;   // [3][PC][64]: 24 KiB at most
#pragma unroll
  for (int p0 = 0; p0 < NC; p0 += PC) {
    if (w > 0) {
#pragma unroll
      for (int j = 0; j < PC; ++j) red[((w - 1) * PC + j) * 64 + lane] = acc[p0 + j];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int ww = 0; ww < kWaves - 1; ++ww)
#pragma unroll
        for (int j = 0; j < PC; ++j) acc[p0 + j] += red[(ww * PC + j) * 64 + lane];
    }
    __syncthreads();
  }
  const int64_t s = s0 + lane;
  if (w != 0 || s >= S) return;
  const int col0 = blockIdx.z * NB;
  if (part) {   // split: padded partials [split][spad][ncb * NB] complex
    double2* dst = (double2*)part + ((int64_t)blockIdx.y * spad + s) * ((int64_t)gridDim.z * NB) + col0;
#pragma unroll
    for (int j = 0; j < NB; ++j) dst[j] = make_double2(acc[2 * j], acc[2 * j + 1]);
  } else {
    double2* dst = (double2*)out + s * out_stride + col0;
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (col0 + j < nf) dst[j] = make_double2(acc[2 * j], acc[2 * j + 1]);
  }
}

// out[s, j] = sum over splits of part[split][s][j], one wave per output, fixed order
__global__ void __launch_bounds__(256)
    demod_reduce(const double2* __restrict__ part, int64_t n_split, int64_t S, int64_t spad,
                 int64_t ncolpad, int32_t nf, double2* __restrict__ out, int64_t out_stride) {
  const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= S * nf) return;   // uniform per wave
  const int64_t s = o / nf, j = o % nf;
  double re = 0.0, im = 0.0;
  for (int64_t k = lane; k < n_split; k += 64) {
    const double2 v = part[(k * spad + s) * ncolpad + j];
    re += v.x;
    im += v.y;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    re += __shfl_xor(re, off, 64);
    im += __shfl_xor(im, off, 64);
  }
  if (lane == 0) out[s * out_stride + j] = make_double2(re, im);
}

int bucket_of(int32_t nf) { return nf <= 4 ? 4 : nf <= 8 ? 8 : nf <= 16 ? 16 : 32; }

int elem_bytes(int kind) { return kind == WFK_IN_F64 ? 8 : kind == WFK_IN_F32 ? 4 : 2; }

const char* type_name(int kind) {
  return kind == WFK_IN_F64 ? "double" : kind == WFK_IN_F32 ? "float" : "short";
}

template <typename T>
int launch_t(int nb, dim3 grid, hipStream_t st, const T* X, int64_t S, int64_t N, int64_t ldx,
             const double* B, int64_t npad, int64_t cps, double* out, int64_t ostride, int32_t nf,
             double* part, int64_t spad) {
  switch (nb) {
#define WFK_DEMOD_CASE(NBV)                                                                        \
  case NBV:                                                                                        \
    hipLaunchKernelGGL((demod_tile<T, NBV>), grid, dim3(256), 0, st, X, S, N, ldx, B, npad, cps, \
                       out, ostride, nf, part, spad);                                              \
    break;
    WFK_DEMOD_CASE(4)
    WFK_DEMOD_CASE(8)
    WFK_DEMOD_CASE(16)
    WFK_DEMOD_CASE(32)
#undef WFK_DEMOD_CASE
    default:
      return wfk_fail(WFK_EINVAL, "bad column bucket");
  }
  return WFK_OK;
}

}  // namespace

struct wfk_demod_plan {
  int64_t n = 0, npad = 0, nch = 0;
  int32_t nf = 0, nb = 0, ncb = 0;
  int kind = 0;
  DevBuf<double> B;        // [ncb][npad][nb] complex
  DevBuf<double> ws;       // split partials: kTarget * 64 * nb complex
  std::string name;
};

namespace {
// splits of N for a launch of S shots: 1 when shots x column blocks fill the chip, else enough
// workgroups to reach kTarget (each wave keeps >= 2 chunks); the workspace holds kTarget * 64 * nb
int64_t splits_for(const wfk_demod_plan* p, int64_t S) {
  const int64_t nblk = (S + kRows - 1) / kRows * p->ncb;
  if (!p->ws || nblk == 0) return 1;
  int64_t ks = kTarget / nblk;
  const int64_t by_len = p->nch / (2 * kWaves);
  if (ks > by_len) ks = by_len;
  return ks > 1 ? ks : 1;
}
}  // namespace

extern "C" {

int wfk_demod_plan_destroy(wfk_demod_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_demod_plan_create(const double* e_host, int64_t n_points, int32_t n_freq, int in_kind,
                          wfk_demod_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!e_host) return wfk_fail(WFK_EINVAL, "null matrix");
  if (n_points < 1 || n_freq < 1 || n_freq > 65535 * 32)
    return wfk_fail(WFK_EINVAL, "bad demodulator shape (n_points >= 1, 1 <= n_freq <= 2097120)");
  if (in_kind != WFK_IN_F64 && in_kind != WFK_IN_F32 && in_kind != WFK_IN_I16)
    return wfk_fail(WFK_EINVAL, "in_kind must be WFK_IN_F64, WFK_IN_F32 or WFK_IN_I16");
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_demod_plan> p(new wfk_demod_plan());
  p->n = n_points;
  p->nf = n_freq;
  p->kind = in_kind;
  p->nb = bucket_of(n_freq);
  p->ncb = (n_freq + p->nb - 1) / p->nb;
  const int64_t kc = kRowBytes / elem_bytes(in_kind);
  p->nch = (n_points + kc - 1) / kc;
  p->npad = p->nch * kc;
  const size_t bbytes = (size_t)p->ncb * p->npad * p->nb * 16;
  bool ok = p->B.alloc(bbytes) && hipMemset(p->B.get(), 0, bbytes) == hipSuccess;
  // column block cb of e (point-major rows of nf complex) -> rows of nb complex
  for (int32_t cb = 0; ok && cb < p->ncb; ++cb) {
    const int32_t w = n_freq - cb * p->nb < p->nb ? n_freq - cb * p->nb : p->nb;
    ok = hipMemcpy2D((char*)p->B.get() + (size_t)cb * p->npad * p->nb * 16, (size_t)p->nb * 16,
                     e_host + (size_t)cb * p->nb * 2, (size_t)n_freq * 16, (size_t)w * 16,
                     (size_t)n_points, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (ok && p->nch >= 4 * kWaves)
    ok = p->ws.alloc((size_t)kTarget * kRows * p->nb * 16);
  if (!ok) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "demodulator plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the demodulator plan");
}

int wfk_demod_apply(wfk_demod_plan* p, const void* traces_dev, int64_t n_shots, int64_t trace_stride,
                    void* out_dev, int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (n_shots < 0) return wfk_fail(WFK_EINVAL, "n_shots < 0");
  if (n_shots == 0) return WFK_OK;
  if (!traces_dev || !out_dev) return wfk_fail(WFK_EINVAL, "null argument");
  if (trace_stride < p->n) return wfk_fail(WFK_EINVAL, "trace_stride < n_points");
  if (out_stride < p->nf) return wfk_fail(WFK_EINVAL, "out_stride < n_freq");
  if (((uintptr_t)out_dev & 15) != 0) return wfk_fail(WFK_EINVAL, "out must be 16-byte aligned");
  if (((uintptr_t)traces_dev % elem_bytes(p->kind)) != 0)
    return wfk_fail(WFK_EINVAL, "traces not aligned to their element size");
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t ks = splits_for(p, n_shots);
  const int64_t nsb = (n_shots + kRows - 1) / kRows;
  const int64_t cps = (p->nch + ks - 1) / ks;
  const int64_t spad = nsb * kRows;
  if (nsb > 0x7fffffff) return wfk_fail(WFK_EINVAL, "too many shots");
  const dim3 grid((unsigned)nsb, (unsigned)ks, (unsigned)p->ncb);
  double* part = ks > 1 ? p->ws.get() : nullptr;
  int rc;
  if (p->kind == WFK_IN_F64)
    rc = launch_t<double>(p->nb, grid, st, (const double*)traces_dev, n_shots, p->n, trace_stride, p->B.get(),
                          p->npad, cps, (double*)out_dev, out_stride, p->nf, part, spad);
  else if (p->kind == WFK_IN_F32)
    rc = launch_t<float>(p->nb, grid, st, (const float*)traces_dev, n_shots, p->n, trace_stride, p->B.get(),
                         p->npad, cps, (double*)out_dev, out_stride, p->nf, part, spad);
  else
    rc = launch_t<int16_t>(p->nb, grid, st, (const int16_t*)traces_dev, n_shots, p->n, trace_stride, p->B.get(),
                           p->npad, cps, (double*)out_dev, out_stride, p->nf, part, spad);
  if (rc != WFK_OK) return rc;
  if (ks > 1) {
    const int64_t nout = n_shots * p->nf;
    hipLaunchKernelGGL(demod_reduce, dim3((unsigned)((nout + 3) / 4)), dim3(256), 0, st,
                       (const double2*)p->ws.get(), ks, n_shots, spad, (int64_t)p->ncb * p->nb, p->nf,
                       (double2*)out_dev, out_stride);
  }
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "demodulator launch failed");
  return WFK_OK;
}

const char* wfk_demod_kernel_name(const wfk_demod_plan* p, int64_t n_shots) {
  if (!p) return "";
  wfk_demod_plan* q = const_cast<wfk_demod_plan*>(p);
  q->name = std::string("demod_tile<") + type_name(p->kind) + "," + std::to_string(p->nb) + ">";
  if (splits_for(p, n_shots) > 1) q->name += " + demod_reduce";
  return q->name.c_str();
}

}  // extern "C"
