// wfk_fir.hip -- FIR stage of the hot path:  predistort(sig, ker=ker)
// (reference: waveforms/distortion.py:329-337 -- zero-pad to [0_N, sig, 0_N],
//  scipy.signal.fftconvolve(..., 'full'), crop [N + K//2, 2N + K//2)), i.e.
//      out[i] = sum_k ker[k] * sig[i + K//2 - k]      with sig = 0 outside [0, N)
//
// The reference takes ONE real FFT of >= 3N + K - 1 points per channel.  Here: batched
// overlap-save on rocFFT.  Per chunk of channels:
//   gather   : overlapping length-L windows (hop M = L - K + 1) of the signal, zero padded,
//              window b of a row starts at sample b*M - (K-1) + K//2          [HIP kernel]
//   R2C FFT  : rocFFT, batch = channels * blocks
//   multiply : by the precomputed kernel spectrum (1/L folded in)             [HIP kernel]
//   C2R FFT  : rocFFT
//   scatter  : valid part [K-1, L) of every block -> out[b*M + r]            [HIP kernel]
// All buffers and rocFFT plans are created in wfk_fir_plan_create; wfk_fir_apply only
// enqueues work on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rocfft.h"

namespace {


template <typename T>
__global__ void __launch_bounds__(256) fir_gather(const T* __restrict__ in, int64_t in_stride,
                                                  T* __restrict__ win, int64_t n, int L, int M,
                                                  int lead, int64_t nblk) {
  // grid: x = L/256 segments, y = block, z = channel (within chunk)
  const int64_t b = blockIdx.y, ch = blockIdx.z;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  const int64_t src = b * M + i - lead;
  T v = (T)0;
  if (src >= 0 && src < n) v = in[ch * in_stride + src];
  win[(ch * nblk + b) * L + i] = v;
}

template <typename C>
__global__ void __launch_bounds__(256) fir_multiply(C* __restrict__ spec, const C* __restrict__ ks,
                                                    int nf, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int f = (int)(idx % nf);
  const C a = spec[idx], k = ks[f];
  C r;
  r.x = a.x * k.x - a.y * k.y;
  r.y = a.x * k.y + a.y * k.x;
  spec[idx] = r;
}

template <typename T>
__global__ void __launch_bounds__(256) fir_scatter(const T* __restrict__ win, T* __restrict__ out,
                                                   int64_t out_stride, int64_t n, int L, int M,
                                                   int K, int64_t nblk) {
  const int64_t b = blockIdx.y, ch = blockIdx.z;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  const int64_t dst = b * M + r;
  if (dst >= n) return;
  out[ch * out_stride + dst] = win[(ch * nblk + b) * L + (K - 1) + r];
}

// long double -> the plan's element kind: complex element `at` of `dst`
void put_cx(std::vector<char>& dst, bool f32, size_t at, const std::complex<long double>& v) {
  if (f32) {
    float* d = reinterpret_cast<float*>(dst.data()) + 2 * at;
    d[0] = (float)v.real(); d[1] = (float)v.imag();
  } else {
    double* d = reinterpret_cast<double*>(dst.data()) + 2 * at;
    d[0] = (double)v.real(); d[1] = (double)v.imag();
  }
}

const char kTooLong[] = "signal too long for one rocFFT FIR plan (blocks > 65535)";

enum { kFwd, kInv, kFwdTail, kInvTail };   // the plans of wfk_fir_plan::fft

}  // namespace

struct wfk_fir_plan {
  bool fused = false;
  int32_t nseg = 1, Kseg = 0;  // fused: the kernel is cut into nseg segments of Kseg taps, one
                               // pass of the fused kernel each (passes after the first accumulate)
  int32_t K = 0, batch = 0, kind = 0, L = 0, M = 0, lead = 0, chunk = 0;
  int64_t n = 0, nblk = 0;
  int32_t tail = 0;  // channels in the last, smaller chunk (0: none)
  int64_t krow = 0;            // per-row kernels (wfk_fir_plan_create_rows): complex elements between the
                               // spectra of consecutive rows; 0: one kernel for every row
  DevBuf<char> tw;             // fused: exp(-2 pi i j / L), j < 256
  DevBuf<char> kspec, spec, win;
  RocfftExec fft;              // the transforms of a chunk and of the smaller last chunk
};

// the R2C / C2R pair over the windows of `channels` rows, as plans fwd and fwd + 1 of p->fft
static bool make_plans(wfk_fir_plan* p, int32_t channels, int fwd) {
  const size_t L = (size_t)p->L, nb = (size_t)channels * (size_t)p->nblk, nf = L / 2 + 1;
  RocfftDesc df, di;
  const size_t one[1] = {1};
  return rocfft_plan_description_create(df.out()) == rocfft_status_success &&
         rocfft_plan_description_set_data_layout(df.get(), rocfft_array_type_real,
                                                 rocfft_array_type_hermitian_interleaved, nullptr, nullptr, 1, one, L,
                                                 1, one, nf) == rocfft_status_success &&
         p->fft.make_plan(fwd, true, p->kind, L, nb, df.get()) &&
         rocfft_plan_description_create(di.out()) == rocfft_status_success &&
         rocfft_plan_description_set_data_layout(di.get(), rocfft_array_type_hermitian_interleaved,
                                                 rocfft_array_type_real, nullptr, nullptr, 1, one, nf, 1, one, L) ==
             rocfft_status_success &&
         p->fft.make_plan(fwd + 1, false, p->kind, L, nb, di.get());
}

template <typename T, typename C>
static int fir_run(wfk_fir_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                   int64_t out_stride, hipStream_t s) {
  const int L = p->L, M = p->M;
  const int64_t nf = L / 2 + 1;
  if (!p->fft.set_stream(s)) return wfk_fft_fail("FIR");
  for (int32_t c0 = 0; c0 < p->batch; c0 += p->chunk) {
    const int32_t nc = std::min(p->chunk, p->batch - c0);
    const bool tail = nc != p->chunk;
    const T* in = static_cast<const T*>(in_dev) + (int64_t)c0 * in_stride;
    T* out = static_cast<T*>(out_dev) + (int64_t)c0 * out_stride;
    T* win = reinterpret_cast<T*>(p->win.get());
    C* spec = reinterpret_cast<C*>(p->spec.get());
    dim3 gg((L + 255) / 256, (unsigned)p->nblk, (unsigned)nc);
    hipLaunchKernelGGL(fir_gather<T>, gg, dim3(256), 0, s, in, in_stride, win, p->n, L, M, p->lead,
                       p->nblk);
    if (!p->fft.run(tail ? kFwdTail : kFwd, win, spec)) return wfk_fft_fail("FIR");
    const int64_t total = (int64_t)nc * p->nblk * nf;
    hipLaunchKernelGGL(fir_multiply<C>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, spec,
                       reinterpret_cast<const C*>(p->kspec.get()), (int)nf, total);
    if (!p->fft.run(tail ? kInvTail : kInv, spec, win)) return wfk_fft_fail("FIR");
    dim3 gs((M + 255) / 256, (unsigned)p->nblk, (unsigned)nc);
    hipLaunchKernelGGL(fir_scatter<T>, gs, dim3(256), 0, s, win, out, out_stride, p->n, L, M, p->K,
                       p->nblk);
  }
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "FIR kernel launch failed");
  return WFK_OK;
}

// used by the sampler -> FIR chain (wfk_fir_sampled.hip): the kernel spectrum and twiddles of a
// plan that runs as ONE pass of the on-chip transform
extern "C" void wfk_internal_fir_tables(const wfk_fir_plan* p, const void** kspec, const void** tw,
                                        int* fused, int* nseg, int* K, int* lead) {
  *kspec = p->kspec.get(); *tw = p->tw.get(); *fused = p->fused ? 1 : 0; *nseg = p->nseg; *K = p->K;
  *lead = (p->K - 1) - p->K / 2;
}

extern "C" int64_t wfk_internal_fir_krow(const wfk_fir_plan* p) { return p->krow; }

extern "C" {

// the form wfk_fir_apply runs, read from the fields it branches on
const char* wfk_fir_kernel_name(const wfk_fir_plan* p) {
  if (!p || p->n == 0) return "";
  static thread_local std::string name;
  const std::string T = p->kind == WFK_OUT_F32 ? "float" : "double";
  if (p->fused)
    name = "fir_fused<" + T + ">" + (p->nseg > 1 ? " x " + std::to_string(p->nseg) : std::string()) +
           (p->krow ? " per-row spectra" : "");
  else
    name = "fir_gather<" + T + "> + rocfft<L=" + std::to_string(p->L) + ",rows=" + std::to_string(p->chunk) + "> + fir_multiply<" +
           T + "> + fir_scatter<" + T + ">";
  return name.c_str();
}

int wfk_fir_plan_destroy(wfk_fir_plan* p) {
  delete p;
  return WFK_OK;
}

static int fir_plan_create(const double* ker_host, int32_t K, int64_t n, int32_t batch, int kind,
                           wfk_fir_plan** out, bool per_row);

int wfk_fir_plan_create(const double* ker_host, int32_t K, int64_t n, int32_t batch, int kind,
                        wfk_fir_plan** out) {
  return fir_plan_create(ker_host, K, n, batch, kind, out, false);
}

int wfk_fir_plan_create_rows(const double* kers_host, int32_t K, int64_t n, int32_t batch, int kind,
                             wfk_fir_plan** out) {
  return fir_plan_create(kers_host, K, n, batch, kind, out, true);
}

static int fir_plan_create(const double* ker_host, int32_t K, int64_t n, int32_t batch, int kind,
                           wfk_fir_plan** out, bool per_row) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!ker_host || K < 1 || n < 0 || batch < 1) return wfk_fail(WFK_EINVAL, "bad FIR arguments");
  if (const int rc = wfk_check_kind(kind, "FIR ")) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_fir_plan> p(new wfk_fir_plan());
  p->K = K; p->n = n; p->batch = batch; p->kind = kind;
  const int FL = wfk_internal_fir_fused_len();
  const char* force = getenv("WFK_FIR_ROCFFT");
  // The fused kernel takes kernels up to FL - 2559 = 1537 taps (hop >= 2560 = 5/8 of the
  // transform).  Longer kernels are cut into up to WFK_FIR_MAXSEG equal segments,
  //   out[i] = sum_j sum_k' ker[j*Kseg + k'] sig[(i + K//2 - j*Kseg) - k'],
  // i.e. one pass per segment with its own input offset, accumulating: 2-4 x 9.4 ms (+ the
  // re-read of `out`) against ~66 ms of the rocFFT pipeline on 256 x 1e7 fp64.
  const int KMAX = FL - 2559, WFK_FIR_MAXSEG = 4;
  p->nseg = (K + KMAX - 1) / KMAX;
  p->Kseg = (K + p->nseg - 1) / p->nseg;
  p->fused = p->nseg <= WFK_FIR_MAXSEG && batch <= 65535 && !(force && force[0] == '1');
  if (!p->fused) { p->nseg = 1; p->Kseg = K; }
  if (per_row && !p->fused)
    return wfk_fail(WFK_EUNSUP, "per-row FIR kernels need the on-chip transform (K <= 6148, batch <= 65535, WFK_FIR_ROCFFT unset)");
  int L = 1024;
  while (L < 8 * K) L *= 2;               // hop M = L - K + 1 >= 7/8 L
  if (const char* e = getenv("WFK_FIR_L")) { int v = atoi(e); if (v >= 2 * K && (v & (v - 1)) == 0) L = v; }
  if (p->fused) L = FL;
  const int Kt = p->fused ? p->Kseg : K;             // taps per transform
  p->L = L; p->M = L - Kt + 1; p->lead = (Kt - 1) - K / 2;   // fused: + j*Kseg for segment j
  p->nblk = n > 0 ? (n + p->M - 1) / p->M : 0;
  if (n == 0) { *out = p.release(); return WFK_OK; }
  // gather / scatter put the block in gridDim.y: refuse before any rocFFT plan or buffer is made
  if (!p->fused && p->nblk > 65535) return wfk_fail(WFK_EINVAL, kTooLong);
  const bool f32 = kind == WFK_OUT_F32;
  const size_t es = wfk_elem_size(kind);
  const size_t nf = p->fused ? (size_t)L : (size_t)L / 2 + 1;   // fused: full complex spectrum
  if (!p->fused) {
    const double per_ch = (double)p->nblk * ((double)L * es + (double)nf * 2 * es);
    int64_t chunk = (int64_t)(3.0e9 / per_ch);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, batch));
    chunk = std::min<int64_t>(chunk, 65535);   // gather / scatter put the chunk's row in gridDim.z
    // WFK_FIR_CHUNK=<rows>: a lower cap, so that the chunk loop and the tail plans run at test sizes
    if (const char* e = getenv("WFK_FIR_CHUNK")) {
      char* end = nullptr;
      const long long v = strtoll(e, &end, 10);
      if (end != e && *end == '\0' && v >= 1) chunk = std::min<int64_t>(chunk, v);
    }
    p->chunk = (int32_t)chunk;
    p->tail = batch % p->chunk;
    if (!make_plans(p.get(), p->chunk, kFwd) || (p->tail && !make_plans(p.get(), p->tail, kFwdTail)))
      return wfk_fft_fail("FIR plan");
    if (const int rc = p->fft.bind()) return wfk_fft_fail("FIR plan", rc);
    if (!p->win.alloc((size_t)p->chunk * p->nblk * L * es) || !p->spec.alloc((size_t)p->chunk * p->nblk * nf * 2 * es))
      return wfk_fft_fail("FIR plan", WFK_ENOMEM);
  }
  const size_t nrow = per_row ? (size_t)batch : 1;
  p->krow = per_row ? (int64_t)((size_t)p->nseg * nf) : 0;
  std::vector<char> ks(nrow * (size_t)p->nseg * nf * 2 * es);
  if (!p->kspec.alloc(ks.size()) || (p->fused && !p->tw.alloc(256 * 2 * es)))
    return wfk_fail(WFK_ENOMEM, "FIR buffer allocation failed");
  // kernel spectrum on the host (K*L/2 flops, once): DFT of ker zero-padded to L, times 1/L, in long double and
  // narrowed once to the plan's kind
  std::vector<std::complex<long double>> tw(L);
  for (int i = 0; i < L; ++i) {
    long double th = -2.0L * 3.141592653589793238462643383279502884L * i / L;
    tw[i] = {cosl(th), sinl(th)};
  }
  if (!per_row) {
    for (int sg = 0; sg < p->nseg; ++sg) {
      const int k0 = sg * p->Kseg, k1 = std::min(K, k0 + (p->fused ? p->Kseg : K));
      for (size_t f = 0; f < nf; ++f) {
        std::complex<long double> acc = 0;
        for (int k = k0; k < k1; ++k)
          acc += (long double)ker_host[k] * tw[(size_t)((f * (size_t)(k - k0)) % L)];
        acc /= (long double)L;
        put_cx(ks, f32, sg * nf + f, acc);
      }
    }
  } else {
    // one spectrum per row: a radix-2 transform in long double (K L / 2 products per kernel, as above, would
    // be seconds for a few thousand rows); bit-reversed input, L = 4096 here (fused path only)
    int lg = 0;
    while ((1 << lg) < L) ++lg;
    std::vector<std::complex<long double>> z((size_t)L);
    for (size_t r = 0; r < nrow; ++r)
      for (int sg = 0; sg < p->nseg; ++sg) {
        const int k0 = sg * p->Kseg, k1 = std::min(K, k0 + p->Kseg);
        for (int i = 0; i < L; ++i) {
          int rev = 0;
          for (int b = 0; b < lg; ++b) rev |= ((i >> b) & 1) << (lg - 1 - b);
          z[(size_t)rev] = i < k1 - k0 ? (long double)ker_host[r * (size_t)K + k0 + i] : 0.0L;
        }
        for (int half = 1; half < L; half <<= 1) {
          const int stepw = L / (2 * half);
          for (int i0 = 0; i0 < L; i0 += 2 * half)
            for (int j = 0; j < half; ++j) {
              const std::complex<long double> t = z[(size_t)(i0 + j + half)] * tw[(size_t)(j * stepw)];
              z[(size_t)(i0 + j + half)] = z[(size_t)(i0 + j)] - t;
              z[(size_t)(i0 + j)] += t;
            }
        }
        for (size_t f = 0; f < nf; ++f) put_cx(ks, f32, (r * p->nseg + sg) * nf + f, z[f] / (long double)L);
      }
  }
  hipError_t e = hipMemcpy(p->kspec.get(), ks.data(), ks.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && p->fused) {
    std::vector<char> t(256 * 2 * es);
    for (int j = 0; j < 256; ++j) put_cx(t, f32, j, tw[j]);
    e = hipMemcpy(p->tw.get(), t.data(), t.size(), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) return wfk_fail(WFK_EHIP, "kernel spectrum upload failed");
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the FIR plan");
}

int wfk_fir_apply(wfk_fir_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                  int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;
  // no path works in place: the fused kernel reads halos that other workgroups overwrite, passes 2 to 4 of a long
  // kernel read `in` again, and the pipeline's later chunks gather after the earlier ones have scattered
  if (const int rc = wfk_check_rows("FIR", p->n, wfk_elem_size(p->kind), in_dev, p->batch, in_stride, out_dev,
                                    p->batch, out_stride, true))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (p->fused) {
    const size_t seg_bytes = (size_t)p->L * 2 * wfk_elem_size(p->kind);
    for (int sg = 0; sg < p->nseg; ++sg)
      if (wfk_internal_fir_fused_launch(p->kind, in_dev, in_stride, out_dev, out_stride,
                                        p->kspec.get() + sg * seg_bytes, p->tw.get(), p->n, p->M,
                                        p->Kseg, p->lead + sg * p->Kseg, p->nblk, p->batch, sg > 0, s, p->krow))
        return wfk_fail(WFK_EHIP, "fused FIR kernel launch failed");
    return WFK_OK;
  }
  if (p->nblk > 65535) return wfk_fail(WFK_EINVAL, kTooLong);   // (refused at creation already)
  if (p->kind == WFK_OUT_F32) return fir_run<float, float2>(p, in_dev, in_stride, out_dev, out_stride, s);
  return fir_run<double, double2>(p, in_dev, in_stride, out_dev, out_stride, s);
}

}  // extern "C"
