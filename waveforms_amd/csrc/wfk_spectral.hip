// wfk_spectral.hip -- whole-signal transfer-function stage:
//   out = irfft( rfft(sig) * H ),  H given per frequency bin k = 0 .. n/2  (f_k = k * fs / n)
// which is what the reference's FFT-domain operations do with scipy.fftpack on the host:
//   reflection(sig, A, tau, fs)          = ifft(fft(sig) * H_refl).real   distortion.py:208-210
//   correct_reflection(sig, A, tau, fs)  = ifft(fft(sig) / H_refl).real   distortion.py:213-223
// (H conjugate-symmetric => the real transforms are exact).  Batched rocFFT R2C / C2R of
// arbitrary length n plus one hand-written multiply kernel (1/n folded in).
#include <hip/hip_runtime.h>

#include <memory>
#include <new>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rocfft.h"

namespace {

template <typename C>
__global__ void __launch_bounds__(256) spec_mul(C* __restrict__ spec, const double2* __restrict__ H,
                                                int64_t nf, int64_t total, double scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const double2 h = H[idx % nf];
  const C a = spec[idx];
  C r;
  r.x = (decltype(r.x))((a.x * h.x - a.y * h.y) * scale);
  r.y = (decltype(r.y))((a.x * h.y + a.y * h.x) * scale);
  spec[idx] = r;
}
}  // namespace

struct wfk_spectral_plan {
  int64_t n = 0, nf = 0;
  int32_t batch = 0, kind = 0;
  RocfftRows fft;   // every apply stages its input: that is what makes out == in legal (wfk.h)
};

extern "C" {

int wfk_spectral_plan_destroy(wfk_spectral_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_spectral_plan_create(int64_t n, int32_t batch, int kind, wfk_spectral_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 1 || batch < 1) return wfk_fail(WFK_EINVAL, "bad spectral plan arguments");
  if (const int rc = wfk_check_kind(kind)) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_spectral_plan> p(new wfk_spectral_plan());
  p->n = n; p->nf = n / 2 + 1; p->batch = batch; p->kind = kind;
  if (!p->fft.create(n, batch, kind)) return wfk_fft_fail("spectral plan");
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the spectral plan");
}

/* rows are CONTIGUOUS (stride n); H_dev: n/2+1 complex128 values on the device */
int wfk_spectral_apply(wfk_spectral_plan* p, const void* in_dev, void* out_dev, const void* H_dev,
                       void* hip_stream) {
  if (!p || !in_dev || !out_dev || !H_dev) return wfk_fail(WFK_EINVAL, "null argument");
  hipStream_t s = (hipStream_t)hip_stream;
  RocfftRows& f = p->fft;
  if (!(f.set_stream(s) && f.stage(in_dev, p->n, p->batch) && f.forward())) return wfk_fft_fail("spectral");
  const int64_t total = (int64_t)p->batch * p->nf;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (p->kind == WFK_OUT_F32)
    hipLaunchKernelGGL(spec_mul<float2>, dim3(blocks), dim3(256), 0, s, (float2*)f.spec(), (const double2*)H_dev,
                       p->nf, total, 1.0 / (double)p->n);
  else
    hipLaunchKernelGGL(spec_mul<double2>, dim3(blocks), dim3(256), 0, s, (double2*)f.spec(), (const double2*)H_dev,
                       p->nf, total, 1.0 / (double)p->n);
  if (!f.inverse(out_dev)) return wfk_fft_fail("spectral");
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "spectral kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
