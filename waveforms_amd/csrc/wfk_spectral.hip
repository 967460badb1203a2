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
  // (members go in reverse order: the rocFFT plans and the execution info before the work buffer they were given)
  DevBuf<char> tmp;       // every apply copies its input here first: rocFFT's real transforms may overwrite their
                          // input, and it is what makes out == in legal (wfk.h)
  DevBuf<char> spec, work;
  RocfftInfo info;
  RocfftPlan fwd, inv;
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
  if (kind != WFK_OUT_F64 && kind != WFK_OUT_F32) return wfk_fail(WFK_EINVAL, "kind must be F64 or F32");
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_spectral_plan> p(new wfk_spectral_plan());
  p->n = n; p->nf = n / 2 + 1; p->batch = batch; p->kind = kind;
  const rocfft_precision prec = kind == WFK_OUT_F32 ? rocfft_precision_single : rocfft_precision_double;
  const size_t es = kind == WFK_OUT_F32 ? 4 : 8;
  const size_t len[1] = {(size_t)n};
  bool ok = rocfft_plan_create(p->fwd.out(), rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                               prec, 1, len, (size_t)batch, nullptr) == rocfft_status_success;
  ok = ok && rocfft_plan_create(p->inv.out(), rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                prec, 1, len, (size_t)batch, nullptr) == rocfft_status_success;
  size_t wa = 0, wb = 0;
  if (ok) {
    rocfft_plan_get_work_buffer_size(p->fwd.get(), &wa);
    rocfft_plan_get_work_buffer_size(p->inv.get(), &wb);
    const size_t wbytes = wa > wb ? wa : wb;
    ok = rocfft_execution_info_create(p->info.out()) == rocfft_status_success;
    if (ok && wbytes)
      ok = p->work.alloc(wbytes) &&
           rocfft_execution_info_set_work_buffer(p->info.get(), p->work.get(), wbytes) == rocfft_status_success;
    ok = ok && p->spec.alloc((size_t)batch * p->nf * 2 * es);
    ok = ok && p->tmp.alloc((size_t)batch * n * es);
  }
  if (!ok) return wfk_fail(WFK_EHIP, "rocFFT plan / buffer creation failed");
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
  const size_t es = p->kind == WFK_OUT_F32 ? 4 : 8;
  if (rocfft_execution_info_set_stream(p->info.get(), s) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft set_stream failed");
  // rocFFT may overwrite the input of an out-of-place real transform: work on a copy
  if (hipMemcpyAsync(p->tmp.get(), in_dev, (size_t)p->batch * p->n * es, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return wfk_fail(WFK_EHIP, "copy failed");
  void* ib[1] = {p->tmp.get()};
  void* ob[1] = {p->spec.get()};
  if (rocfft_execute(p->fwd.get(), ib, ob, p->info.get()) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft forward failed");
  const int64_t total = (int64_t)p->batch * p->nf;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (p->kind == WFK_OUT_F32)
    hipLaunchKernelGGL(spec_mul<float2>, dim3(blocks), dim3(256), 0, s, (float2*)p->spec.get(),
                       (const double2*)H_dev, p->nf, total, 1.0 / (double)p->n);
  else
    hipLaunchKernelGGL(spec_mul<double2>, dim3(blocks), dim3(256), 0, s, (double2*)p->spec.get(),
                       (const double2*)H_dev, p->nf, total, 1.0 / (double)p->n);
  void* ib2[1] = {p->spec.get()};
  void* ob2[1] = {out_dev};
  if (rocfft_execute(p->inv.get(), ib2, ob2, p->info.get()) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft inverse failed");
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "spectral kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
