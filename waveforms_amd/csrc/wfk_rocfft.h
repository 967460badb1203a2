// wfk_rocfft.h -- for the stages that run rocFFT (wfk_fir.hip, wfk_spectral.hip, wfk_spectral_rows.hip,
// wfk_extract_rows.hip): the library's one-time setup, the owners of its handles, RocfftExec (a stage's plans with
// the execution info and the work buffer they share) and RocfftRows (the batched real-transform pair over contiguous
// rows, with its staging rows and spectrum, that the three whole-row stages are built on).  Host code only.
#pragma once
#include <rocfft/rocfft.h>

#include <mutex>

#include "wfk_host.h"

// rocfft_setup() once per process, whichever stage comes first
inline void wfk_rocfft_setup_once() {
  static std::once_flag once;
  std::call_once(once, [] { rocfft_setup(); });
}

namespace {

// owner of one rocFFT handle; out() is what the library's *_create functions fill
template <typename H, rocfft_status (*Destroy)(H)>
class RocfftHandle {
  H h_ = nullptr;

 public:
  RocfftHandle() = default;
  RocfftHandle(const RocfftHandle&) = delete;
  RocfftHandle& operator=(const RocfftHandle&) = delete;
  ~RocfftHandle() { if (h_) (void)Destroy(h_); }
  H* out() { return &h_; }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
};
using RocfftPlan = RocfftHandle<rocfft_plan, rocfft_plan_destroy>;
using RocfftInfo = RocfftHandle<rocfft_execution_info, rocfft_execution_info_destroy>;
using RocfftDesc = RocfftHandle<rocfft_plan_description, rocfft_plan_description_destroy>;

// the one text of a failed rocFFT call, device allocation or copy of the classes below
inline int wfk_fft_fail(const char* stage, int code = WFK_EHIP) {
  return wfk_fail(code, std::string(stage) + ": a rocFFT call, a device allocation or a copy failed");
}

// rows of `width` bytes, `rows` of them, device to device; one plain copy when both sides are contiguous
inline bool copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows,
                      hipStream_t s) {
  if (rows == 1 || (dpitch == width && spitch == width))
    return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, s) == hipSuccess;
}

// Up to kPlans out-of-place batched 1-D real transforms with the execution info and the work buffer they share.  The
// library wants a work buffer to outlive the plans and the info that were given it: the members below are declared
// in that order (they go in reverse), so a stage that holds its plans here has nothing to order.
class RocfftExec {
  static constexpr int kPlans = 4;
  DevBuf<char> work_;
  RocfftInfo info_;
  RocfftPlan plan_[kPlans];

 public:
  // plan i: R2C (`forward`) or C2R of length n, `batch` of them; desc: a data layout other than contiguous rows
  bool make_plan(int i, bool forward, int kind, size_t n, size_t batch, rocfft_plan_description desc = nullptr) {
    const size_t len[1] = {n};
    return rocfft_plan_create(plan_[i].out(), rocfft_placement_notinplace,
                              forward ? rocfft_transform_type_real_forward : rocfft_transform_type_real_inverse,
                              kind == WFK_OUT_F32 ? rocfft_precision_single : rocfft_precision_double, 1, len, batch,
                              desc) == rocfft_status_success;
  }
  bool has(int i) const { return (bool)plan_[i]; }
  // after the last make_plan: the info, and a work buffer of the largest size a plan asks for.  WFK_OK, WFK_EHIP
  // (the library refused) or WFK_ENOMEM (no work buffer)
  int bind() {
    size_t bytes = 0;
    for (const RocfftPlan& q : plan_) {
      size_t w = 0;
      if (q && rocfft_plan_get_work_buffer_size(q.get(), &w) != rocfft_status_success) return WFK_EHIP;
      bytes = w > bytes ? w : bytes;
    }
    if (rocfft_execution_info_create(info_.out()) != rocfft_status_success) return WFK_EHIP;
    if (!bytes) return WFK_OK;
    if (!work_.alloc(bytes)) return WFK_ENOMEM;
    const bool ok = rocfft_execution_info_set_work_buffer(info_.get(), work_.get(), bytes) == rocfft_status_success;
    return ok ? WFK_OK : WFK_EHIP;
  }
  bool set_stream(hipStream_t s) { return rocfft_execution_info_set_stream(info_.get(), s) == rocfft_status_success; }
  bool run(int i, void* in, void* out) {
    void* ib[1] = {in};
    void* ob[1] = {out};
    return rocfft_execute(plan_[i].get(), ib, ob, info_.get()) == rocfft_status_success;
  }
};

// The R2C / C2R pair of length n over `batch` contiguous rows, with what every whole-row stage puts around it: staging
// rows [batch][n] (rocFFT may overwrite the input of a real transform, and the caller's rows may be strided or be the
// output) and the spectrum [batch][n / 2 + 1].  rows2 > 0 adds a second spectrum of rows2 rows for a second input that
// goes through the same staging, and, where rows2 != batch, the forward plan of that batch count.
class RocfftRows {
  enum { kFwd, kInv, kFwd2 };
  size_t es_ = 0, width_ = 0, batch_ = 0;   // bytes of a sample and of a staged row; rows
  hipStream_t s_ = nullptr;
  DevBuf<char> rows_, spec_, spec2_;
  RocfftExec fft_;

 public:
  bool create(int64_t n, int32_t batch, int kind, int32_t rows2 = 0) {
    es_ = wfk_elem_size(kind);
    width_ = (size_t)n * es_;
    const size_t spec_row = (size_t)(n / 2 + 1) * 2 * es_;
    batch_ = (size_t)batch;
    bool ok = fft_.make_plan(kFwd, true, kind, (size_t)n, batch_);
    if (ok && rows2 && rows2 != batch) ok = fft_.make_plan(kFwd2, true, kind, (size_t)n, (size_t)rows2);
    ok = ok && fft_.make_plan(kInv, false, kind, (size_t)n, batch_) && fft_.bind() == WFK_OK;
    ok = ok && spec_.alloc(batch_ * spec_row) && (!rows2 || spec2_.alloc((size_t)rows2 * spec_row));
    ok = ok && rows_.alloc(batch_ * width_);
    if (!ok) (void)hipGetLastError();
    return ok;
  }
  char* rows() const { return rows_.get(); }
  char* spec() const { return spec_.get(); }
  char* spec2() const { return spec2_.get(); }
  // the stream of everything below, until the next call
  bool set_stream(hipStream_t s) { s_ = s; return fft_.set_stream(s); }
  // the caller's `rows` rows, `stride` samples apart -> staging
  bool stage(const void* src, int64_t stride, int64_t rows) {
    return copy_rows(rows_.get(), width_, src, (size_t)stride * es_, width_, (size_t)rows, s_);
  }
  bool forward() { return fft_.run(kFwd, rows_.get(), spec_.get()); }                               // staging -> spec
  bool forward2() { return fft_.run(fft_.has(kFwd2) ? kFwd2 : kFwd, rows_.get(), spec2_.get()); }   // staging -> spec2
  bool inverse(void* out) { return fft_.run(kInv, spec_.get(), out); }   // spec -> contiguous rows at `out`
  // staging -> the caller's batch rows, `stride` samples apart
  bool unstage(void* dst, int64_t stride) {
    return copy_rows(dst, (size_t)stride * es_, rows_.get(), width_, width_, batch_, s_);
  }
};

}  // namespace
