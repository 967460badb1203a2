// wfk_rocfft.h -- for the stages that run rocFFT (wfk_fir.hip, wfk_spectral.hip): owners of its handles and the
// library's one-time setup.  Host code only.
#pragma once
#include <rocfft/rocfft.h>

#include <mutex>

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

}  // namespace
