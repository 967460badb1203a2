// wfk_probe.hip -- the tail of the Z-distortion fit model (reference: waveforms/distortion.py:349-366,
// phase_curve): a boxcar integral of every row of a batch of distorted signals, read off at the probe
// times by linear interpolation,
//   conv[r, i] = gain * sum_{m < pp} y[r, i + c - m]            np.convolve(s, [ones(pp), zeros(sp)], 'same')
//   out[r, q]  = np.interp(t_q, tlist, conv[r])                 (y is zero outside [0, n))
// without ever forming conv: a probe needs conv at its two bracketing grid points only.
//
// The plan is built on the host from the caller's own tlist and t: per query q the bracket index j_q,
// dx_q = t_q - tlist[j_q] and w_q = tlist[j_q + 1] - tlist[j_q], by np.interp's rules (clamped to the
// first / last grid value, NaN in -> NaN out, queries in any order; wfk_boxprobe_brackets).
//
// boxprobe_wave: ONE wave owns one (row, query).  The windows of conv[j] and conv[j + 1] share pp - 1 of
// their pp samples: the 64 lanes stride the pp + 1 samples of both (coalesced 512-B loads), every lane
// keeps two partial sums in the order of its own samples, a fixed xor butterfly adds the lanes, and lane 0
// stores  f0 + (f1 - f0) / w * dx  -- np.interp's expression, without contraction into an fma.  No atomics,
// nothing that depends on the row's place in the batch: results are bitwise reproducible, and equal rows
// give equal results.  fp64 throughout.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"

namespace {

constexpr int kWavesPerBlock = 4;

__global__ void __launch_bounds__(64 * kWavesPerBlock)
    boxprobe_wave(const double* __restrict__ y, int64_t n_rows, int64_t y_stride, int64_t n,
                  const int64_t* __restrict__ jq, const double* __restrict__ dxq, const double* __restrict__ wq,
                  int32_t nq, int64_t pp, int64_t c, double gain, double* __restrict__ out, int64_t out_stride) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (o >= n_rows * nq) return;   // uniform per wave
  const int64_t r = o / nq, q = o % nq;
  const double* __restrict__ row = y + r * y_stride;
  // samples lo .. lo + pp: the first belongs to conv[j] only, the last to conv[j + 1] only
  const int64_t lo = jq[q] + c - pp + 1;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t k = lane; k <= pp; k += 64) {
    const int64_t i = lo + k;
    const double v = (i >= 0 && i < n) ? row[i] : 0.0;
    s0 += k < pp ? v : 0.0;
    s1 += k > 0 ? v : 0.0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, 64);
    s1 += __shfl_xor(s1, off, 64);
  }
  if (lane == 0) {
    const double f0 = gain * s0, f1 = gain * s1;
    const double slope = (f1 - f0) / wq[q];
    out[r * out_stride + q] = __dadd_rn(__dmul_rn(slope, dxq[q]), f0);
  }
}

}  // namespace

struct wfk_boxprobe_plan {
  int64_t n = 0, pp = 0, c = 0;
  int32_t nq = 0;
  double gain = 0.0;
  DevBuf<int64_t> j;
  DevBuf<double> dx, w;
};

extern "C" {

int wfk_boxprobe_brackets(const double* tlist, int64_t n, const double* t, int64_t n_query, int64_t* j_out,
                          double* dx_out, double* w_out) {
  if (n < 1 || n_query < 0 || !tlist || (n_query > 0 && (!t || !j_out || !dx_out || !w_out)))
    return wfk_fail(WFK_EINVAL, "probe brackets: need n >= 1 grid values, n_query >= 0 and non-null arrays");
  for (int64_t i = 0; i < n; ++i)
    if (std::isnan(tlist[i]) || (i > 0 && tlist[i] < tlist[i - 1]))
      return wfk_fail(WFK_EINVAL, "probe brackets: tlist must be ascending without NaN (index " +
                                      std::to_string((long long)i) + ")");
  for (int64_t q = 0; q < n_query; ++q) {
    const double x = t[q];
    int64_t j = 0;
    double dx = 0.0, w = 1.0;
    if (std::isnan(x)) {
      dx = x;                                   // NaN in -> NaN out
    } else if (x >= tlist[n - 1]) {
      j = n - 1;                                // right of (or on) the last grid value: that value
    } else if (x > tlist[0]) {
      int64_t lo = 0, hi = n - 1;               // tlist[lo] <= x < tlist[hi]
      while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (x >= tlist[mid]) lo = mid; else hi = mid;
      }
      j = lo;
      dx = x - tlist[j];
      w = tlist[j + 1] - tlist[j];
    }                                           // else: left of (or on) the first grid value
    j_out[q] = j;
    dx_out[q] = dx;
    w_out[q] = w;
  }
  return WFK_OK;
}

int wfk_boxprobe_plan_destroy(wfk_boxprobe_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_boxprobe_plan_create(const double* tlist_host, int64_t n, const double* t_host, int32_t n_query,
                             int64_t pp, int64_t c, double gain, wfk_boxprobe_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n_query < 1) return wfk_fail(WFK_EINVAL, "probe plan: n_query >= 1");
  if (n < 1 || n > ((int64_t)1 << 40)) return wfk_fail(WFK_EINVAL, "probe plan: 1 <= n <= 2^40");
  if (pp < 0 || pp > n) return wfk_fail(WFK_EINVAL, "probe plan: 0 <= pp <= n");
  if (c < -n || c > 2 * n) return wfk_fail(WFK_EINVAL, "probe plan: -n <= c <= 2 n");
  if (!std::isfinite(gain)) return wfk_fail(WFK_EINVAL, "probe plan: gain must be finite");
  std::vector<int64_t> j((size_t)n_query);
  std::vector<double> dx((size_t)n_query), w((size_t)n_query);
  const int rc = wfk_boxprobe_brackets(tlist_host, n, t_host, n_query, j.data(), dx.data(), w.data());
  if (rc != WFK_OK) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_boxprobe_plan> p(new wfk_boxprobe_plan());
  p->n = n; p->pp = pp; p->c = c; p->nq = n_query; p->gain = gain;
  if (!p->j.upload(j) || !p->dx.upload(dx) || !p->w.upload(w)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "probe plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the probe plan");
}

int wfk_boxprobe_apply(wfk_boxprobe_plan* p, const double* y_dev, int64_t n_rows, int64_t y_stride,
                       double* out_dev, int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (n_rows < 0) return wfk_fail(WFK_EINVAL, "n_rows < 0");
  if (n_rows == 0) return WFK_OK;
  if (!y_dev || !out_dev) return wfk_fail(WFK_EINVAL, "null argument");
  if (y_stride < p->n) return wfk_fail(WFK_EINVAL, "y_stride < n");
  if (out_stride < p->nq) return wfk_fail(WFK_EINVAL, "out_stride < n_query");
  if ((((uintptr_t)y_dev | (uintptr_t)out_dev) & 7) != 0)
    return wfk_fail(WFK_EINVAL, "y and out must be 8-byte aligned");
  const int64_t blocks = (n_rows * p->nq + kWavesPerBlock - 1) / kWavesPerBlock;
  if (n_rows > ((int64_t)1 << 40) || blocks > 0x7fffffff) return wfk_fail(WFK_EINVAL, "too many (row, query) pairs");
  hipLaunchKernelGGL(boxprobe_wave, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, (hipStream_t)hip_stream,
                     y_dev, n_rows, y_stride, p->n, p->j.get(), p->dx.get(), p->w.get(), p->nq, p->pp, p->c,
                     p->gain, out_dev, out_stride);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "probe launch failed");
  return WFK_OK;
}

const char* wfk_boxprobe_kernel_name(const wfk_boxprobe_plan* p) { return p ? "boxprobe_wave" : ""; }

}  // extern "C"
