// wfk_spectral_rows.hip -- per-row reflection / inverse-reflection / delay correction in the frequency domain:
//   out[r] = irfft( rfft(in[r]) * H_r ),   H_r(k) = prod_t H_rt(k),   k = 0 .. n/2,   f_k = k * fs / n
// with, for e = exp(-2 pi i f_k tau),
//   REFLECT  (1 - A) / (1 - A e)     reflection(sig, A, tau, fs)           distortion.py:188-210
//   CORRECT  (1 - A e) / (1 - A)     correct_reflection(sig, A, tau, fs)   distortion.py:213-223
//   DELAY    e                       band-limited circular delay by tau (tau < 0: advance)
// Every row has its own list of up to WFK_SPEC_ROWS_MAX_TERMS terms.  H is never stored: spec_rows_mul forms it per
// (row, bin) from the row's small term table while it makes its one pass over the R2C output (1/n folded in).
//
// Phase.  f_k tau = k * c with c = tau fs / n.  k c reaches thousands of cycles, so rounding it to one double before
// the sincos would cost (cycles * 2^-53) of phase.  The host computes c in quad precision and stores it as a
// (hi, lo) pair of doubles; the device takes p = fl(k * hi), the exact error of that product with one fma, drops
// the whole cycles of p -- p - rint(p) is exact -- and only then adds the small parts: the reduced phase in
// [-1/2, 1/2] cycles is good to ~2^-54 cycles, whatever its size was, and goes to sincospi.  k is an integer
// below 2^53: exact in a double.  (The file is compiled with contraction off: a contracted k * hi - rint(p) would
// count the product's rounding error twice.)
//
// Table access.  spec_rows_mul is a row-slot kernel (wfk_rows_dev.h): the row's term count and terms arrive by scalar
// loads, once per wave, and the branch on a term's kind is a scalar branch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rocfft.h"
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxTerms = WFK_SPEC_ROWS_MAX_TERMS;

// one term as the device reads it: c = tau fs / n as (hi, lo); g = 1 - A (REFLECT), 1 / (1 - A) (CORRECT)
struct SpecTerm {
  double c_hi, c_lo, a, g;
  int32_t kind, pad;
};

typedef __float128 quad;

// c = tau fs / n in quad precision -> (hi, lo)
inline void phase_step(double tau, double fs, int64_t n, double* hi, double* lo) {
  const quad c = (quad)tau * (quad)fs / (quad)n;
  *hi = (double)c;
  *lo = (double)(c - (quad)*hi);
}

// scale * prod_t H_t(k) for the T terms at tt
__device__ __forceinline__ double2 row_transfer(const SpecTerm* __restrict__ tt, int T, double k, double scale) {
  double hr = scale, hi = 0.0;
  for (int t = 0; t < T; ++t) {
    const double chi = tt[t].c_hi, clo = tt[t].c_lo, A = tt[t].a, g = tt[t].g;
    const int kind = tt[t].kind;
    const double p = k * chi;
    const double err = fma(k, chi, -p) + k * clo;   // k c = p + err
    const double cyc = (p - rint(p)) + err;         // reduced phase in cycles
    double s, c;
    sincospi(-2.0 * cyc, &s, &c);                   // e = c + i s
    double tr, ti;
    if (kind == WFK_SPEC_DELAY) {
      tr = c;
      ti = s;
    } else {
      const double dr = fma(-A, c, 1.0), di = -A * s;   // 1 - A e
      if (kind == WFK_SPEC_CORRECT) {
        tr = dr * g;
        ti = di * g;
      } else {                                          // (1 - A) conj(d) / |d|^2
        const double q = g / fma(dr, dr, di * di);
        tr = dr * q;
        ti = -di * q;
      }
    }
    const double nr = hr * tr - hi * ti;
    hi = hr * ti + hi * tr;
    hr = nr;
  }
  return make_double2(hr, hi);
}

template <typename R>
__device__ __forceinline__ void cmul(R& x, R& y, const double2 h) {
  const double a = (double)x, b = (double)y;
  x = (R)(a * h.x - b * h.y);
  y = (R)(a * h.y + b * h.x);
}

// spec: [batch][nf] complex (C = double2 or float2), multiplied in place.  With float2 a slot is two bins, and a row
// that starts at an odd element (nf odd, odd row) has lead = 1; the slot is loaded as it is stored, whole or one bin.
template <typename C>
__global__ void __launch_bounds__(kThreads)
    spec_rows_mul(C* __restrict__ spec, const SpecTerm* __restrict__ terms, const int32_t* __restrict__ counts,
                  int64_t nf, uint32_t blocks_per_row, double scale) {
  constexpr int V = 16 / sizeof(C);   // bins per slot
  const auto [row, blk] = row_block(blocks_per_row);
  const int T = counts[row];
  const SpecTerm* __restrict__ tt = terms + (size_t)row * kMaxTerms;
  const int64_t base = (int64_t)row * nf;
  const int64_t lead = base & (V - 1);
  C* __restrict__ rowp = spec + base;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int64_t slot = ((int64_t)blk * kSlots + u) * kThreads + threadIdx.x;
    const int64_t k0 = slot * V - lead;   // first bin of the slot (-1: the bin before the row)
    if (k0 >= nf) break;
    if constexpr (V == 1) {
      double2 v = rowp[k0];
      cmul(v.x, v.y, row_transfer(tt, T, (double)k0, scale));
      rowp[k0] = v;
    } else {
      const bool first = k0 >= 0, second = k0 + 1 < nf;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (first && second) {
        v = *reinterpret_cast<const float4*>(rowp + k0);
      } else if (first) {
        const float2 a = rowp[k0];
        v.x = a.x; v.y = a.y;
      } else {
        const float2 a = rowp[k0 + 1];
        v.z = a.x; v.w = a.y;
      }
      if (first) cmul(v.x, v.y, row_transfer(tt, T, (double)k0, scale));
      if (second) cmul(v.z, v.w, row_transfer(tt, T, (double)(k0 + 1), scale));
      if (first && second)
        *reinterpret_cast<float4*>(rowp + k0) = v;
      else if (first)
        rowp[k0] = make_float2(v.x, v.y);
      else
        rowp[k0 + 1] = make_float2(v.z, v.w);
    }
  }
}

}  // namespace

struct wfk_spectral_rows_plan {
  int64_t n = 0, nf = 0;
  int32_t batch = 0, kind = 0;
  uint32_t blocks_per_row = 0;
  size_t terms_off = 0, counts_off = 0;
  DevBuf<char> tables;    // SpecTerm [batch][kMaxTerms], int32 counts [batch]
  RocfftRows fft;         // its staging rows take the C2R output too when out_stride != n
};

extern "C" {

int wfk_spectral_rows_phase_step(double tau, double sample_rate, int64_t n, double* hi_out, double* lo_out) {
  if (!hi_out || !lo_out || n < 1) return wfk_fail(WFK_EINVAL, "bad phase step arguments");
  phase_step(tau, sample_rate, n, hi_out, lo_out);
  return WFK_OK;
}

int wfk_spectral_rows_plan_destroy(wfk_spectral_rows_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_spectral_rows_plan_create(int64_t n, int32_t batch, int kind, double sample_rate,
                                  const wfk_spec_term* terms_host, const int32_t* n_terms_per_row_host,
                                  wfk_spectral_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 1 || batch < 1 || !n_terms_per_row_host) return wfk_fail(WFK_EINVAL, "bad spectral rows plan arguments");
  if (const int rc = wfk_check_kind(kind)) return rc;
  if (!std::isfinite(sample_rate) || sample_rate <= 0) return wfk_fail(WFK_EINVAL, "sample_rate must be positive");
  const int64_t nf = n / 2 + 1;
  const int V = 8 / (int)wfk_elem_size(kind);   // bins per slot
  uint32_t bpr = 0;
  if (const int rc = wfk_row_blocks("spectral rows plan", nf, V * kThreads * kSlots, V - 1, batch, &bpr)) return rc;
  std::vector<SpecTerm> terms((size_t)batch * kMaxTerms, SpecTerm{0, 0, 0, 0, 0, 0});
  std::vector<int32_t> counts(n_terms_per_row_host, n_terms_per_row_host + batch);
  const wfk_spec_term* src = terms_host;
  for (int32_t r = 0; r < batch; ++r) {
    if (counts[r] < 0 || counts[r] > kMaxTerms)
      return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": " + std::to_string(counts[r]) +
                                      " terms, a row takes 0 .. " + std::to_string(kMaxTerms));
    if (counts[r] > 0 && !terms_host) return wfk_fail(WFK_EINVAL, "null terms");
    for (int32_t t = 0; t < counts[r]; ++t, ++src) {
      SpecTerm& d = terms[(size_t)r * kMaxTerms + t];
      if (src->kind != WFK_SPEC_REFLECT && src->kind != WFK_SPEC_CORRECT && src->kind != WFK_SPEC_DELAY)
        return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": unknown term kind");
      if (!std::isfinite(src->tau)) return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": tau is not finite");
      d.kind = src->kind;
      phase_step(src->tau, sample_rate, n, &d.c_hi, &d.c_lo);
      if (src->kind == WFK_SPEC_DELAY) continue;
      if (!(std::fabs(src->A) < 1.0))      // (A = 1: the reference divides by zero; |A| > 1: no stable reflection)
        return wfk_fail(WFK_EINVAL, "row " + std::to_string(r) + ": a reflection needs |A| < 1");
      d.a = src->A;
      d.g = src->kind == WFK_SPEC_REFLECT ? 1.0 - src->A : 1.0 / (1.0 - src->A);
    }
  }
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_spectral_rows_plan> p(new wfk_spectral_rows_plan());
  p->n = n; p->nf = nf; p->batch = batch; p->kind = kind;
  p->blocks_per_row = bpr;
  DevTables tab;
  p->terms_off = tab.add(terms);
  p->counts_off = tab.add(counts);
  if (!(p->fft.create(n, batch, kind) && p->tables.alloc(tab.total()) && tab.upload(p->tables.get()))) {
    (void)hipGetLastError();
    return wfk_fft_fail("spectral rows plan");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the spectral rows plan");
}

int wfk_spectral_rows_apply(wfk_spectral_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                            int64_t out_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (const int rc = wfk_check_rows("spectral rows", p->n, wfk_elem_size(p->kind), in_dev, p->batch, in_stride, out_dev,
                                    p->batch, out_stride))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  RocfftRows& f = p->fft;
  // the transforms work on contiguous rows the plan owns: the caller's input stays intact (or is `out`), any stride
  if (!(f.set_stream(s) && f.stage(in_dev, in_stride, p->batch) && f.forward())) return wfk_fft_fail("spectral rows");
  const dim3 grid(p->blocks_per_row * (uint32_t)p->batch);
  const SpecTerm* terms = DevTables::at<const SpecTerm>(p->tables.get(), p->terms_off);
  const int32_t* counts = DevTables::at<const int32_t>(p->tables.get(), p->counts_off);
  if (p->kind == WFK_OUT_F32)
    hipLaunchKernelGGL(spec_rows_mul<float2>, grid, dim3(kThreads), 0, s, (float2*)f.spec(), terms, counts, p->nf,
                       p->blocks_per_row, 1.0 / (double)p->n);
  else
    hipLaunchKernelGGL(spec_rows_mul<double2>, grid, dim3(kThreads), 0, s, (double2*)f.spec(), terms, counts, p->nf,
                       p->blocks_per_row, 1.0 / (double)p->n);
  const bool direct = p->batch == 1 || out_stride == p->n;
  if (!(f.inverse(direct ? out_dev : (void*)f.rows()) && (direct || f.unstage(out_dev, out_stride))))
    return wfk_fft_fail("spectral rows");
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "spectral rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
