// wfk_extract_rows.hip -- the reference's extractKernel(sig_in, sig_out, sample_rate, bw, skip) (distortion.py:42-48)
// for a batch of rows, fp64.  Per row of n real samples:
//   R[k] = rfft(sig_in)[k] / rfft(sig_out)[k] / n,  k = 0 .. n/2     extract_ratio, over the R2C output of sig_out
//   c    = irfft(R, n)                                               rocFFT C2R into the plan's staging buffer
//   s[i] = c[(i + n/2) mod n]                                        ifftshift                       }
//   t[i] = sum_m g[m] s[i + (M - 1)/2 - m],  s = 0 outside [0, n)    np.convolve(s, g, 'same'), M <= n } extract_smooth,
//   out[j] = t[j + skip],  0 <= j < K = max(n - 2 skip, 0)           the crop                        } one pass
// (the full complex FFT of a real signal is Hermitian: the real transforms hold the same numbers).  Without taps
// (M = 0) t = s and the last pass only moves values, bit for bit.
//
// extract_ratio.  Fin / Fout as Fin conj(Fout) / |Fout|^2, one division per bin, 1/n folded in, written over the
// spectrum of sig_out.  A sig_in shared by all rows is transformed once and read at `bin` by every row.  Geometry as
// spec_rows_mul: flat grid, a workgroup never straddles rows, a thread owns kSlots 16-B slots (one bin each) kThreads
// apart.  A zero bin of sig_out gives inf / NaN and with it a row that is not finite, as in the reference.
//
// extract_smooth.  A workgroup owns kTile consecutive outputs of one row; a lane owns kSlots 16-B slots of them,
// kThreads slots apart, laid out from the 16-B boundary at or before the first sample of the OUTPUT row (as
// shift_rows: rows may be windows of a wider buffer), stored whole where they lie inside the row and element by
// element at its two ends.  The two bodies are chosen by a scalar branch on M.
//   copy body: out[j] = c[(j + skip + n/2) mod n], element loads (the rotation misaligns source and destination).
//   smoothing body: the taps are walked in blocks of at most kTapBlock.  For a block [m0, m0 + mb) the workgroup
//   stages s[base .. base + cnt + mb - 1) into LDS, base = (tile's first i) + (M - 1)/2 - m0 - mb + 1: rotation and
//   zero fill are resolved here, once per staged sample.  Output o of the tile and tap m0 + u then read LDS[o + mb -
//   1 - u]: a lane's two outputs share all but one of their samples, so a tap costs one ds_read_b64 per slot (lane
//   stride 16 B: two lanes of a 32-lane group per bank, the price of storing 16 B per lane; the LDS image is linear,
//   there is no padding that would help a unit-stride walk).  g[m] sits at a wave-uniform address of a read-only
//   array: scalar loads.  Every output adds its products in ascending m, one rounded product and one rounded sum each
//   (contraction off), whatever the tile, the row or the batch: reproducible.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_rocfft.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;                  // threads per workgroup
constexpr int kSlots = 4;                      // 16-B slots per thread, kThreads slots apart
constexpr int kTile = kThreads * kSlots * 2;   // outputs of one extract_smooth workgroup
constexpr int kTapBlock = 1024;                // taps per LDS pass: the halo is at most kTapBlock - 1 samples
constexpr int kLds = kTile + kTapBlock;        // doubles of LDS (24 KiB): tile + halo, one spare

// spec: [batch][nf] the transform of sig_out, overwritten with the ratio; fin: [in_rows][nf], in_rows 1 or batch
__global__ void __launch_bounds__(kThreads)
    extract_ratio(double2* __restrict__ spec, const double2* __restrict__ fin, int64_t fin_row_stride, int64_t nf,
                  uint32_t blocks_per_row, double scale) {
  const uint32_t row = blockIdx.x / blocks_per_row, blk = blockIdx.x - row * blocks_per_row;
  double2* __restrict__ fo = spec + (int64_t)row * nf;
  const double2* __restrict__ fi = fin + (int64_t)row * fin_row_stride;
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int64_t k = ((int64_t)blk * kSlots + u) * kThreads + threadIdx.x;
    if (k >= nf) break;
    const double2 a = fi[k], b = fo[k];
    const double d = b.x * b.x + b.y * b.y;
    double2 r;
    r.x = (a.x * b.x + a.y * b.y) / d * scale;
    r.y = (a.y * b.x - a.x * b.y) / d * scale;
    fo[k] = r;
  }
}

// the two outputs of the slot at output sample j0: whole where the slot lies inside [0, K)
__device__ __forceinline__ void store_slot(double* __restrict__ y, int64_t K, int64_t j0, double v0, double v1) {
  if (j0 >= 0 && j0 + 2 <= K) {
    *reinterpret_cast<double2*>(y + j0) = make_double2(v0, v1);
  } else {
    if (j0 >= 0 && j0 < K) y[j0] = v0;
    if (j0 + 1 >= 0 && j0 + 1 < K) y[j0 + 1] = v1;
  }
}

// c: [batch][n] contiguous, the C2R output; out: [batch] rows of K samples, out_stride elements apart
__global__ void __launch_bounds__(kThreads)
    extract_smooth(const double* __restrict__ c, double* __restrict__ out, int64_t out_stride,
                   const double* __restrict__ taps, int32_t M, int64_t n, int64_t skip, int64_t K,
                   uint32_t blocks_per_row) {
  __shared__ double lds[kLds];
  const uint32_t row = blockIdx.x / blocks_per_row, blk = blockIdx.x - row * blocks_per_row;
  const double* __restrict__ x = c + (int64_t)row * n;
  double* __restrict__ y = out + (int64_t)row * out_stride;
  const int64_t lead = (int64_t)((reinterpret_cast<uintptr_t>(y) / sizeof(double)) & 1);
  const int64_t first = (int64_t)blk * kTile - lead;   // the tile's first output sample (-1: the one before the row)
  if (first >= K) return;
  const int64_t half = n / 2;
  if (M == 0) {
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int64_t j0 = first + ((int64_t)u * kThreads + threadIdx.x) * 2;
      if (j0 >= K) break;
      double v[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int64_t j = j0 + e;
        int64_t src = j + skip + half;   // j + skip < n, so src < 2 n
        if (src >= n) src -= n;
        v[e] = (j >= 0 && j < K) ? x[src] : 0.0;
      }
      store_slot(y, K, j0, v[0], v[1]);
    }
    return;
  }
  // outputs the tile holds, rounded up to whole slots: what is staged and summed
  const int64_t left = K - first;
  const int cnt = left >= kTile ? kTile : (int)((left + 1) & ~(int64_t)1);
  const int64_t centre = (int64_t)((M - 1) / 2);
  double a0[kSlots], a1[kSlots];
#pragma unroll
  for (int u = 0; u < kSlots; ++u) a0[u] = a1[u] = 0.0;
  for (int32_t m0 = 0; m0 < M; m0 += kTapBlock) {
    const int mb = M - m0 < kTapBlock ? M - m0 : kTapBlock;
    const int64_t base = first + skip + centre - m0 - mb + 1;   // s index of lds[0]
    const int staged = cnt + mb - 1;                            // <= kTile + kTapBlock - 1 < kLds
    if (m0) __syncthreads();                                    // the block before has been read
    for (int q = threadIdx.x; q < staged; q += kThreads) {
      const int64_t i = base + q;
      double v = 0.0;
      if (i >= 0 && i < n) {
        int64_t src = i + half;
        if (src >= n) src -= n;
        v = x[src];
      }
      lds[q] = v;
    }
    __syncthreads();
    const double* __restrict__ g = taps + m0;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int o0 = (u * kThreads + (int)threadIdx.x) * 2;
      if (o0 >= cnt) break;
      double s0 = a0[u], s1 = a1[u];
      double prev = lds[o0 + mb];   // (o0 + 1) + mb - 1; o0 + mb <= cnt + mb - 2
      for (int t = 0; t < mb; ++t) {
        const double gm = g[t];
        const double cur = lds[o0 + mb - 1 - t];
        s0 = s0 + gm * cur;
        s1 = s1 + gm * prev;
        prev = cur;
      }
      a0[u] = s0;
      a1[u] = s1;
    }
  }
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int o0 = (u * kThreads + (int)threadIdx.x) * 2;
    if (o0 >= cnt) break;
    store_slot(y, K, first + o0, a0[u], a1[u]);
  }
}

// rows of `width` bytes, `rows` of them, device to device; one plain copy when both sides are contiguous
bool copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t s) {
  if (rows == 1 || (dpitch == width && spitch == width))
    return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, s) == hipSuccess;
}

}  // namespace

struct wfk_extract_rows_plan {
  int64_t n = 0, nf = 0, skip = 0, K = 0;
  int32_t batch = 0, in_rows = 0, n_taps = 0;
  uint32_t ratio_bpr = 0, smooth_bpr = 0;
  // (members go in reverse order: the rocFFT plans and the execution info before the work buffer they were given)
  DevBuf<double> taps;
  DevBuf<char> tmp;        // the staged input of a forward transform (sig_out, then sig_in), then the C2R output
  DevBuf<char> spec;       // [batch][nf] the transform of sig_out, then the ratio
  DevBuf<char> spec_in;    // [in_rows][nf] the transform of sig_in
  DevBuf<char> work;
  RocfftInfo info;
  RocfftPlan fwd, fwd_one, inv;   // fwd_one: the batch-1 forward transform of a shared sig_in (batch > 1)
};

extern "C" {

int wfk_extract_rows_plan_destroy(wfk_extract_rows_plan* p) {
  delete p;
  return WFK_OK;
}

const char* wfk_extract_rows_kernel_name(const wfk_extract_rows_plan* p) {
  return p ? "extract_ratio + extract_smooth" : "";
}

int wfk_extract_rows_plan_create(int64_t n, int32_t batch, int32_t in_rows, const double* taps_host, int32_t n_taps,
                                 int64_t skip, wfk_extract_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n < 1 || batch < 1) return wfk_fail(WFK_EINVAL, "extract rows plan: n >= 1 and batch >= 1");
  if (in_rows != 1 && in_rows != batch)
    return wfk_fail(WFK_EINVAL, "extract rows plan: in_rows is 1 (one sig_in for all rows) or batch");
  if (skip < 0) return wfk_fail(WFK_EINVAL, "extract rows plan: skip must not be negative");
  if (n_taps < 0 || n_taps > n)
    return wfk_fail(WFK_EINVAL, "extract rows plan: " + std::to_string(n_taps) + " taps, a row of " +
                                    std::to_string(n) + " samples takes 0 .. n (the reference returns n_taps "
                                    "samples beyond; rows keep their length here)");
  if (n_taps > 0 && !taps_host) return wfk_fail(WFK_EINVAL, "null taps");
  for (int32_t m = 0; m < n_taps; ++m)
    if (!std::isfinite(taps_host[m])) return wfk_fail(WFK_EINVAL, "tap " + std::to_string(m) + " is not finite");
  const int64_t nf = n / 2 + 1;
  const int64_t K = skip < (n + 1) / 2 ? n - 2 * skip : 0;
  const int64_t ratio_bpr = (nf + (int64_t)kThreads * kSlots - 1) / ((int64_t)kThreads * kSlots);
  const int64_t smooth_bpr = (K + 1 + kTile - 1) / kTile;   // (+ 1: a row may start inside a slot)
  if (ratio_bpr * batch > 0x7fffffffLL || smooth_bpr * batch > 0x7fffffffLL)
    return wfk_fail(WFK_EINVAL, "extract rows plan: batch * n too large for one launch");
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_extract_rows_plan> p(new wfk_extract_rows_plan());
  p->n = n; p->nf = nf; p->skip = skip; p->K = K;
  p->batch = batch; p->in_rows = in_rows; p->n_taps = n_taps;
  p->ratio_bpr = (uint32_t)ratio_bpr;
  p->smooth_bpr = (uint32_t)smooth_bpr;
  const size_t len[1] = {(size_t)n};
  const bool shared_one = in_rows == 1 && batch > 1;
  bool ok = rocfft_plan_create(p->fwd.out(), rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                               rocfft_precision_double, 1, len, (size_t)batch, nullptr) == rocfft_status_success;
  if (ok && shared_one)
    ok = rocfft_plan_create(p->fwd_one.out(), rocfft_placement_notinplace, rocfft_transform_type_real_forward,
                            rocfft_precision_double, 1, len, 1, nullptr) == rocfft_status_success;
  ok = ok && rocfft_plan_create(p->inv.out(), rocfft_placement_notinplace, rocfft_transform_type_real_inverse,
                                rocfft_precision_double, 1, len, (size_t)batch, nullptr) == rocfft_status_success;
  if (ok) {
    size_t wbytes = 0, w = 0;
    for (rocfft_plan q : {p->fwd.get(), p->fwd_one.get(), p->inv.get()}) {
      if (!q) continue;
      rocfft_plan_get_work_buffer_size(q, &w);
      wbytes = w > wbytes ? w : wbytes;
    }
    ok = rocfft_execution_info_create(p->info.out()) == rocfft_status_success;
    if (ok && wbytes)
      ok = p->work.alloc(wbytes) &&
           rocfft_execution_info_set_work_buffer(p->info.get(), p->work.get(), wbytes) == rocfft_status_success;
    ok = ok && p->spec.alloc((size_t)batch * nf * 16);
    ok = ok && p->spec_in.alloc((size_t)in_rows * nf * 16);
    ok = ok && p->tmp.alloc((size_t)batch * n * 8);
    if (ok && n_taps) ok = p->taps.upload(taps_host, (size_t)n_taps * 8);
  }
  if (!ok) {
    (void)hipGetLastError();
    return wfk_fail(WFK_EHIP, "extract rows plan: rocFFT plan / buffer creation failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the extract rows plan");
}

int wfk_extract_rows_apply(wfk_extract_rows_plan* p, const double* sig_in_dev, int64_t in_stride,
                           const double* sig_out_dev, int64_t out_sig_stride, double* ker_dev, int64_t ker_stride,
                           void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->K == 0) return WFK_OK;   // nothing to write (the result's pointer may be null)
  if (!sig_in_dev || !sig_out_dev || !ker_dev) return wfk_fail(WFK_EINVAL, "extract rows: null buffer");
  if (((uintptr_t)sig_in_dev | (uintptr_t)sig_out_dev | (uintptr_t)ker_dev) & 7)
    return wfk_fail(WFK_EINVAL, "extract rows: rows are not aligned to their element");
  if (in_stride < p->n || out_sig_stride < p->n || ker_stride < p->K)
    return wfk_fail(WFK_EINVAL, "extract rows: row stride smaller than the row");
  const size_t ker_bytes = wfk_rows_bytes(p->batch, ker_stride, p->K, 8);
  if (wfk_ranges_overlap(ker_dev, ker_bytes, sig_in_dev, wfk_rows_bytes(p->in_rows, in_stride, p->n, 8)) ||
      wfk_ranges_overlap(ker_dev, ker_bytes, sig_out_dev, wfk_rows_bytes(p->batch, out_sig_stride, p->n, 8)))
    return wfk_fail(WFK_EINVAL, "extract rows is out of place: the result overlaps an input");
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t width = (size_t)p->n * 8;
  if (rocfft_execution_info_set_stream(p->info.get(), s) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft set_stream failed");
  // both inputs go through the plan's own contiguous rows: they stay intact, any stride, any overlap between them
  void* tmp[1] = {p->tmp.get()};
  void* spec[1] = {p->spec.get()};
  void* spec_in[1] = {p->spec_in.get()};
  if (!copy_rows(p->tmp.get(), width, sig_out_dev, (size_t)out_sig_stride * 8, width, (size_t)p->batch, s))
    return wfk_fail(WFK_EHIP, "copy failed");
  if (rocfft_execute(p->fwd.get(), tmp, spec, p->info.get()) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft forward failed");
  if (!copy_rows(p->tmp.get(), width, sig_in_dev, (size_t)in_stride * 8, width, (size_t)p->in_rows, s))
    return wfk_fail(WFK_EHIP, "copy failed");
  const rocfft_plan fwd_in = p->fwd_one ? p->fwd_one.get() : p->fwd.get();
  if (rocfft_execute(fwd_in, tmp, spec_in, p->info.get()) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft forward failed");
  hipLaunchKernelGGL(extract_ratio, dim3(p->ratio_bpr * (uint32_t)p->batch), dim3(kThreads), 0, s,
                     (double2*)p->spec.get(), (const double2*)p->spec_in.get(),
                     p->in_rows == 1 ? (int64_t)0 : p->nf, p->nf, p->ratio_bpr, 1.0 / (double)p->n);
  if (rocfft_execute(p->inv.get(), spec, tmp, p->info.get()) != rocfft_status_success)
    return wfk_fail(WFK_EHIP, "rocfft inverse failed");
  hipLaunchKernelGGL(extract_smooth, dim3(p->smooth_bpr * (uint32_t)p->batch), dim3(kThreads), 0, s,
                     (const double*)p->tmp.get(), ker_dev, ker_stride, (const double*)p->taps.get(), p->n_taps, p->n,
                     p->skip, p->K, p->smooth_bpr);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "extract rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
