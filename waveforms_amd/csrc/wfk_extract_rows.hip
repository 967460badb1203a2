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
// spectrum of sig_out.  A sig_in shared by all rows is transformed once and read at `bin` by every row.  A row-slot
// kernel (wfk_rows_dev.h) whose slots are one bin each and start at the row (no lead).  A zero bin of sig_out gives
// inf / NaN and with it a row that is not finite, as in the reference.
//
// extract_smooth.  A row-slot kernel over the OUTPUT rows: a workgroup owns kTile consecutive outputs of one row.  The
// two bodies are chosen by a scalar branch on M.
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
#include "wfk_rows_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = kThreads * kSlots * 2;   // outputs of one extract_smooth workgroup
constexpr int kTapBlock = 1024;                // taps per LDS pass: the halo is at most kTapBlock - 1 samples
constexpr int kLds = kTile + kTapBlock;        // doubles of LDS (24 KiB): tile + halo, one spare

// spec: [batch][nf] the transform of sig_out, overwritten with the ratio; fin: [in_rows][nf], in_rows 1 or batch
__global__ void __launch_bounds__(kThreads)
    extract_ratio(double2* __restrict__ spec, const double2* __restrict__ fin, int64_t fin_row_stride, int64_t nf,
                  uint32_t blocks_per_row, double scale) {
  const auto [row, blk] = row_block(blocks_per_row);
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

// store_slot of wfk_rows_dev.h for a pair of doubles, in this kernel's own spelling: under the shared one the compiler
// lays the two branches out the other way round, and the machine code is kept as it was
__device__ __forceinline__ void store_pair(double* __restrict__ y, int64_t K, int64_t j0, double v0, double v1) {
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
  const auto [row, blk] = row_block(blocks_per_row);
  const double* __restrict__ x = c + (int64_t)row * n;
  double* __restrict__ y = out + (int64_t)row * out_stride;
  const int64_t lead = row_lead(y);
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
      store_pair(y, K, j0, v[0], v[1]);
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
    store_pair(y, K, first + o0, a0[u], a1[u]);
  }
}

}  // namespace

struct wfk_extract_rows_plan {
  int64_t n = 0, nf = 0, skip = 0, K = 0;
  int32_t batch = 0, in_rows = 0, n_taps = 0;
  uint32_t ratio_bpr = 0, smooth_bpr = 0;
  DevBuf<double> taps;
  // staging rows: sig_out, then sig_in, then the C2R output; spec: the transform of sig_out, then the ratio; spec2:
  // [in_rows][nf] the transform of sig_in, by a batch-1 forward plan of its own when it is shared (batch > 1)
  RocfftRows fft;
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
  uint32_t ratio_bpr = 0, smooth_bpr = 0;
  if (const int rc = wfk_row_blocks("extract rows plan", nf, kThreads * kSlots, 0, batch, &ratio_bpr)) return rc;
  if (const int rc = wfk_row_blocks("extract rows plan", K, kTile, 1, batch, &smooth_bpr)) return rc;
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  wfk_rocfft_setup_once();
  std::unique_ptr<wfk_extract_rows_plan> p(new wfk_extract_rows_plan());
  p->n = n; p->nf = nf; p->skip = skip; p->K = K;
  p->batch = batch; p->in_rows = in_rows; p->n_taps = n_taps;
  p->ratio_bpr = ratio_bpr;
  p->smooth_bpr = smooth_bpr;
  if (!(p->fft.create(n, batch, WFK_OUT_F64, in_rows) && (!n_taps || p->taps.upload(taps_host, (size_t)n_taps * 8)))) {
    (void)hipGetLastError();
    return wfk_fft_fail("extract rows plan");
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
  if (const int rc = wfk_row_rule("extract rows",
                                  {{"sig_in", sig_in_dev, p->in_rows, in_stride, p->n, 8},
                                   {"sig_out", sig_out_dev, p->batch, out_sig_stride, p->n, 8}},
                                  {"ker", ker_dev, p->batch, ker_stride, p->K, 8}, kRowsAligned | kRowsDisjoint,
                                  wfk_fail))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  RocfftRows& f = p->fft;
  // both inputs go through the plan's own contiguous rows: they stay intact, any stride, any overlap between them
  if (!(f.set_stream(s) && f.stage(sig_out_dev, out_sig_stride, p->batch) && f.forward() &&
        f.stage(sig_in_dev, in_stride, p->in_rows) && f.forward2()))
    return wfk_fft_fail("extract rows");
  hipLaunchKernelGGL(extract_ratio, dim3(p->ratio_bpr * (uint32_t)p->batch), dim3(kThreads), 0, s,
                     (double2*)f.spec(), (const double2*)f.spec2(), p->in_rows == 1 ? (int64_t)0 : p->nf, p->nf,
                     p->ratio_bpr, 1.0 / (double)p->n);
  if (!f.inverse(f.rows())) return wfk_fft_fail("extract rows");
  hipLaunchKernelGGL(extract_smooth, dim3(p->smooth_bpr * (uint32_t)p->batch), dim3(kThreads), 0, s,
                     (const double*)f.rows(), ker_dev, ker_stride, (const double*)p->taps.get(), p->n_taps, p->n,
                     p->skip, p->K, p->smooth_bpr);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "extract rows kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
