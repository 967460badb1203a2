// wfk_iir_rows.hip -- IIR stage with one cascade PER ROW: row r of a batch runs through its own
// (b, a) sections, as every flux line has its own exp-decay correction (reference:
// waveforms/distortion.py:100-185 exp_decay_filter, :298-321 predistort, :340-346 distort).
// Semantics per row are those of wfk_iir.hip (scipy.signal.lfilter / sosfilt, direct form II
// transposed, state layout of scipy's zi):  out[r] = F_r(in[r] - initial[r]) + initial[r].
//
// Execution form: a workgroup of 256 lanes OWNS a row and walks it tile by tile
// (256 lanes x 16 samples) through LDS; no workgroup ever waits for another one.
//   1. the tile is loaded as whole lines (the loads of tile t+1 are in flight while tile t is
//      filtered) and laid out in LDS so that lane l finds its RUN of 16 consecutive samples at
//      l * 17 elements (odd pitch in elements: 32 lanes of a ds_read_b64 / b32 group hit 32 distinct banks);
//   2. every lane sweeps its run from a ZERO state -> local end state f_l; the 64 lanes of a
//      wave scan them, v_l = sum_{j<=l} T^(l-j) f_j (T = the row's own 16-step transition
//      matrix, T^(2^k) tables), and each wave leaves its total in LDS;
//   3. state at the wave's start: S_0 = carry of the previous tile, S_(w+1) = total_w + T^64 S_w
//      (wave w evaluates its own chain; the last wave also produces the next carry);
//   4. the lanes replay their run from LDS with the true start state v_(l-1) + T^l S_w, write y
//      over x in LDS, and the tile is stored as whole lines.
// x is read once and y written once (16 B/sample fp64, 8 fp32).  Everything is evaluated in a
// fixed order: two runs are bitwise identical, and a row's result does not depend on its
// position in the batch.
// Accuracy: poles of exp-decay corrections sit at 1 - 1e-3 .. 1 - 1e-5, where T is far from
// normal (entries that cancel against each other).  As in wfk_iir.hip the tables are computed
// in __float128 on the host, stored as (hi, lo) pairs and applied in double-double, so that a
// run boundary perturbs the state no more than one step of the sequential filter does.  State
// is always double, also for float rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "wfk.h"
#include "wfk_iir_common.h"
#include "wfk_iir_rows_dev.h"

#define IRW_LOADS_INPUT          // for wfk_iir_rows_head.inc: this file's kernel loads its tiles (it holds T^lane, has x)
#define IRW_STORE_INC "wfk_iir_rows_store.inc"   // for wfk_iir_rows_body.inc: the tile is stored as T, whole lines

namespace {

template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) iir_rows_tile(const T* in, int64_t in_stride, T* out,
                                                             int64_t out_stride, const double* __restrict__ tab,
                                                             const double* __restrict__ zi, double* __restrict__ zf,
                                                             const double* __restrict__ initial, int64_t n) {
#include "wfk_iir_rows_head.inc"

  T nxt[IRW_RUN];
  auto fetch = [&](int64_t t) {
    const int64_t base = t * IRW_TILE, left = n - base;
    if (left >= IRW_TILE) {       // (a whole tile loads unconditionally: all 16 loads are issued back to back)
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) nxt[i] = x[base + i * IRW_THREADS + tid];
    } else {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) {
        const int j = i * IRW_THREADS + tid;
        nxt[i] = j < left ? x[base + j] : (T)0;
      }
    }
  };
  fetch(0);
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t base = t * IRW_TILE, left = n - base;
#pragma unroll
    for (int i = 0; i < IRW_RUN; ++i) {
      const int j = i * IRW_THREADS + tid;
      tile[(j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN)] = nxt[i];
    }
    if (t + 1 < ntile) fetch(t + 1);
    __syncthreads();
    // ---- steps 2-4 on the tile in LDS: the text the evaluating kernels share
#include "wfk_iir_rows_body.inc"
  }
}

// ---- host: one row's table (wfk_iir_common.h: quad precision, (hi, lo) pairs)
// b, a: the row's normalised coefficients, sections back to back
void irw_build_row(int nsec, const int32_t* orders, const double* b, const double* a, double* dst) {
  const int ord = orders[0], D = nsec * ord, NC = nsec * (ord + 1);
  std::memcpy(dst, b, (size_t)NC * 8);
  std::memcpy(dst + NC, a, (size_t)NC * 8);
  double* pw = dst + 2 * NC;
  iir_power_tables(iir_transition(nsec, orders, b, a, D, IRW_RUN), D, 0, pw, pw + (size_t)IRW_NPW * D * D * 2);
}

}  // namespace

struct wfk_iir_rows_plan {
  int nsec = 0, ord = 0, D = 0;
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  DevBuf<double> tab;        // [batch][irw_row_doubles]
  std::string name;
};

template <typename T, int NSEC, int ORD>
static void irw_launch_t(const wfk_iir_rows_plan* p, const void* in, int64_t is, void* out, int64_t os,
                         const double* zi, double* zf, const double* initial, hipStream_t s) {
  hipLaunchKernelGGL((iir_rows_tile<T, NSEC, ORD>), dim3((unsigned)p->batch), dim3(IRW_THREADS), 0, s,
                     (const T*)in, is, (T*)out, os, p->tab.get(), zi, zf, initial, p->n);
}

template <typename T>
static int irw_launch(const wfk_iir_rows_plan* p, const void* in, int64_t is, void* out, int64_t os,
                      const double* zi, double* zf, const double* initial, hipStream_t s) {
#define IRW_CASE(NS, OD) \
  if (p->nsec == NS && p->ord == OD) { irw_launch_t<T, NS, OD>(p, in, is, out, os, zi, zf, initial, s); return WFK_OK; }
  IRW_CASE(1, 1) IRW_CASE(1, 2) IRW_CASE(1, 3) IRW_CASE(1, 4)           // lfilter on a combined (b, a): predistort
  IRW_CASE(2, 1) IRW_CASE(3, 1) IRW_CASE(4, 1)                          // cascades of first-order corrections
  IRW_CASE(2, 2)                                                        // two biquads
#undef IRW_CASE
  return wfk_fail(WFK_EINVAL, "per-row IIR: no kernel for this shape");
}

extern "C" {

int wfk_iir_rows_plan_destroy(wfk_iir_rows_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_iir_rows_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows, const double* a_rows,
                             int64_t n, int32_t batch, int kind, wfk_iir_rows_plan** out) {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (n_sections < 1 || !orders || !b_rows || !a_rows || n < 0 || batch < 1)
    return wfk_fail(WFK_EINVAL, "bad per-row IIR arguments");
  if (const int rc = wfk_check_kind(kind, "IIR ")) return rc;
  bool equal = true;
  int64_t Dtot = 0;
  for (int s = 0; s < n_sections; ++s) {
    if (orders[s] < 0) return wfk_fail(WFK_EINVAL, "negative section order");
    equal = equal && orders[s] == orders[0];
    Dtot += orders[s];
  }
  const int ord = orders[0];
  if (!equal || ord < 1 || Dtot > IRW_MAXD || (ord == 2 && n_sections > 2))
    return wfk_fail(WFK_EUNSUP,
                 "per-row IIR cascades take sections of EQUAL order >= 1 with a total state dimension <= " +
                     std::to_string(IRW_MAXD) + " (one section of order 1..4, 1..4 first-order sections, one or two "
                     "biquads); got " + std::to_string(n_sections) + " section(s), state dimension " +
                     std::to_string((long long)Dtot) + (equal ? "" : ", mixed orders"));
  const int NC = n_sections * (ord + 1);
  // scipy normalises every section by its a[0]
  std::vector<double> bn((size_t)batch * NC), an((size_t)batch * NC);
  for (int64_t r = 0; r < batch; ++r)
    for (int s = 0; s < n_sections; ++s) {
      const size_t at = (size_t)r * NC + (size_t)s * (ord + 1);
      const double a0 = a_rows[at];
      if (!(a0 != 0.0) || !std::isfinite(a0))
        return wfk_fail(WFK_EINVAL, "a[0] must be finite and non-zero (row " + std::to_string((long long)r) + ")");
      for (int i = 0; i <= ord; ++i) {
        bn[at + i] = b_rows[at + i] / a0;
        an[at + i] = a_rows[at + i] / a0;
      }
    }
  if (!wfk_have_device()) return wfk_fail(WFK_EHIP, "no HIP device visible");
  std::unique_ptr<wfk_iir_rows_plan> p(new wfk_iir_rows_plan());
  p->nsec = n_sections; p->ord = ord; p->D = (int)Dtot;
  p->n = n; p->batch = batch; p->kind = kind;
  p->name = std::string("iir_rows_tile<") + (kind == WFK_OUT_F64 ? "f64" : "f32") + "," + std::to_string(n_sections) +
            "," + std::to_string(ord) + ">";
  // one table per row, built on a few host threads (quad arithmetic: ~0.3 ms per row of state dimension 4)
  const size_t rd = (size_t)irw_row_doubles(n_sections, ord);
  std::vector<double> tab((size_t)batch * rd);
  {
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<unsigned>(hw ? hw : 1u, 16u);
    nt = std::max(1, std::min<int>(nt, batch / 16));
    std::atomic<int64_t> next(0);
    auto work = [&]() {
      for (;;) {
        const int64_t r0 = next.fetch_add(16);
        if (r0 >= batch) return;
        for (int64_t r = r0; r < std::min<int64_t>(r0 + 16, batch); ++r)
          irw_build_row(n_sections, orders, bn.data() + (size_t)r * NC, an.data() + (size_t)r * NC,
                        tab.data() + (size_t)r * rd);
      }
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; ++i) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
  }
  if (!p->tab.upload(tab)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "per-row IIR plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
}

int wfk_iir_rows_state_dim(const wfk_iir_rows_plan* p) { return p ? p->D : WFK_EINVAL; }

const char* wfk_iir_rows_kernel_name(const wfk_iir_rows_plan* p) { return p ? p->name.c_str() : ""; }

const double* wfk_internal_iir_rows_table(const wfk_iir_rows_plan* p) { return p ? p->tab.get() : nullptr; }

int wfk_iir_rows_apply(wfk_iir_rows_plan* p, const void* in_dev, int64_t in_stride, void* out_dev,
                       int64_t out_stride, const double* zi_dev, double* zf_dev, const double* initial_dev,
                       void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;
  if (const int rc = wfk_check_rows("per-row IIR", p->n, p->kind == WFK_OUT_F64 ? 8 : 4, in_dev, p->batch, in_stride,
                                    out_dev, p->batch, out_stride))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const int rc = p->kind == WFK_OUT_F64
                     ? irw_launch<double>(p, in_dev, in_stride, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s)
                     : irw_launch<float>(p, in_dev, in_stride, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s);
  if (rc != WFK_OK) return rc;
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "per-row IIR launch failed");
  return WFK_OK;
}

int wfk_iir_rows_apply_shared_in(wfk_iir_rows_plan* p, const void* in_dev, void* out_dev, int64_t out_stride,
                                 const double* zi_dev, double* zf_dev, const double* initial_dev,
                                 void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;
  // every row reads the one input row (an extent of one row) while other rows are already being written: no overlap
  if (const int rc = wfk_check_rows("per-row IIR, shared input", p->n, p->kind == WFK_OUT_F64 ? 8 : 4, in_dev, 1, p->n,
                                    out_dev, p->batch, out_stride, true))
    return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const int rc = p->kind == WFK_OUT_F64
                     ? irw_launch<double>(p, in_dev, 0, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s)
                     : irw_launch<float>(p, in_dev, 0, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s);
  if (rc != WFK_OK) return rc;
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "per-row IIR launch failed");
  return WFK_OK;
}

}  // extern "C"
