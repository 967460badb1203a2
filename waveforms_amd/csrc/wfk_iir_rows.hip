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

#define IRW_RUN 16                        // samples per lane and tile
#define IRW_THREADS 256
#define IRW_WAVES (IRW_THREADS / 64)
#define IRW_TILE (IRW_RUN * IRW_THREADS)  // 4096 samples: 34 KB of LDS in fp64, four workgroups per CU
#define IRW_PITCH (IRW_RUN + 1)           // elements between the runs of neighbouring lanes
#define IRW_MAXD 4                        // state dimension limit
#define IRW_NPW 7                         // T^(2^k), k = 0 .. 6 (k = 6: one wave)

namespace {

// per-row table (doubles): b[NC] a[NC] | pw[IRW_NPW][D][D][2] | lanep[64][D][D][2] (T^l, l = 0 .. 63)
__host__ __device__ constexpr int irw_row_doubles(int nsec, int ord) {
  return 2 * nsec * (ord + 1) + (IRW_NPW + 64) * (nsec * ord) * (nsec * ord) * 2;
}

template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) iir_rows_tile(const T* in, int64_t in_stride, T* out,
                                                             int64_t out_stride, const double* __restrict__ tab,
                                                             const double* __restrict__ zi, double* __restrict__ zf,
                                                             const double* __restrict__ initial, int64_t n) {
  constexpr int D = NSEC * ORD, NC = NSEC * (ORD + 1), MM = D * D * 2;
  __shared__ T tile[IRW_THREADS * IRW_PITCH];
  __shared__ double s_tot[IRW_WAVES][D];
  __shared__ double s_carry[2][D];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row = blockIdx.x;
  const double* rt = tab + row * (int64_t)irw_row_doubles(NSEC, ORD);   // workgroup-uniform: scalar loads
  double cb[NC], ca[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) { cb[i] = rt[i]; ca[i] = rt[NC + i]; }
  const auto B = [&](int s, int i) { return cb[s * (ORD + 1) + i]; };
  const auto A = [&](int s, int i) { return ca[s * (ORD + 1) + i]; };
  const double* pw = rt + 2 * NC;
  const double* W = pw + (IRW_NPW - 1) * MM;                            // T^64
  double L[MM];                                                         // T^lane, kept for the whole row
#pragma unroll
  for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
  const double pre = initial ? initial[row] : 0.0;
  if (tid < D) s_carry[0][tid] = zi ? zi[row * D + tid] : 0.0;
  const T* x = in + row * in_stride;
  T* y = out + row * out_stride;
  const int64_t ntile = (n + IRW_TILE - 1) / IRW_TILE;
  T* const my = tile + tid * IRW_PITCH;

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
    const int64_t mine = left - (int64_t)tid * IRW_RUN;                 // samples of the row from this lane's run on
    const int cnt = (int)(mine < 0 ? 0 : (mine > IRW_RUN ? IRW_RUN : mine));

    // ---- sweep 1: zero state -> local end state; inclusive scan over the wave
    double z[D];
#pragma unroll
    for (int i = 0; i < D; ++i) z[i] = 0.0;
    if (cnt == IRW_RUN) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) (void)iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z);
    } else {
      for (int i = 0; i < cnt; ++i) (void)iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z);
    }
    // (a lane past the end of the row keeps a zero state; the scan still multiplies by T per lane, which only
    //  matters AFTER the last sample -- nothing there is used)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int d = 1 << k;
      double u[D], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) u[i] = __shfl_up(z[i], d);
      dd_matvec_add<D>(r, z, pw + k * MM, u);
#pragma unroll
      for (int i = 0; i < D; ++i) z[i] = lane >= d ? r[i] : z[i];
    }
    double vprev[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double up = __shfl_up(z[i], 1);
      vprev[i] = lane == 0 ? 0.0 : up;
    }
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i < D; ++i) s_tot[wv][i] = z[i];
    }
    __syncthreads();

    // ---- state at this wave's start: the carry pushed through the waves before it
    double S[D];
#pragma unroll
    for (int i = 0; i < D; ++i) S[i] = s_carry[t & 1][i];
    for (int w = 0; w < wv; ++w) {
      double tot[D], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) tot[i] = s_tot[w][i];
      dd_matvec_add<D>(r, tot, W, S);
#pragma unroll
      for (int i = 0; i < D; ++i) S[i] = r[i];
    }
    if (wv == IRW_WAVES - 1) {     // the next tile's carry (double-buffered: the other waves still read this tile's)
      double r[D];
      dd_matvec_add<D>(r, z, W, S);                                    // lane 63: z = this wave's total
      if (lane == 63) {
#pragma unroll
        for (int i = 0; i < D; ++i) s_carry[(t + 1) & 1][i] = r[i];
      }
    }

    // ---- sweep 2 from the true start state v_(l-1) + T^l S_w, y over x in LDS
    dd_matvec_add<D>(z, vprev, L, S);
    if (cnt == IRW_RUN) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) my[i] = (T)(iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z) + pre);
    } else {
      for (int i = 0; i < cnt; ++i) my[i] = (T)(iir_cascade_step<NSEC, ORD>(B, A, (double)my[i] - pre, z) + pre);
    }
    if (zf && cnt > 0 && mine <= IRW_RUN) {                             // the lane that holds the row's last sample
#pragma unroll
      for (int i = 0; i < D; ++i) zf[row * D + i] = z[i];
    }
    __syncthreads();
    if (left >= IRW_TILE) {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) {
        const int j = i * IRW_THREADS + tid;
        y[base + j] = tile[(j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN)];
      }
    } else {
#pragma unroll
      for (int i = 0; i < IRW_RUN; ++i) {
        const int j = i * IRW_THREADS + tid;
        if (j < left) y[base + j] = tile[(j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN)];
      }
    }
    __syncthreads();
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
