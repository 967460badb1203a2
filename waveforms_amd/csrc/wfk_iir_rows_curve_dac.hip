// wfk_iir_rows_curve_dac.hip -- a flux line's whole back end in one kernel: the line's calibration curve
// (wfk_curve_rows.hip), its own exp-decay correction (wfk_iir_rows.hip) and the converter (wfk_dac_rows.hip), without
// the float rows between them.  Per sample
//   u = np.interp(x, xp[r], fp[r], left[r], right[r])      curve_block's statements; a float plan rounds u to float once
//   y = iir_rows_tile's result on u, as it stands in LDS after sweep 2
//   code = dac_block's statements on y
// -- the statements of the three stages in their order: codes, both reports and zf equal CurveStage followed by
// IirDacStage bit for bit.
//
// Execution form: iir_rows_dac's, to the letter (wfk_iir_rows_head.inc, wfk_iir_rows_body.inc with the codes store), plus
// wfk_iir_rows_curve_row.inc: the workgroup owns its row, so it copies the row's knots and buckets into dynamic LDS once,
// before the first tile, and every sample goes through the curve where it is in a register -- nxt[i], on its way into
// the tile; neighbouring lanes hold neighbouring samples there, so a smooth waveform reads the same LDS words and bisects
// to the same depth across a wave.  `beyond` is counted like the converter's counts: ballots into per-wave scalar
// counters over the row, one meeting in LDS at the row's end, three stores.  Static plus dynamic LDS stays within 64 KiB:
// the plan builds its own bucket table (curve_build, wfk_curve_dev.h), halved until the largest row fits.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_curve_dev.h"
#include "wfk_iir_common.h"
#include "wfk_iir_rows_dev.h"

#define IRW_LOADS_INPUT                              // for wfk_iir_rows_head.inc: the kernel loads its tiles, as iir_rows_tile
#define IRW_OUT_T int16_t                            // ... and its `out` rows are codes
#define IRW_STORE_INC "wfk_iir_rows_store_dac.inc"   // for wfk_iir_rows_body.inc: the tile leaves LDS as codes

namespace {

template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS)
    iir_rows_curve_dac(const T* in, int64_t in_stride, int16_t* out, int64_t out_stride, IRW_DAC_PARAMS,
                       IRW_CURVE_PARAMS, const double* __restrict__ tab, const double* __restrict__ zi,
                       double* __restrict__ zf, const double* __restrict__ initial, int64_t n) {
#include "wfk_iir_rows_head.inc"
#include "wfk_iir_rows_dac_row.inc"
#include "wfk_iir_rows_curve_row.inc"

  T nxt[IRW_RUN];
  auto fetch = [&](int64_t t) {
    const int64_t base = t * IRW_TILE, left = n - base;
    if (left >= IRW_TILE) {
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
    for (int i = 0; i < IRW_RUN; ++i)
      tile[irw_at(i * IRW_THREADS + tid)] = through_curve(nxt[i], i * IRW_THREADS + tid < left);
    if (t + 1 < ntile) fetch(t + 1);
    __syncthreads();
#include "wfk_iir_rows_body.inc"
  }
#include "wfk_iir_rows_dac_end.inc"
#include "wfk_iir_rows_curve_end.inc"
}

}  // namespace

struct wfk_curve_iir_dac_plan {
  wfk_iir_rows_plan* iir = nullptr;   // the rows' tables (irw_build_row), the shape
  int nsec = 0, ord = 0, bits = 0, shift = 0;
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  DevBuf<double> gd;                  // [batch][2]: gain, offset
  DevBuf<char> tables;                // CurveRow [batch], the knots, the buckets
  size_t rows_off = 0, knots_off = 0, buckets_off = 0, lds_bytes = 0;
  int lds_knots = 0;
  std::string name;
  ~wfk_curve_iir_dac_plan() { wfk_iir_rows_plan_destroy(iir); }
};

namespace {

template <typename T>
int icd_run(const double* tab, int nsec, int ord, int32_t batch, int64_t n, const void* in, int64_t is, int16_t* out,
            int64_t os, const double* gd, int64_t* counts, const CurveRow* crows, const double* cknots,
            const uint32_t* cbuckets, int64_t* beyond, int lds_knots, size_t lds_bytes, const double* zi, double* zf,
            const double* initial, int bits, int shift, hipStream_t s) {
  const double lo = -(double)(1 << (bits - 1)), hi = (double)((1 << (bits - 1)) - 1);
  if (lds_bytes > irw_curve_lds_budget(sizeof(T)))
    return wfk_fail(WFK_EINVAL, "per-row curve IIR dac: the curve tables exceed the kernel's LDS");
#define ICD_CASE(NS, OD)                                                                                              \
  if (nsec == NS && ord == OD) {                                                                                      \
    hipLaunchKernelGGL((iir_rows_curve_dac<T, NS, OD>), dim3((unsigned)batch), dim3(IRW_THREADS), lds_bytes, s,       \
                       (const T*)in, is, out, os, gd, (unsigned long long*)counts, lo, hi, shift, crows, cknots,      \
                       cbuckets, (unsigned long long*)beyond, lds_knots, tab, zi, zf, initial, n);                    \
    return WFK_OK;                                                                                                    \
  }
  ICD_CASE(1, 1) ICD_CASE(1, 2) ICD_CASE(1, 3) ICD_CASE(1, 4)           // the eight shapes of iir_rows_tile
  ICD_CASE(2, 1) ICD_CASE(3, 1) ICD_CASE(4, 1)
  ICD_CASE(2, 2)
#undef ICD_CASE
  return wfk_fail(WFK_EINVAL, "per-row curve IIR dac: no kernel for this shape");
}

// shared: every row reads the one input row at `in` (an extent of one row; the kernel's in_stride is 0)
int icd_apply(wfk_curve_iir_dac_plan* p, const char* stage, const void* in, bool shared, int64_t in_stride,
              int16_t* out, int64_t out_stride, int64_t* counts, int64_t* beyond, const double* zi, double* zf,
              const double* initial, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts, p->batch, 3};
  // nothing to look up or filter (the pointers of empty rows may be null): no kernel; the reports are still zeroed
  if (p->n == 0) {
    if (const int rc = curve_beyond_rule(stage, beyond, p->batch, counts, {})) return rc;
    if (const int rc = wfk_zero_report(stage, report, s)) return rc;
    return wfk_zero_report(stage, RowReport{beyond, p->batch, 3}, s);
  }
  const RowSide in_side{"in", in, shared ? 1 : p->batch, shared ? p->n : in_stride, p->n, wfk_elem_size(p->kind)};
  const RowSide out_side{"out", out, p->batch, out_stride, p->n, sizeof(int16_t), false};   // a lone code row's stride is not read
  if (const int rc = wfk_row_rule(stage, {in_side}, out_side, kRowsAligned | kRowsDisjoint, wfk_fail, report)) return rc;
  if (const int rc = curve_beyond_rule(stage, beyond, p->batch, counts, {in_side, out_side})) return rc;
  const int rc = wfk_internal_curve_iir_dac_run(
      wfk_internal_iir_rows_table(p->iir), p->nsec, p->ord, p->kind, p->batch, p->n, in, shared ? 0 : in_stride, out,
      out_stride, p->gd.get(), counts, DevTables::at<const char>(p->tables.get(), p->rows_off),
      DevTables::at<const double>(p->tables.get(), p->knots_off),
      DevTables::at<const uint32_t>(p->tables.get(), p->buckets_off), beyond, p->lds_knots, p->lds_bytes, zi, zf,
      initial, p->bits, p->shift, hip_stream);
  if (rc != WFK_OK) return rc;
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, std::string(stage) + " kernel launch failed");
  return WFK_OK;
}

}  // namespace

extern "C" {

// the launch of iir_rows_curve_dac on rows whose IIR tables, (gain, offset) pairs and curve tables (curve_build, held to
// irw_curve_lds_budget) the caller holds: this file's applies, and the two-launch route of the sampled plan
int wfk_internal_curve_iir_dac_run(const double* tab, int nsec, int ord, int kind, int32_t batch, int64_t n,
                                   const void* in, int64_t in_stride, int16_t* out, int64_t out_stride, const double* gd,
                                   int64_t* counts, const void* curve_rows, const double* curve_knots,
                                   const uint32_t* curve_buckets, int64_t* beyond, int lds_knots, size_t lds_bytes,
                                   const double* zi, double* zf, const double* initial, int bits, int shift,
                                   void* hip_stream) {
  hipStream_t s = (hipStream_t)hip_stream;
  const CurveRow* crows = (const CurveRow*)curve_rows;
  return kind == WFK_OUT_F32
             ? icd_run<float>(tab, nsec, ord, batch, n, in, in_stride, out, out_stride, gd, counts, crows, curve_knots,
                              curve_buckets, beyond, lds_knots, lds_bytes, zi, zf, initial, bits, shift, s)
             : icd_run<double>(tab, nsec, ord, batch, n, in, in_stride, out, out_stride, gd, counts, crows, curve_knots,
                               curve_buckets, beyond, lds_knots, lds_bytes, zi, zf, initial, bits, shift, s);
}

int wfk_curve_iir_dac_plan_destroy(wfk_curve_iir_dac_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_curve_iir_dac_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows, const double* a_rows,
                                  int64_t n, int32_t batch, int kind, const int64_t* knot_ptr, const double* xp,
                                  const double* fp, const double* left, const double* right, const double* gain,
                                  const double* offset, int bits, int shift, wfk_curve_iir_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  // the curve's refusals, then the converter's, then the cascades': all before any device work
  if (const int rc = curve_check(n, batch, kind, knot_ptr, xp, fp)) return rc;
  if (!gain || !offset) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  if (const int rc = wfk_internal_dac_check(batch, gain, offset, bits, shift, 1)) return rc;
  std::unique_ptr<wfk_curve_iir_dac_plan> p(new wfk_curve_iir_dac_plan());
  if (const int rc = wfk_iir_rows_plan_create(n_sections, orders, b_rows, a_rows, n, batch, kind, &p->iir)) return rc;
  p->nsec = n_sections; p->ord = orders[0];
  p->bits = bits; p->shift = shift;
  p->n = n; p->batch = batch; p->kind = kind;
  p->name = std::string("iir_rows_curve_dac<") + (kind == WFK_OUT_F64 ? "f64" : "f32") + "," +
            std::to_string(n_sections) + "," + std::to_string(p->ord) + ">";
  const CurveTables ct = curve_build(batch, knot_ptr, xp, fp, left, right, true, irw_curve_lds_budget(wfk_elem_size(kind)));
  p->lds_knots = ct.max_k;
  p->lds_bytes = ct.lds_bytes();
  DevTables tab;
  p->rows_off = tab.add(ct.rows);
  p->knots_off = tab.add(ct.knots);
  p->buckets_off = tab.add(ct.buckets);
  if (const int rc = wfk_upload_tables("per-row curve IIR dac plan", tab, p->tables)) return rc;
  std::vector<double> gd((size_t)batch * 2);
  for (int32_t r = 0; r < batch; ++r) { gd[2 * (size_t)r] = gain[r]; gd[2 * (size_t)r + 1] = offset[r]; }
  if (!p->gd.upload(gd)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "per-row curve IIR dac plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the per-row curve IIR dac plan");
}

int wfk_curve_iir_dac_state_dim(const wfk_curve_iir_dac_plan* p) { return p ? wfk_iir_rows_state_dim(p->iir) : WFK_EINVAL; }

const char* wfk_curve_iir_dac_kernel_name(const wfk_curve_iir_dac_plan* p) { return p ? p->name.c_str() : ""; }

int wfk_curve_iir_dac_apply(wfk_curve_iir_dac_plan* p, const void* in_dev, int64_t in_stride, int16_t* out_dev,
                            int64_t out_stride, int64_t* counts_dev, int64_t* beyond_dev, const double* zi_dev,
                            double* zf_dev, const double* initial_dev, void* hip_stream) {
  return icd_apply(p, "per-row curve IIR dac", in_dev, false, in_stride, out_dev, out_stride, counts_dev, beyond_dev,
                   zi_dev, zf_dev, initial_dev, hip_stream);
}

int wfk_curve_iir_dac_apply_shared_in(wfk_curve_iir_dac_plan* p, const void* in_dev, int16_t* out_dev,
                                      int64_t out_stride, int64_t* counts_dev, int64_t* beyond_dev,
                                      const double* zi_dev, double* zf_dev, const double* initial_dev,
                                      void* hip_stream) {
  return icd_apply(p, "per-row curve IIR dac, shared input", in_dev, true, 0, out_dev, out_stride, counts_dev,
                   beyond_dev, zi_dev, zf_dev, initial_dev, hip_stream);
}

}  // extern "C"
