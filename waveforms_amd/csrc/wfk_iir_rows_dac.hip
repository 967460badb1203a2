// wfk_iir_rows_dac.hip -- the per-row IIR stage (wfk_iir_rows.hip) that ends in int16 DAC codes (wfk_dac_rows.hip): the
// last float stage of a flux line without a crosstalk matrix -- its own exp-decay correction -- and the converter
// behind it in one kernel, without the float rows between them.  Per sample
//   y = iir_rows_tile's result as it stands in LDS after sweep 2 (a float plan has rounded it to float), widened
//   v = fl(fl(y * gain[r]) + offset[r]);  q = rint(v);  c = 0 if v is NaN, lo if q < lo, hi if q > hi, else q
//   code = (int)c << shift as int16
// -- the statements of iir_rows_tile and of dac_block, in their order: codes, counts and zf equal the two launches bit
// for bit.  The converter lines run without a fused multiply-add (their own scope in wfk_iir_rows_store_dac.inc); the
// IIR arithmetic is the shared text, contracted as it is in iir_rows_tile.
//
// Execution form: iir_rows_tile's, to the letter (the row head, the tile loads with the next tile in flight, the body's
// sweeps, scan and carry chain: wfk_iir_rows_head.inc, wfk_iir_rows_body.inc) up to the store section, which the body
// takes from IRW_STORE_INC: here wfk_iir_rows_store_dac.inc.  8 B read and 2 B written per sample in fp64 (4 + 2 in
// fp32) instead of 8 + 8 + 8 + 2.  A workgroup owns its row, so it also owns the row's three counters: every wave counts
// in scalar registers over the whole row, the waves' sums meet in LDS once, at the end of the row, and are STORED -- no
// atomic, no zeroing launch in front, a `counts` full of garbage comes out exact.  counts == nullptr: no counting (a
// workgroup-uniform test, not another instantiation).
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_iir_common.h"
#include "wfk_iir_rows_dev.h"

#define IRW_LOADS_INPUT                              // for wfk_iir_rows_head.inc: the kernel loads its tiles, as iir_rows_tile
#define IRW_OUT_T int16_t                            // ... and its `out` rows are codes
#define IRW_STORE_INC "wfk_iir_rows_store_dac.inc"   // for wfk_iir_rows_body.inc: the tile leaves LDS as codes

namespace {

// IRW_DAC_PARAMS (wfk_iir_rows_dev.h): the rows' gains and offsets, the counts or null, the rails.  Row strides in
// elements of their own side; in_stride = 0: every row reads the one input row.
template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS)
    iir_rows_dac(const T* in, int64_t in_stride, int16_t* out, int64_t out_stride, IRW_DAC_PARAMS,
                 const double* __restrict__ tab, const double* __restrict__ zi, double* __restrict__ zf,
                 const double* __restrict__ initial, int64_t n) {
#include "wfk_iir_rows_head.inc"
#include "wfk_iir_rows_dac_row.inc"

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
    for (int i = 0; i < IRW_RUN; ++i) tile[irw_at(i * IRW_THREADS + tid)] = nxt[i];
    if (t + 1 < ntile) fetch(t + 1);
    __syncthreads();
#include "wfk_iir_rows_body.inc"
  }
#include "wfk_iir_rows_dac_end.inc"
}

}  // namespace

struct wfk_iir_rows_dac_plan {
  wfk_iir_rows_plan* iir = nullptr;   // the rows' tables (irw_build_row), the shape, the name's suffix
  int nsec = 0, ord = 0, bits = 0, shift = 0;
  int64_t n = 0;
  int32_t batch = 0, kind = 0;
  DevBuf<double> gd;                  // [batch][2]: gain, offset
  std::string name;
  ~wfk_iir_rows_dac_plan() { wfk_iir_rows_plan_destroy(iir); }
};

namespace {

template <typename T>
int ird_run(const double* tab, int nsec, int ord, int32_t batch, int64_t n, const void* in, int64_t is, int16_t* out,
            int64_t os, const double* gd, int64_t* counts, const double* zi, double* zf, const double* initial, int bits,
            int shift, hipStream_t s) {
  const double lo = -(double)(1 << (bits - 1)), hi = (double)((1 << (bits - 1)) - 1);
#define IRD_CASE(NS, OD)                                                                                              \
  if (nsec == NS && ord == OD) {                                                                                      \
    hipLaunchKernelGGL((iir_rows_dac<T, NS, OD>), dim3((unsigned)batch), dim3(IRW_THREADS), 0, s, (const T*)in, is,  \
                       out, os, gd, (unsigned long long*)counts, lo, hi, shift, tab, zi, zf, initial, n);             \
    return WFK_OK;                                                                                                    \
  }
  IRD_CASE(1, 1) IRD_CASE(1, 2) IRD_CASE(1, 3) IRD_CASE(1, 4)           // the eight shapes of iir_rows_tile
  IRD_CASE(2, 1) IRD_CASE(3, 1) IRD_CASE(4, 1)
  IRD_CASE(2, 2)
#undef IRD_CASE
  return wfk_fail(WFK_EINVAL, "per-row IIR dac: no kernel for this shape");
}

// shared: every row reads the one input row at `in` (an extent of one row; the kernel's in_stride is 0)
int ird_apply(wfk_iir_rows_dac_plan* p, const char* stage, const void* in, bool shared, int64_t in_stride,
              int16_t* out, int64_t out_stride, int64_t* counts, const double* zi, double* zf, const double* initial,
              void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts, p->batch, 3};
  // nothing to filter (the pointers of empty rows may be null): no kernel; the report is still zeroed
  if (p->n == 0) return wfk_zero_report(stage, report, s);
  // a lone code row's stride is not read
  if (const int rc = wfk_row_rule(stage, {{"in", in, shared ? 1 : p->batch, shared ? p->n : in_stride, p->n,
                                           wfk_elem_size(p->kind)}},
                                  {"out", out, p->batch, out_stride, p->n, sizeof(int16_t), false},
                                  kRowsAligned | kRowsDisjoint, wfk_fail, report))
    return rc;
  const int64_t is = shared ? 0 : in_stride;
  const int rc = wfk_internal_iir_rows_dac_run(wfk_internal_iir_rows_table(p->iir), p->nsec, p->ord, p->kind, p->batch,
                                               p->n, in, is, out, out_stride, p->gd.get(), counts, zi, zf, initial,
                                               p->bits, p->shift, hip_stream);
  if (rc != WFK_OK) return rc;
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, std::string(stage) + " kernel launch failed");
  return WFK_OK;
}

}  // namespace

extern "C" {

// the launch of iir_rows_dac on rows whose tables (wfk_internal_iir_rows_table) and (gain, offset) pairs the caller
// holds: this file's applies, and the two-launch route of the sampled plan (wfk_iir_rows_sampled.hip)
int wfk_internal_iir_rows_dac_run(const double* tab, int nsec, int ord, int kind, int32_t batch, int64_t n,
                                  const void* in, int64_t in_stride, int16_t* out, int64_t out_stride, const double* gd,
                                  int64_t* counts, const double* zi, double* zf, const double* initial, int bits,
                                  int shift, void* hip_stream) {
  hipStream_t s = (hipStream_t)hip_stream;
  return kind == WFK_OUT_F32
             ? ird_run<float>(tab, nsec, ord, batch, n, in, in_stride, out, out_stride, gd, counts, zi, zf, initial, bits, shift, s)
             : ird_run<double>(tab, nsec, ord, batch, n, in, in_stride, out, out_stride, gd, counts, zi, zf, initial, bits, shift, s);
}

int wfk_iir_rows_dac_plan_destroy(wfk_iir_rows_dac_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_iir_rows_dac_plan_create(int32_t n_sections, const int32_t* orders, const double* b_rows, const double* a_rows,
                                 int64_t n, int32_t batch, int kind, const double* gain, const double* offset, int bits,
                                 int shift, wfk_iir_rows_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (batch < 1 || !gain || !offset) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  // the converter's refusals, then the cascades': both before any device work
  if (const int rc = wfk_internal_dac_check(batch, gain, offset, bits, shift, 1)) return rc;
  std::unique_ptr<wfk_iir_rows_dac_plan> p(new wfk_iir_rows_dac_plan());
  if (const int rc = wfk_iir_rows_plan_create(n_sections, orders, b_rows, a_rows, n, batch, kind, &p->iir)) return rc;
  p->nsec = n_sections; p->ord = orders[0];
  p->bits = bits; p->shift = shift;
  p->n = n; p->batch = batch; p->kind = kind;
  p->name = std::string("iir_rows_dac<") + (kind == WFK_OUT_F64 ? "f64" : "f32") + "," + std::to_string(n_sections) +
            "," + std::to_string(p->ord) + ">";
  std::vector<double> gd((size_t)batch * 2);
  for (int32_t r = 0; r < batch; ++r) { gd[2 * (size_t)r] = gain[r]; gd[2 * (size_t)r + 1] = offset[r]; }
  if (!p->gd.upload(gd)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "per-row IIR dac plan: device allocation / upload failed");
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the per-row IIR dac plan");
}

int wfk_iir_rows_dac_state_dim(const wfk_iir_rows_dac_plan* p) { return p ? wfk_iir_rows_state_dim(p->iir) : WFK_EINVAL; }

const char* wfk_iir_rows_dac_kernel_name(const wfk_iir_rows_dac_plan* p) { return p ? p->name.c_str() : ""; }

int wfk_iir_rows_dac_apply(wfk_iir_rows_dac_plan* p, const void* in_dev, int64_t in_stride, int16_t* out_dev,
                           int64_t out_stride, int64_t* counts_dev, const double* zi_dev, double* zf_dev,
                           const double* initial_dev, void* hip_stream) {
  return ird_apply(p, "per-row IIR dac", in_dev, false, in_stride, out_dev, out_stride, counts_dev, zi_dev,
                   zf_dev, initial_dev, hip_stream);
}

int wfk_iir_rows_dac_apply_shared_in(wfk_iir_rows_dac_plan* p, const void* in_dev, int16_t* out_dev,
                                     int64_t out_stride, int64_t* counts_dev, const double* zi_dev, double* zf_dev,
                                     const double* initial_dev, void* hip_stream) {
  return ird_apply(p, "per-row IIR dac, shared input", in_dev, true, 0, out_dev, out_stride, counts_dev, zi_dev,
                   zf_dev, initial_dev, hip_stream);
}

}  // extern "C"
