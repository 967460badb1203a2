// wfk_chain_dac.hip -- the sampler that writes DAC codes itself: the host side of wfk_chain_dac_*.
//
// Reference path: Waveform.sample() (waveforms/waveform.py:173-207) followed by the scaling to converter codes every
// AWG driver does.  Unfused that is the sampler's launch (8 B per sample written) and dac_rows (8 B read, 2 B
// written).  A microwave drive line has nothing between the two, and the DAC step has no carried state and no
// dependence between samples, so at AWG rates the short tier's own unit pipeline ends in the code instead of the
// double: wfk_sample_short_dac (wfk_short.hip, the DAC build of wfk_sample_short's body) stores 2 B per sample and the
// float64 rows never exist.  This file holds the plan: the decision (taken once, at creation), the row table, the
// checks of a launch, and the two launches of everything the fused kernel does not take.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_internal.h"

struct wfk_chain_dac_plan {
  wfk_plan* sampler = nullptr;        // the plain sampler plan: the fused kernel walks ITS units; the unfused path's first launch
  wfk_dac_rows_plan* dac = nullptr;   // the argument checks, and the unfused path's second launch
  bool fused = false;
  std::string why, name, name_counts; // why the sampler does not write the codes itself; what a launch runs
  int32_t n_channels = 0, k = 1, fam = 0;
  int bits = 0, shift = 0;
  int64_t n = 0;
  size_t rows_off = 0;
  DevBuf<char> tables;                // (gain, offset) [n_channels], the fused kernel's row table
  ~wfk_chain_dac_plan() {             // (the table goes after this body: nothing on the device reads it any more)
    if (tables) (void)hipDeviceSynchronize();
    wfk_plan_destroy(sampler);
    wfk_dac_rows_plan_destroy(dac);
  }
};

extern "C" {

int wfk_chain_dac_plan_destroy(wfk_chain_dac_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_chain_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, const double* gain_host,
                              const double* offset_host, int bits, int shift, int interleave,
                              wfk_chain_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!prog || !grid) return wfk_fail(WFK_EINVAL, "null argument");
  if (prog->n_channels < 1) return wfk_fail(WFK_EINVAL, "dac chain: a program without channels");
  std::unique_ptr<wfk_chain_dac_plan> p(new wfk_chain_dac_plan());
  p->n = grid->n;
  p->n_channels = prog->n_channels;
  p->bits = bits; p->shift = shift; p->k = interleave;
  // the DAC stage first: its argument errors come before any device work
  int rc = wfk_dac_rows_plan_create(grid->n, prog->n_channels, WFK_OUT_F64, gain_host, offset_host, bits, shift,
                                    interleave, &p->dac);
  if (!rc) rc = wfk_plan_create_grid(prog, grid, &p->sampler);
  if (rc) return rc;
  const HostPlan* hs = nullptr;
  const double* d_recs = nullptr;
  wfk_internal_plan_tables(p->sampler, &hs, &d_recs);
  if (!hs) return wfk_fail(WFK_EINVAL, "dac chain: no compiled sampler plan");
  for (uint8_t cx : hs->channel_complex)
    if (cx) return wfk_fail(WFK_EINVAL, "dac chain: complex rows");
  const std::string unfused = std::string(wfk_plan_kernel_name(p->sampler, WFK_OUT_F64)) + " + ";

  // ---- does the sampler write the codes itself?  Decided here, once: is_fused, the reason, the names and the launch read it
  SArgs sa{};
  const char* off = getenv("WFK_CHAIN_UNFUSED");
  const int f = hs->short_fam;
  if (off && off[0] == '1') p->why = "disabled by WFK_CHAIN_UNFUSED";
  else if (p->n == 0) p->why = "empty rows";
  else if (!hs->shortp || hs->tlist || hs->grid_as_tlist || !wfk_internal_plan_short_args(p->sampler, &sa)) p->why = "not a short plan";
  else if (hs->mixed) p->why = "a mixed plan (pieces without a short form)";
  else if (interleave != 1) p->why = "interleaved pairs";
  else if (f != 0 && f != 1 && f != 2 && f != 4 && f != 6) p->why = "no DAC build for op family " + std::to_string(f);
  p->fused = p->why.empty();
  p->fam = f;
  if (p->fused) {
    std::vector<double> rows((size_t)p->n_channels * 2);
    for (int32_t r = 0; r < p->n_channels; ++r) { rows[2 * r] = gain_host[r]; rows[2 * r + 1] = offset_host[r]; }
    DevTables tab;
    p->rows_off = tab.add(rows);
    if (const int rc2 = wfk_upload_tables("dac chain plan", tab, p->tables)) return rc2;
    const std::string head = "wfk_sample_short_dac<" + std::to_string(WFK_SH_R) + "," + std::to_string(f) + ",";
    p->name = head + "false>";
    p->name_counts = head + "true>";
  } else {
    p->name = unfused + wfk_dac_rows_kernel_name(p->dac, 0);
    p->name_counts = unfused + wfk_dac_rows_kernel_name(p->dac, 1);
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the dac chain plan");
}

int wfk_chain_dac_is_fused(const wfk_chain_dac_plan* p) { return p && p->fused ? 1 : 0; }

const char* wfk_chain_dac_unfused_reason(const wfk_chain_dac_plan* p) { return p ? p->why.c_str() : ""; }

const char* wfk_chain_dac_kernel_name(const wfk_chain_dac_plan* p, int with_counts) {
  if (!p) return "";
  return with_counts ? p->name_counts.c_str() : p->name.c_str();
}

int64_t wfk_chain_dac_table_bytes(const wfk_chain_dac_plan* p) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  return wfk_plan_table_bytes(p->sampler) + (int64_t)p->n_channels * 16;
}

int wfk_chain_dac_launch(wfk_chain_dac_plan* p, int16_t* out_dev, int64_t out_stride, int64_t* counts_dev,
                         void* scratch_dev, int64_t scratch_stride, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, p->n_channels, 3};
  // nothing to sample (the pointers of empty rows may be null); the report is still zeroed
  if (p->n == 0) return wfk_zero_report("dac chain", report, s);
  // a lone output row's stride is not read
  const RowSide codes{"out", out_dev, p->n_channels / p->k, out_stride, p->k * p->n, sizeof(int16_t), false};
  if (!p->fused) {
    if (!scratch_dev) return wfk_fail(WFK_EINVAL, "dac chain: an unfused launch needs scratch (" + p->why + ")");
    if (const int rc = wfk_row_rule("dac chain", {{"scratch", scratch_dev, p->n_channels, scratch_stride, p->n, sizeof(double)}},
                                    codes, kRowsAligned | kRowsDisjoint, wfk_fail, report))
      return rc;
    if (const int rc = wfk_plan_launch(p->sampler, scratch_dev, scratch_stride, WFK_OUT_F64, 0, hip_stream)) return rc;
    return wfk_dac_rows_apply(p->dac, scratch_dev, scratch_stride, out_dev, out_stride, counts_dev, hip_stream);
  }
  // (no input side: the rule takes `out` in its place; scratch is not touched)
  if (const int rc = wfk_row_rule("dac chain", {codes}, codes, kRowsAligned, wfk_fail, report)) return rc;
  if (const int rc = wfk_zero_report("dac chain", report, s)) return rc;
  SArgs sa{};
  if (!wfk_internal_plan_short_args(p->sampler, &sa)) return wfk_fail(WFK_EINVAL, "dac chain: the sampler plan has no device tables");
  sa.out = out_dev;
  sa.ch_stride = out_stride;
  DacKArgs d{};
  d.rows = DevTables::at<const double>(p->tables.get(), p->rows_off);
  d.counts = (unsigned long long*)counts_dev;
  d.lo = -(double)(1 << (p->bits - 1));
  d.hi = (double)((1 << (p->bits - 1)) - 1);
  d.shift = p->shift;
  if (hip_stream) wfk_internal_plan_note_async(p->sampler);
  std::string err;
  if (const int rc = wfk_launch_short_dac(sa, d, p->fam, hip_stream, err)) return wfk_fail(rc, "dac chain: " + err);
  return WFK_OK;
}

}  // extern "C"
