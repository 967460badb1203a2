// wfk_iir_rows_sampled.hip -- the sampler inside the per-row IIR stage.
//
// Reference chain, per flux line:  predistort(wav(t), filters=[exp_decay_filter(...), ...], initial=level)
// (waveforms/waveform.py:529-563 -> waveforms/distortion.py:100-185, :298-321): every row has its own waveform AND its
// own cascade.  Unfused that is the sampler's launch followed by iir_rows_tile in place: 8 B/sample written, read
// back and written again for 8 B of result.  iir_rows_tile has no look-back -- a workgroup owns a row and walks it in
// tiles of 4096 samples through LDS -- so the sampler fits in front of it as a FILL PHASE of the tile: the workgroup
// evaluates the tile's samples into the LDS array instead of loading them, then runs the tile body as it is
// (wfk_iir_rows_body.inc).  The unfiltered samples never exist in HBM, no workgroup waits for another,
// and rows of any length fuse.  Two fills, the two the FIR chain already has (wfk_fir_sampled.hip):
//   iir_rows_sampled  fine grids: thread `tid` evaluates the chain of 16 samples tile base + tid + 256 k with the lean
//                     sampler's arithmetic at lane stride 256 (wfk_chain_dev.h, the plan compiled by
//                     wfk_compile_geom(256, 16)) -- the very samples iir_rows_tile's loads bring a thread;
//   iir_rows_short    AWG rates: a thread owns runs of <= 16 CONTIGUOUS samples of one piece (the entries of the tile,
//                     wfk_chain_windows with hop = half = 4096 and no lead) and steps the short tier's recurrences by dt
//                     (wfk_short_dev.h); the runs land in the tile at i + (i >> 4), which IS the tile's layout.
// Tile t is evaluated right before its sweeps: there is no next-tile prefetch (nothing to load), and the row's T^lane
// table -- 64 VGPRs that iir_rows_tile holds across the row -- is read where it is applied, after the fill (64 dwords
// per lane and 4096 samples), so that the fill phases have the registers they want.
// Both kernels are built a second time with the tile leaving LDS as int16 DAC codes (iir_rows_sampled_dac,
// iir_rows_short_dac; the plan behind them is at the end of this file).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "wfk.h"
#include "wfk_host.h"
#include "wfk_internal.h"
#include "wfk_short_dev.h"
#include "wfk_chain_dev.h"
#include "wfk_curve_dev.h"
#include "wfk_iir_rows_dev.h"

#define IRW_STORE_INC "wfk_iir_rows_store.inc"   // for wfk_iir_rows_body.inc: the tile is stored as T, whole lines

#define IRS_PAR 2048            // doubles of LDS the lean fill stages a piece's parameter block in (its own area: the
                                // tile array is not free while a tile is filled)

namespace {

struct IrsLeanArgs {
  const DevChannel* channels;
  const DevPiece* pieces;
  const double* params;
  const int32_t* tile_first;   // [n_channels * ntile] first piece overlapping each tile
  double t0, step, last;
  int32_t has_last, pad;
  int64_t i0;                  // wfk_grid.i0: sample j is sample i0 + j of the caller's full grid
};

struct IrsShortArgs {
  const DevChannel* channels;
  const ShortWin* wins;        // [n_channels * 2 * npairs]: tile t of channel c at c * 2 * npairs + t
  const uint32_t* entries;     // WFK_CW_ENTRY: drec (16 bit) | offset in the tile (12 bit) | length - 1 (4 bit)
  const double* recs;          // the sampler plan's parameter table (op records)
  int64_t npairs;
  double step;
};

// the two kernels (wfk_iir_rows_sampled_kernels.inc: the text this file had here), storing their rows as T ...
#define IRS_K(name) name
#define IRS_OUT_PARAMS T* out, int64_t out_stride,
#include "wfk_iir_rows_sampled_kernels.inc"
#undef IRS_K
#undef IRS_OUT_PARAMS
#undef IRW_OUT_T
#undef IRW_STORE_INC

// ... and once more ending in int16 DAC codes: iir_rows_sampled_dac, iir_rows_short_dac
#define IRW_DAC
#define IRW_OUT_T int16_t
#define IRW_STORE_INC "wfk_iir_rows_store_dac.inc"
#define IRS_K(name) name##_dac
#define IRS_OUT_PARAMS int16_t* out, int64_t out_stride, IRW_DAC_PARAMS,
#include "wfk_iir_rows_sampled_kernels.inc"
#undef IRS_K
#undef IRS_OUT_PARAMS

// ... and a third time with the row's calibration curve in front of the tile:
// iir_rows_sampled_curve_dac, iir_rows_short_curve_dac
#define IRW_CURVE
#define IRS_K(name) name##_curve_dac
#define IRS_OUT_PARAMS int16_t* out, int64_t out_stride, IRW_DAC_PARAMS, IRW_CURVE_PARAMS,
#include "wfk_iir_rows_sampled_kernels.inc"
#undef IRW_CURVE
#undef IRW_DAC

// the static LDS of the lean fill next to the tile: what a curve in front of it cannot have (irw_curve_lds_budget)
constexpr size_t kIrsLeanLds = (IRS_PAR + 2 * (IRW_RUN + 1)) * sizeof(double);

// the eight cascade shapes iir_rows_tile has: f(NSEC, ORD as integral constants); false: none of them
template <typename F>
bool irs_shape(int nsec, int ord, F&& f) {
#define IRS_CASE(NS, OD) \
  if (nsec == NS && ord == OD) { f(std::integral_constant<int, NS>{}, std::integral_constant<int, OD>{}); return true; }
  IRS_CASE(1, 1) IRS_CASE(1, 2) IRS_CASE(1, 3) IRS_CASE(1, 4)
  IRS_CASE(2, 1) IRS_CASE(3, 1) IRS_CASE(4, 1)
  IRS_CASE(2, 2)
#undef IRS_CASE
  return false;
}

enum class IrsFill { None, Lean, Short };   // the decision of a plan, taken once at creation

}  // namespace

struct wfk_chain_iir_rows_plan {
  wfk_plan* sampler = nullptr;      // the plain sampler plan: the unfused path, the short fill's op records
  wfk_iir_rows_plan* iir = nullptr; // the rows' tables (irw_build_row) and the unfused path's second launch
  IrsFill fill = IrsFill::None;
  std::string why, name;            // why the sampler does not run inside the IIR stage; what a launch runs
  int32_t kind = 0, n_channels = 0, nsec = 0, ord = 0;
  int64_t n = 0, table_bytes = 0;
  DevBuf<char> d_tables;            // lean: the plan compiled for the tile geometry; short: channels, tile descriptors, entries
  IrsLeanArgs la{};
  IrsShortArgs sa{};
  ~wfk_chain_iir_rows_plan() {      // (the buffer goes after this body: nothing on the device reads it any more)
    if (d_tables) (void)hipDeviceSynchronize();
    wfk_plan_destroy(sampler);
    wfk_iir_rows_plan_destroy(iir);
  }
};

// the lean fill's tables; "" or why the plan cannot take it
static std::string irs_plan_lean(wfk_chain_iir_rows_plan* p, const wfk_program* prog, const wfk_grid* grid, bool& oom) {
  HostPlan H;
  std::string err;
  if (wfk_compile_geom(prog, grid, 256, IRW_RUN, H, err) != WFK_OK) return "geometry compile: " + err;
  if (!H.lean) return "plan is not fully fused (generic / direct terms, or too many ops per piece)";
  for (const DevChannel& c : H.channels)
    if (c.do_clip) return "clip (min/max) on a channel";
  for (const DevPiece& pc : H.pieces)
    if (pc.n_blk != 0 && (pc.n_blk != 1 || pc.first_len > IRS_PAR))
      return "a piece's parameter block does not fit the fill's LDS area of " + std::to_string(IRS_PAR) + " doubles";
  const int64_t ntile = (p->n + IRW_TILE - 1) / IRW_TILE;
  std::vector<int32_t> tile_first((size_t)ntile * p->n_channels);
  for (int32_t c = 0; c < p->n_channels; ++c) {
    int32_t q = H.channels[c].piece_begin;
    for (int64_t t = 0; t < ntile; ++t) {
      while (q < H.channels[c].piece_end - 1 && H.pieces[q].stop <= t * IRW_TILE) ++q;
      tile_first[(size_t)c * ntile + t] = q;
    }
  }
  DevTables t;
  const size_t o_ch = t.add(H.channels), o_pc = t.add(H.pieces), o_pa = t.add(H.params), o_tf = t.add(tile_first);
  if (!p->d_tables.alloc(t.total()) || !t.upload(p->d_tables.get())) { oom = true; return "table allocation failed"; }
  IrsLeanArgs& a = p->la;
  a.channels = t.at<const DevChannel>(p->d_tables.get(), o_ch);
  a.pieces = t.at<const DevPiece>(p->d_tables.get(), o_pc);
  a.params = t.at<const double>(p->d_tables.get(), o_pa);
  a.tile_first = t.at<const int32_t>(p->d_tables.get(), o_tf);
  a.t0 = grid->t0; a.step = grid->step; a.last = grid->last; a.has_last = grid->has_last; a.i0 = grid->i0;
  p->table_bytes = (int64_t)t.total();
  return "";
}

// the short fill's tables over the sampler plan's own op records; "" or why the plan cannot take it
static std::string irs_plan_short(wfk_chain_iir_rows_plan* p, const wfk_grid* grid, bool& oom) {
  const HostPlan* hs = nullptr;
  const double* d_recs = nullptr;
  wfk_internal_plan_tables(p->sampler, &hs, &d_recs);
  if (!hs || !d_recs || !hs->shortp) return "not a short plan";
  const int64_t ntile = (p->n + IRW_TILE - 1) / IRW_TILE, npairs = (ntile + 1) / 2;
  std::vector<ShortWin> wins;
  std::vector<uint32_t> ents;
  std::string bad;
  (void)wfk_chain_windows(*hs, p->n, IRW_TILE, 0, IRW_TILE, npairs, wins, ents, bad);
  if (!bad.empty()) return bad;
  for (const ShortWin& w : wins)
    if (w.ccnt != 0) return "a mixed plan (pieces without a short form)";
  if (ents.empty()) ents.push_back(0);
  DevTables t;
  const size_t o_ch = t.add(hs->channels), o_w = t.add(wins), o_e = t.add(ents);
  if (!p->d_tables.alloc(t.total()) || !t.upload(p->d_tables.get())) { oom = true; return "table allocation failed"; }
  IrsShortArgs& a = p->sa;
  a.channels = t.at<const DevChannel>(p->d_tables.get(), o_ch);
  a.wins = t.at<const ShortWin>(p->d_tables.get(), o_w);
  a.entries = t.at<const uint32_t>(p->d_tables.get(), o_e);
  a.recs = d_recs;
  a.npairs = npairs;
  a.step = grid->step;
  p->table_bytes = (int64_t)(t.total() + hs->params.size() * sizeof(double));
  return "";
}

extern "C" {

int wfk_chain_iir_rows_plan_destroy(wfk_chain_iir_rows_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_chain_iir_rows_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                   const int32_t* orders, const double* b_rows, const double* a_rows, int kind,
                                   wfk_chain_iir_rows_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!prog || !grid) return wfk_fail(WFK_EINVAL, "null argument");
  if (const int rc = wfk_check_kind(kind, "chain ")) return rc;
  if (prog->n_channels < 1) return wfk_fail(WFK_EINVAL, "per-row IIR chain: a program without channels");
  std::unique_ptr<wfk_chain_iir_rows_plan> p(new wfk_chain_iir_rows_plan());
  p->kind = kind;
  p->n = grid->n;
  p->n_channels = prog->n_channels;
  // the cascades first: their argument and shape errors come before any device work
  int rc = wfk_iir_rows_plan_create(n_sections, orders, b_rows, a_rows, grid->n, prog->n_channels, kind, &p->iir);
  if (!rc) rc = wfk_plan_create_grid(prog, grid, &p->sampler);
  if (rc) return rc;
  p->nsec = n_sections;
  p->ord = orders[0];
  const char* T = kind == WFK_OUT_F32 ? "f32" : "f64";   // (as iir_rows_tile prints its element type)
  const std::string shape = std::string(T) + "," + std::to_string(p->nsec) + "," + std::to_string(p->ord) + ">";
  const std::string unfused = std::string(wfk_plan_kernel_name(p->sampler, kind)) + " + " + wfk_iir_rows_kernel_name(p->iir);
  if (p->n == 0) { p->why = "empty rows"; p->name = unfused; *out = p.release(); return WFK_OK; }

  // ---- can the sampler run inside the tile?  Decided here, once: is_fused, the reason, the name and the launch read it
  const HostPlan* hs = nullptr;
  const double* d_recs = nullptr;
  wfk_internal_plan_tables(p->sampler, &hs, &d_recs);
  const char* off = getenv("WFK_CHAIN_UNFUSED");
  bool oom = false;
  if (off && off[0] == '1') p->why = "disabled by WFK_CHAIN_UNFUSED";
  else if (!irs_shape(p->nsec, p->ord, [](auto, auto) {})) p->why = "no fused kernel for this cascade shape";
  else if (!hs) p->why = "no compiled sampler plan";
  else if (hs->tlist || hs->grid_as_tlist) p->why = "the sampler plan is a time list";
  else {
    for (uint8_t cx_ : hs->channel_complex)
      if (cx_) p->why = "complex-valued channel";
  }
  if (p->why.empty()) {
    // the lean fill first, as the FIR chain decides: at AWG rates the tile geometry does not come out lean (a chain of 16
    // samples 256 apart would cross 16 pulses), and the sampler's own short plan serves the short fill
    p->why = irs_plan_lean(p.get(), prog, grid, oom);
    if (p->why.empty()) p->fill = IrsFill::Lean;
    else if (!oom && hs->shortp) {
      const std::string bad = irs_plan_short(p.get(), grid, oom);
      if (bad.empty()) { p->fill = IrsFill::Short; p->why.clear(); }
      else p->why += "; short geometry: " + bad;
    }
  }
  if (oom) return wfk_fail(WFK_ENOMEM, "per-row IIR chain: table allocation failed");
  p->name = p->fill == IrsFill::Lean ? "iir_rows_sampled<" + shape : p->fill == IrsFill::Short ? "iir_rows_short<" + shape : unfused;
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the chain plan");
}

int wfk_chain_iir_rows_is_fused(const wfk_chain_iir_rows_plan* p) { return p && p->fill != IrsFill::None ? 1 : 0; }

const char* wfk_chain_iir_rows_unfused_reason(const wfk_chain_iir_rows_plan* p) { return p ? p->why.c_str() : ""; }

const char* wfk_chain_iir_rows_kernel_name(const wfk_chain_iir_rows_plan* p) { return p ? p->name.c_str() : ""; }

int64_t wfk_chain_iir_rows_table_bytes(const wfk_chain_iir_rows_plan* p) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  return p->fill != IrsFill::None ? p->table_bytes : wfk_plan_table_bytes(p->sampler);
}

int wfk_chain_iir_rows_state_dim(const wfk_chain_iir_rows_plan* p) { return p ? wfk_iir_rows_state_dim(p->iir) : WFK_EINVAL; }

}  // extern "C"

template <typename T>
static void irs_launch(const wfk_chain_iir_rows_plan* p, void* out, int64_t os, const double* zi, double* zf,
                       const double* initial, hipStream_t s) {
  const double* tab = wfk_internal_iir_rows_table(p->iir);
  const dim3 grid((unsigned)p->n_channels), block(IRW_THREADS);
  (void)irs_shape(p->nsec, p->ord, [&](auto ns, auto od) {
    constexpr int NS = decltype(ns)::value, OD = decltype(od)::value;
    if (p->fill == IrsFill::Lean)
      hipLaunchKernelGGL((iir_rows_sampled<T, NS, OD>), grid, block, 0, s, p->la, (T*)out, os, tab, zi, zf, initial, p->n);
    else
      hipLaunchKernelGGL((iir_rows_short<T, NS, OD>), grid, block, 0, s, p->sa, (T*)out, os, tab, zi, zf, initial, p->n);
  });
}

extern "C" int wfk_chain_iir_rows_launch(wfk_chain_iir_rows_plan* p, void* out_dev, int64_t out_stride,
                                         const double* zi_dev, double* zf_dev, const double* initial_dev,
                                         void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  if (p->n == 0) return WFK_OK;
  if (const int rc = wfk_check_rows("per-row IIR chain", p->n, wfk_elem_size(p->kind), out_dev, p->n_channels,
                                    out_stride, out_dev, p->n_channels, out_stride))
    return rc;
  if (p->fill == IrsFill::None) {
    const int rc = wfk_plan_launch(p->sampler, out_dev, out_stride, p->kind, 0, hip_stream);
    if (rc) return rc;
    return wfk_iir_rows_apply(p->iir, out_dev, out_stride, out_dev, out_stride, zi_dev, zf_dev, initial_dev, hip_stream);
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (p->kind == WFK_OUT_F64) irs_launch<double>(p, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s);
  else irs_launch<float>(p, out_dev, out_stride, zi_dev, zf_dev, initial_dev, s);
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "fused sampler -> per-row IIR kernel launch failed");
  return WFK_OK;
}

// ---- the same chain ending in int16 DAC codes: SampledIirRows -> DacStage in one kernel -----------------
// The plan is a float64 chain plan -- its fill decision, its tables, its sampler, its rows' IIR tables -- and the rows'
// (gain, offset) pairs.  Where the chain plan fuses, the same fill runs in front of the codes store
// (iir_rows_sampled_dac / iir_rows_short_dac); where it does not, the sampler writes float64 rows into a scratch the
// caller lends and iir_rows_dac (wfk_iir_rows_dac.hip) reads them: two launches instead of three.
struct wfk_chain_iir_rows_dac_plan {
  wfk_chain_iir_rows_plan* chain = nullptr;
  DevBuf<double> gd;                // [n_channels][2]: gain, offset
  int bits = 0, shift = 0;
  std::string why, name;
  ~wfk_chain_iir_rows_dac_plan() {  // (the pairs go after this body: nothing on the device reads them any more)
    if (gd) (void)hipDeviceSynchronize();
    wfk_chain_iir_rows_plan_destroy(chain);
  }
};

extern "C" {

int wfk_chain_iir_rows_dac_plan_destroy(wfk_chain_iir_rows_dac_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_chain_iir_rows_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                       const int32_t* orders, const double* b_rows, const double* a_rows,
                                       const double* gain, const double* offset, int bits, int shift,
                                       wfk_chain_iir_rows_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!prog || !grid) return wfk_fail(WFK_EINVAL, "null argument");
  if (prog->n_channels < 1) return wfk_fail(WFK_EINVAL, "per-row IIR chain: a program without channels");
  if (!gain || !offset) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  // the converter's refusals, then the chain's: both before any device work
  if (const int rc = wfk_internal_dac_check(prog->n_channels, gain, offset, bits, shift, 1)) return rc;
  std::unique_ptr<wfk_chain_iir_rows_dac_plan> p(new wfk_chain_iir_rows_dac_plan());
  if (const int rc = wfk_chain_iir_rows_plan_create(prog, grid, n_sections, orders, b_rows, a_rows, WFK_OUT_F64, &p->chain))
    return rc;
  const wfk_chain_iir_rows_plan* c = p->chain;
  p->bits = bits; p->shift = shift;
  std::vector<double> gd((size_t)c->n_channels * 2);
  for (int32_t r = 0; r < c->n_channels; ++r) { gd[2 * (size_t)r] = gain[r]; gd[2 * (size_t)r + 1] = offset[r]; }
  if (!p->gd.upload(gd)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "per-row IIR dac chain: device allocation / upload failed");
  }
  const std::string shape = "f64," + std::to_string(c->nsec) + "," + std::to_string(c->ord) + ">";
  if (c->fill == IrsFill::Lean) p->name = "iir_rows_sampled_dac<" + shape;
  else if (c->fill == IrsFill::Short) p->name = "iir_rows_short_dac<" + shape;
  else {
    p->why = c->why + ": the sampler writes float64 rows into the plan's scratch, iir_rows_dac reads them";
    p->name = std::string(wfk_plan_kernel_name(c->sampler, WFK_OUT_F64)) + " + iir_rows_dac<" + shape;
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the chain plan");
}

int wfk_chain_iir_rows_dac_is_fused(const wfk_chain_iir_rows_dac_plan* p) { return p ? wfk_chain_iir_rows_is_fused(p->chain) : 0; }

const char* wfk_chain_iir_rows_dac_unfused_reason(const wfk_chain_iir_rows_dac_plan* p) { return p ? p->why.c_str() : ""; }

const char* wfk_chain_iir_rows_dac_kernel_name(const wfk_chain_iir_rows_dac_plan* p) { return p ? p->name.c_str() : ""; }

int64_t wfk_chain_iir_rows_dac_table_bytes(const wfk_chain_iir_rows_dac_plan* p) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  return wfk_chain_iir_rows_table_bytes(p->chain) + (int64_t)p->chain->n_channels * 16;
}

int wfk_chain_iir_rows_dac_state_dim(const wfk_chain_iir_rows_dac_plan* p) {
  return p ? wfk_chain_iir_rows_state_dim(p->chain) : WFK_EINVAL;
}

int wfk_chain_iir_rows_dac_launch(wfk_chain_iir_rows_dac_plan* p, int16_t* out_dev, int64_t out_stride,
                                  int64_t* counts_dev, void* scratch_dev, int64_t scratch_stride, const double* zi_dev,
                                  double* zf_dev, const double* initial_dev, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  const wfk_chain_iir_rows_plan* c = p->chain;
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, c->n_channels, 3};
  // nothing to sample (the pointers of empty rows may be null); the report is still zeroed
  if (c->n == 0) return wfk_zero_report("per-row IIR dac chain", report, s);
  // a lone code row's stride is not read
  const RowSide codes{"out", out_dev, c->n_channels, out_stride, c->n, sizeof(int16_t), false};
  const double* tab = wfk_internal_iir_rows_table(c->iir);
  if (c->fill == IrsFill::None) {
    if (!scratch_dev) return wfk_fail(WFK_EINVAL, "per-row IIR dac chain: an unfused launch needs scratch (" + c->why + ")");
    if (const int rc = wfk_row_rule("per-row IIR dac chain",
                                    {{"scratch", scratch_dev, c->n_channels, scratch_stride, c->n, sizeof(double)}}, codes,
                                    kRowsAligned | kRowsDisjoint, wfk_fail, report))
      return rc;
    if (const int rc = wfk_plan_launch(c->sampler, scratch_dev, scratch_stride, WFK_OUT_F64, 0, hip_stream)) return rc;
    if (const int rc = wfk_internal_iir_rows_dac_run(tab, c->nsec, c->ord, WFK_OUT_F64, c->n_channels, c->n, scratch_dev,
                                                     scratch_stride, out_dev, out_stride, p->gd.get(), counts_dev, zi_dev,
                                                     zf_dev, initial_dev, p->bits, p->shift, hip_stream))
      return rc;
  } else {
    // (no input side: the rule takes `out` in its place; scratch is not touched)
    if (const int rc = wfk_row_rule("per-row IIR dac chain", {codes}, codes, kRowsAligned, wfk_fail, report)) return rc;
    const double lo = -(double)(1 << (p->bits - 1)), hi = (double)((1 << (p->bits - 1)) - 1);
    const dim3 grid((unsigned)c->n_channels), block(IRW_THREADS);
    unsigned long long* counts = (unsigned long long*)counts_dev;
    (void)irs_shape(c->nsec, c->ord, [&](auto ns, auto od) {
      constexpr int NS = decltype(ns)::value, OD = decltype(od)::value;
      if (c->fill == IrsFill::Lean)
        hipLaunchKernelGGL((iir_rows_sampled_dac<double, NS, OD>), grid, block, 0, s, c->la, out_dev, out_stride,
                           p->gd.get(), counts, lo, hi, p->shift, tab, zi_dev, zf_dev, initial_dev, c->n);
      else
        hipLaunchKernelGGL((iir_rows_short_dac<double, NS, OD>), grid, block, 0, s, c->sa, out_dev, out_stride,
                           p->gd.get(), counts, lo, hi, p->shift, tab, zi_dev, zf_dev, initial_dev, c->n);
    });
  }
  if (hipGetLastError() != hipSuccess) return wfk_fail(WFK_EHIP, "sampler -> per-row IIR -> codes kernel launch failed");
  return WFK_OK;
}

}  // extern "C"

// ---- the same chain with the row's calibration curve between the sampler and the IIR:
// BatchSampler -> CurveStage -> IirDacStage in one kernel.  The plan is a float64 chain plan -- its fill decision, its
// tables, its sampler, its rows' IIR tables -- the rows' (gain, offset) pairs and the curves' tables.  Where the chain
// plan fuses and the curves' tables fit next to the fill's LDS, the fill's samples go through the curve on their way
// into the sweeps (iir_rows_sampled_curve_dac / iir_rows_short_curve_dac); otherwise the sampler writes float64 rows
// into a scratch the caller lends and iir_rows_curve_dac (wfk_iir_rows_curve_dac.hip) reads them: two launches.
struct wfk_chain_curve_iir_dac_plan {
  wfk_chain_iir_rows_plan* chain = nullptr;
  bool fused = false;
  DevBuf<double> gd;                // [n_channels][2]: gain, offset
  DevBuf<char> tables;              // CurveRow [n_channels], the knots, the buckets
  size_t rows_off = 0, knots_off = 0, buckets_off = 0, lds_bytes = 0, table_bytes = 0;
  int lds_knots = 0, bits = 0, shift = 0;
  std::string why, name;
  ~wfk_chain_curve_iir_dac_plan() {  // (the buffers go after this body: nothing on the device reads them any more)
    if (gd || tables) (void)hipDeviceSynchronize();
    wfk_chain_iir_rows_plan_destroy(chain);
  }
};

extern "C" {

int wfk_chain_curve_iir_dac_plan_destroy(wfk_chain_curve_iir_dac_plan* p) {
  delete p;
  return WFK_OK;
}

int wfk_chain_curve_iir_dac_plan_create(const wfk_program* prog, const wfk_grid* grid, int32_t n_sections,
                                        const int32_t* orders, const double* b_rows, const double* a_rows,
                                        const int64_t* knot_ptr, const double* xp, const double* fp, const double* left,
                                        const double* right, const double* gain, const double* offset, int bits,
                                        int shift, wfk_chain_curve_iir_dac_plan** out) try {
  if (!out) return wfk_fail(WFK_EINVAL, "null out");
  *out = nullptr;
  if (!prog || !grid) return wfk_fail(WFK_EINVAL, "null argument");
  if (prog->n_channels < 1) return wfk_fail(WFK_EINVAL, "per-row IIR chain: a program without channels");
  // the curve's refusals, then the converter's, then the chain's: all before any device work
  if (const int rc = curve_check(grid->n, prog->n_channels, WFK_OUT_F64, knot_ptr, xp, fp)) return rc;
  if (!gain || !offset) return wfk_fail(WFK_EINVAL, "bad dac rows plan arguments");
  if (const int rc = wfk_internal_dac_check(prog->n_channels, gain, offset, bits, shift, 1)) return rc;
  std::unique_ptr<wfk_chain_curve_iir_dac_plan> p(new wfk_chain_curve_iir_dac_plan());
  if (const int rc = wfk_chain_iir_rows_plan_create(prog, grid, n_sections, orders, b_rows, a_rows, WFK_OUT_F64, &p->chain))
    return rc;
  const wfk_chain_iir_rows_plan* c = p->chain;
  p->bits = bits; p->shift = shift;
  // fused exactly where the chain plan is -- but for curves whose knots alone do not fit next to the lean fill's
  // parameter area: those plans take the composed route, whose kernel has the room
  int max_k = 0;
  for (int32_t r = 0; r < c->n_channels; ++r) max_k = std::max(max_k, (int)(knot_ptr[r + 1] - knot_ptr[r]));
  const size_t lean_budget = irw_curve_lds_budget(sizeof(double), kIrsLeanLds);
  const bool tight = c->fill == IrsFill::Lean && (size_t)24 * max_k > lean_budget;
  p->fused = c->fill != IrsFill::None && !tight;
  const size_t budget = p->fused && c->fill == IrsFill::Lean ? lean_budget : irw_curve_lds_budget(sizeof(double));
  const CurveTables ct = curve_build(c->n_channels, knot_ptr, xp, fp, left, right, true, budget);
  p->lds_knots = ct.max_k;
  p->lds_bytes = ct.lds_bytes();
  DevTables tab;
  p->rows_off = tab.add(ct.rows);
  p->knots_off = tab.add(ct.knots);
  p->buckets_off = tab.add(ct.buckets);
  p->table_bytes = tab.total();
  if (const int rc = wfk_upload_tables("per-row curve IIR dac chain", tab, p->tables)) return rc;
  std::vector<double> gd((size_t)c->n_channels * 2);
  for (int32_t r = 0; r < c->n_channels; ++r) { gd[2 * (size_t)r] = gain[r]; gd[2 * (size_t)r + 1] = offset[r]; }
  if (!p->gd.upload(gd)) {
    (void)hipGetLastError();
    return wfk_fail(WFK_ENOMEM, "per-row curve IIR dac chain: device allocation / upload failed");
  }
  const std::string shape = "f64," + std::to_string(c->nsec) + "," + std::to_string(c->ord) + ">";
  if (p->fused) p->name = (c->fill == IrsFill::Lean ? "iir_rows_sampled_curve_dac<" : "iir_rows_short_curve_dac<") + shape;
  else {
    p->why = (tight ? "a curve of " + std::to_string(max_k) + " knots does not fit next to the lean fill's LDS (" +
                          std::to_string(lean_budget / 24) + " at most)"
                    : c->why) +
             ": the sampler writes float64 rows into the plan's scratch, iir_rows_curve_dac reads them";
    p->name = std::string(wfk_plan_kernel_name(c->sampler, WFK_OUT_F64)) + " + iir_rows_curve_dac<" + shape;
  }
  *out = p.release();
  return WFK_OK;
} catch (const std::bad_alloc&) {
  return wfk_fail(WFK_ENOMEM, "out of host memory while building the chain plan");
}

int wfk_chain_curve_iir_dac_is_fused(const wfk_chain_curve_iir_dac_plan* p) { return p && p->fused ? 1 : 0; }

const char* wfk_chain_curve_iir_dac_unfused_reason(const wfk_chain_curve_iir_dac_plan* p) { return p ? p->why.c_str() : ""; }

const char* wfk_chain_curve_iir_dac_kernel_name(const wfk_chain_curve_iir_dac_plan* p) { return p ? p->name.c_str() : ""; }

int64_t wfk_chain_curve_iir_dac_table_bytes(const wfk_chain_curve_iir_dac_plan* p) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  const int64_t chain = p->fused ? wfk_chain_iir_rows_table_bytes(p->chain) : wfk_plan_table_bytes(p->chain->sampler);
  return chain + (int64_t)p->chain->n_channels * 16 + (int64_t)p->table_bytes;
}

int wfk_chain_curve_iir_dac_state_dim(const wfk_chain_curve_iir_dac_plan* p) {
  return p ? wfk_chain_iir_rows_state_dim(p->chain) : WFK_EINVAL;
}

int wfk_chain_curve_iir_dac_launch(wfk_chain_curve_iir_dac_plan* p, int16_t* out_dev, int64_t out_stride,
                                   int64_t* counts_dev, int64_t* beyond_dev, void* scratch_dev, int64_t scratch_stride,
                                   const double* zi_dev, double* zf_dev, const double* initial_dev, void* hip_stream) {
  if (!p) return wfk_fail(WFK_EINVAL, "null plan");
  const wfk_chain_iir_rows_plan* c = p->chain;
  const char* stage = "per-row curve IIR dac chain";
  hipStream_t s = (hipStream_t)hip_stream;
  const RowReport report{counts_dev, c->n_channels, 3};
  // nothing to sample (the pointers of empty rows may be null); the reports are still zeroed
  if (c->n == 0) {
    if (const int rc = curve_beyond_rule(stage, beyond_dev, c->n_channels, counts_dev, {})) return rc;
    if (const int rc = wfk_zero_report(stage, report, s)) return rc;
    return wfk_zero_report(stage, RowReport{beyond_dev, c->n_channels, 3}, s);
  }
  // a lone code row's stride is not read
  const RowSide codes{"out", out_dev, c->n_channels, out_stride, c->n, sizeof(int16_t), false};
  const double* tab = wfk_internal_iir_rows_table(c->iir);
  const CurveRow* crows = DevTables::at<const CurveRow>(p->tables.get(), p->rows_off);
  const double* cknots = DevTables::at<const double>(p->tables.get(), p->knots_off);
  const uint32_t* cbuckets = DevTables::at<const uint32_t>(p->tables.get(), p->buckets_off);
  if (!p->fused) {
    if (!scratch_dev) return wfk_fail(WFK_EINVAL, std::string(stage) + ": an unfused launch needs scratch (" + p->why + ")");
    const RowSide scratch{"scratch", scratch_dev, c->n_channels, scratch_stride, c->n, sizeof(double)};
    if (const int rc = wfk_row_rule(stage, {scratch}, codes, kRowsAligned | kRowsDisjoint, wfk_fail, report)) return rc;
    if (const int rc = curve_beyond_rule(stage, beyond_dev, c->n_channels, counts_dev, {scratch, codes})) return rc;
    if (const int rc = wfk_plan_launch(c->sampler, scratch_dev, scratch_stride, WFK_OUT_F64, 0, hip_stream)) return rc;
    if (const int rc = wfk_internal_curve_iir_dac_run(tab, c->nsec, c->ord, WFK_OUT_F64, c->n_channels, c->n, scratch_dev,
                                                      scratch_stride, out_dev, out_stride, p->gd.get(), counts_dev, crows,
                                                      cknots, cbuckets, beyond_dev, p->lds_knots, p->lds_bytes, zi_dev,
                                                      zf_dev, initial_dev, p->bits, p->shift, hip_stream))
      return rc;
  } else {
    // (no input side: the rule takes `out` in its place; scratch is not touched)
    if (const int rc = wfk_row_rule(stage, {codes}, codes, kRowsAligned, wfk_fail, report)) return rc;
    if (const int rc = curve_beyond_rule(stage, beyond_dev, c->n_channels, counts_dev, {codes})) return rc;
    const double lo = -(double)(1 << (p->bits - 1)), hi = (double)((1 << (p->bits - 1)) - 1);
    const dim3 grid((unsigned)c->n_channels), block(IRW_THREADS);
    unsigned long long* counts = (unsigned long long*)counts_dev;
    unsigned long long* beyond = (unsigned long long*)beyond_dev;
    (void)irs_shape(c->nsec, c->ord, [&](auto ns, auto od) {
      constexpr int NS = decltype(ns)::value, OD = decltype(od)::value;
      if (c->fill == IrsFill::Lean)
        hipLaunchKernelGGL((iir_rows_sampled_curve_dac<double, NS, OD>), grid, block, p->lds_bytes, s, c->la, out_dev,
                           out_stride, p->gd.get(), counts, lo, hi, p->shift, crows, cknots, cbuckets, beyond,
                           p->lds_knots, tab, zi_dev, zf_dev, initial_dev, c->n);
      else
        hipLaunchKernelGGL((iir_rows_short_curve_dac<double, NS, OD>), grid, block, p->lds_bytes, s, c->sa, out_dev,
                           out_stride, p->gd.get(), counts, lo, hi, p->shift, crows, cknots, cbuckets, beyond,
                           p->lds_knots, tab, zi_dev, zf_dev, initial_dev, c->n);
    });
  }
  if (hipGetLastError() != hipSuccess)
    return wfk_fail(WFK_EHIP, "sampler -> curve -> per-row IIR -> codes kernel launch failed");
  return WFK_OK;
}

}  // extern "C"
