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
#include "wfk_iir_rows_dev.h"

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

// ---- the lean fill: stride-256 chains (the sampling phase of fir_sampled, CL = 16, no carried op state) -----------
template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) iir_rows_sampled(const IrsLeanArgs a, T* out, int64_t out_stride,
                                                                const double* __restrict__ tab,
                                                                const double* __restrict__ zi, double* __restrict__ zf,
                                                                const double* __restrict__ initial, int64_t n) {
  constexpr int CL = IRW_RUN;
#include "wfk_iir_rows_head.inc"
  __shared__ __attribute__((aligned(16))) double s_par[IRS_PAR + 2 * (CL + 1)];
  double2* const unit_tab = reinterpret_cast<double2*>(s_par + IRS_PAR);
  const DevChannel C = a.channels[row];
  if (tid <= CL) unit_tab[tid] = make_double2(1.0, 0.0);       // phasor table of ops without a carrier
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t s1 = t * IRW_TILE, range_end = s1 + IRW_TILE; // per-thread sample index: s1 + tid + 256 k
    T acc[CL];
    CH_EACH(CL, k) acc[k] = (T)0; CH_END
    double x;
    {
      // t[j] = fl(fl(j*step) + t0) (NumPy's linspace / arange element formula), as fir_sampled's chain_time.  As there,
      // the time is taken for the chain's FIRST sample only: an endpoint grid's overridden last sample gets `last` where
      // it starts a chain (k = 0); further down a chain its time is the stride-256 continuation, one ulp of t away
#pragma clang fp contract(off)
      const int64_t j = s1 + tid;
      const double m = (double)(j + a.i0) * a.step;
      x = m + a.t0;
      if (a.has_last && j == n - 1) x = a.last;
    }
    if (C.tshift != 0.0) x = x - C.tshift;
    int q = cuni(a.tile_first[row * ntile + t]);
    for (; q < C.piece_end; q = cuni(q + 1)) {
      const DevPiece P = a.pieces[q];
      if (P.start >= range_end) break;
      if (P.n_blk == 0 || P.stop <= s1) continue;               // zero piece / entirely before the tile
      __syncthreads();                                           // every wave is done with the previous block
      for (int i = tid; i < P.first_len; i += IRW_THREADS) s_par[i] = a.params[P.par_off + i];
      __syncthreads();
      const int nops = cuni((int)s_par[1]);
      const bool full = P.start <= s1 && P.stop >= range_end;   // wave-uniform: the whole tile is inside
      int klo = 0, khi = CL;
      if (!full) {
        // samples k of this thread inside the piece: P.start <= s1 + tid + 256 k < P.stop (scalar parts clamped to
        // what matters for k in [0, CL): the per-thread part is 32-bit)
        const int64_t lim = 256 * (int64_t)(CL + 2);
        const int64_t los = P.start - s1, his = P.stop - s1;
        const int lo = (int)(los < -lim ? -lim : (los > lim ? lim : los)) - tid;
        const int hi = (int)(his < -lim ? -lim : (his > lim ? lim : his)) - tid;
        klo = lo <= 0 ? 0 : (lo + 255) >> 8;
        khi = hi <= 0 ? 0 : (hi + 255) >> 8;
        klo = klo > CL ? CL : klo;
        khi = khi > CL ? CL : khi;
      }
      for (int op = 0; op < nops; ++op) {
        const double* rec = s_par + WFK_BLK_HDR + op * WFK_FCE_REC;
        const int fl = cuni(WFK_FCE_WORD(rec));
        const int env = (fl >> 4) & 3, carrier = (fl >> 2) & 1;
        ChSeeds nx;
        const ChSeeds sd = chain_make_seeds(rec, x, fl);         // exact
        if (env == 3) {
          chain_envmul<T, CL, -1>(rec, sd, acc, klo, khi, nx);
        } else {
          const double2* ptab = carrier ? reinterpret_cast<const double2*>(s_par + WFK_FCE_TABOFF(fl)) : unit_tab;
          const double qq = env ? rec[WFK_FCE_Q] : 1.0;
          const double u0 = x - rec[WFK_FCE_SLIN];
          if (full && (fl & 3) <= 1) chain_loop<T, CL, -1, false, true>(ptab, rec, sd, u0, qq, acc, 0, CL, nx);
          else if (full) chain_loop<T, CL, -1, false, false>(ptab, rec, sd, u0, qq, acc, 0, CL, nx);
          else chain_loop<T, CL, -1, true, false>(ptab, rec, sd, u0, qq, acc, klo, khi, nx);
        }
      }
    }
    // channel offset inside [0, n), zeros behind the row; into the tile by the scatter of iir_rows_tile's loads
    // (the previous tile's body ended with a barrier: the array is free)
    const T off = (T)C.offset;
    const int64_t left = n - s1;
    CH_EACH(CL, k)
      const int j = k * IRW_THREADS + tid;
      tile[irw_at(j)] = j < left ? acc[k] + off : (T)0;
    CH_END
    __syncthreads();
    {
      const int64_t base = s1;
      double L[MM];                                              // T^lane, read here: after the fill
#pragma unroll
      for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
#include "wfk_iir_rows_body.inc"
    }
  }
}

// ---- the short fill: runs of one piece (the entry evaluation of fir_short) -----------------------------------------
template <typename T, int NSEC, int ORD>
__global__ void __launch_bounds__(IRW_THREADS) iir_rows_short(const IrsShortArgs a, T* out, int64_t out_stride,
                                                              const double* __restrict__ tab,
                                                              const double* __restrict__ zi, double* __restrict__ zf,
                                                              const double* __restrict__ initial, int64_t n) {
  constexpr int R = WFK_SH_R;
  static_assert(R == IRW_RUN, "an entry is at most one run of the tile");
#include "wfk_iir_rows_head.inc"
  const DevChannel C = a.channels[row];
  const double coff = C.offset;
  const ShortWin* const wp = a.wins + row * 2 * a.npairs;
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t h0 = t * IRW_TILE, left = n - h0;
    const int64_t rec0 = cuni64(wp[t].rec0), e0 = cuni64(wp[t].e0);   // (block-uniform: SGPRs)
    const int cnt = cuni(wp[t].cnt);
    // zeros behind the row, the channel offset inside (skipped zero pieces, gaps between entries); the previous tile's
    // body ended with a barrier: the array is free.  Always the padded layout: it is the tile's
    CH_EACH(IRW_RUN, k)
      const int j = k * IRW_THREADS + tid;
      tile[irw_at(j)] = j < left ? (T)coff : (T)0;
    CH_END
    __syncthreads();
    for (int eb = 0; eb < cnt; eb += IRW_THREADS) {             // block-uniform trip count
      const int idx = eb + tid;
      bool live = idx < cnt;
      const uint32_t word = live ? a.entries[e0 + idx] : 0u;
      const int len = live ? (int)(word >> 28) + 1 : 0;
      const int o = (int)((word >> 16) & 0xfff);
      const double* op = a.recs + 2 * (rec0 + (int64_t)(word & 0xffff));
      shdev::OpRec rec = shdev::load_op(op);
      const double kf = (double)((int)(uint32_t)(h0 + o) - shdev::op_ref(rec));   // samples from the record's reference sample
      double acc[R], acci[1];
      CH_EACH(R, k) acc[k] = 0.0; CH_END
      acci[0] = 0.0;
      auto eval = [&](const shdev::OpRec& rc, const double* opp, bool lv) -> bool {   // -> another op follows
        const int w = shdev::op_word(rc);
        const bool closing = ((w >> 4) & 3) == 3;               // erf edge multiplier
        const bool mine = lv && !closing && !(w & 8);           // (real channels only: no op of an imaginary part)
        const bool cubic = __any(mine && (w & 3) > 1);
        if (mine) {
          if (cubic) shdev::short_op<R, true, false>(rc, opp, w, kf, a.step, acc, acci);
          else shdev::short_op<R, false, false>(rc, opp, w, kf, a.step, acc, acci);
        }
        if (__any(lv && closing)) {
          if (lv && closing) shdev::short_erfmul<R, false>(rc, kf, acc, acci);
        }
        return lv && !(w & WFK_SH_LAST);
      };
      live = eval(rec, op, live);
      while (__any(live)) {
        op += (shdev::op_word(rec) & 3) > 1 ? WFK_SH_OP3 : WFK_SH_OP1;
        if (live) rec = shdev::load_op(op);
        live = eval(rec, op, live);
      }
      if (C.do_clip) {
        CH_EACH(R, k) acc[k] = shdev::clip_np(acc[k], C.clip_lo, C.clip_hi); CH_END
      }
      // element o + k of the tile sits at (o + k) + ((o + k) >> 4) = irw_at(o) + k + [k >= 16 - (o & 15)]
      T* const b0 = tile + o + (o >> 4);
      const int tk = 16 - (o & 15);
      CH_EACH(R, k)
        if (k < len) *((k >= tk ? b0 + 1 : b0) + k) = (T)(acc[k] + coff);
      CH_END
    }
    __syncthreads();
    {
      const int64_t base = h0;
      double L[MM];                                              // T^lane, read here: after the fill
#pragma unroll
      for (int e = 0; e < MM; ++e) L[e] = pw[(IRW_NPW + lane) * MM + e];
#include "wfk_iir_rows_body.inc"
    }
  }
}

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
