// wfk_compile.cpp -- host compiler: flattened expression forest (include/wfk.h)
// + time axis -> device tables (wfk_internal.h).  Pure host C++, no HIP calls.
//
// What it decides, all of it O(#pieces), never per sample:
//  * integer piece membership: np.searchsorted(x - tshift, bounds, 'left') per
//    member (reference: waveforms/_waveform.pyx:156), evaluated on the EXACT grid
//    formula t[i] = fl(fl(i*step)+t0) so indices are bit-identical to NumPy's
//  * WaveVStack members (waveforms/waveform.py:690-692) merged into disjoint
//    pieces per channel, so each output sample is written exactly once
//  * per factor: uniform-grid fast path (phasor table / recurrences) or direct
//    device-libm evaluation
//  * parameter blocks sized for the LDS staging buffer
//
// Compiled with -ffp-contract=off: the grid formula must round twice.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "wfk.h"
#include "wfk_internal.h"

#include "wfk_compile_types.h"

namespace {

int argc_of(int type) {
  switch (type) {
    case WFK_LINEAR: return 0;
    case WFK_GAUSSIAN: case WFK_ERF: case WFK_COS: case WFK_SINC: case WFK_EXP:
    case WFK_COSH: case WFK_SINH: return 1;
    case WFK_MOLLIFIER: case WFK_D_GAUSSIAN: return 2;
    case WFK_EXPONENTIALCHIRP: case WFK_HYPERBOLICCHIRP: return 3;
    case WFK_LINEARCHIRP: return 4;
    case WFK_DRAG: return 6;
    case WFK_INTERP: return -1;
    case WFK_DRAG_SIN: case WFK_DRAG_SINX: return -3;
    case WFK_SAMPLED: return -4;
    default: return -2;
  }
}

}  // namespace

// the sample times of a grid, as NumPy forms them (this file is built -ffp-contract=off)
void wfk_internal_grid_times(const wfk_grid* g, double* out) {
  const TimeAxis ax{g, nullptr, g->n};
  for (int64_t i = 0; i < g->n; ++i) out[i] = ax.at(i);
}

// WFK_TIMING=1: where a compile spends its time, phase by phase, on stderr (tools/plan_build_bench.py)
struct PhaseTimer {
  bool on;
  std::chrono::steady_clock::time_point t0;
  PhaseTimer() : on(std::getenv("WFK_TIMING") != nullptr), t0(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "wfk_compile %-14s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
  ~PhaseTimer() { mark("rest"); }
};

// ---- validate structure ----------------------------------------------------
static int validate_program(const wfk_program* P, std::string& err) {
  auto offsets_ok = [](const auto* off, int64_t count, int64_t total) {
    if (off[0] != 0 || off[count] != total) return false;
    for (int64_t i = 0; i < count; ++i)
      if (off[i] > off[i + 1]) return false;
    return true;
  };
  if (P->n_pieces < 0 || P->n_terms < 0 || P->n_factors < 0 || P->n_pool < 0 ||
      !offsets_ok(P->ch_member_off, P->n_channels, P->n_members) ||
      !offsets_ok(P->mb_piece_off, P->n_members, P->n_pieces) ||
      !offsets_ok(P->pc_term_off, P->n_pieces, P->n_terms) ||
      !offsets_ok(P->tm_factor_off, P->n_terms, P->n_factors) ||
      !offsets_ok(P->fc_arg_off, P->n_factors, P->n_pool)) {
    err = "offset arrays must start at 0, be non-decreasing and end at the element counts";
    return WFK_EINVAL;
  }
  for (int32_t c = 0; c < P->n_channels; ++c)
    if (P->ch_member_off[c] > P->ch_member_off[c + 1]) { err = "ch_member_off not monotone"; return WFK_EINVAL; }
    else if (std::isnan(P->ch_clip_lo[c]) || std::isnan(P->ch_clip_hi[c])) { err = "NaN clip"; return WFK_EINVAL; }
  for (int32_t m = 0; m < P->n_members; ++m) {
    int32_t a = P->mb_piece_off[m], b = P->mb_piece_off[m + 1];
    if (b <= a) { err = "member without pieces"; return WFK_EINVAL; }
    if (!(P->pc_bound[b - 1] == INFINITY)) { err = "last bound of a member must be +inf"; return WFK_EINVAL; }
    for (int32_t p = a + 1; p < b; ++p)
      if (!(P->pc_bound[p - 1] <= P->pc_bound[p])) { err = "bounds not ascending"; return WFK_EINVAL; }
  }
  for (int32_t f = 0; f < P->n_factors; ++f) {
    int want = argc_of(P->fc_type[f]);
    int64_t have = P->fc_arg_off[f + 1] - P->fc_arg_off[f];
    if (want == -2) {
      err = "primitive id " + std::to_string(P->fc_type[f]) + " has no device implementation";
      return WFK_EUNSUP;
    }
    if (want == -3) {   // compiled multi-notch DRAG: header + tables, lengths must agree
      const double* a = P->pool + P->fc_arg_off[f];
      bool ok = have >= 9;
      if (ok) {
        const double m = a[7], dq = a[8];
        ok = m >= 0 && m <= 64 && m == std::floor(m) && dq >= -1 && dq <= 256 && dq == std::floor(dq) &&
             have == 9 + 2 * ((int64_t)m + 1) + 2 + (dq >= 0 ? 4 * ((int64_t)dq + 1) : 0) &&
             (P->fc_type[f] == WFK_DRAG_SINX) == (dq >= 0);
      }
      if (!ok) { err = "malformed compiled DRAG_SIN/DRAG_SINX argument block"; return WFK_EINVAL; }
      continue;
    }
    if (want == -4) {   // caller-evaluated factor: (i0, values...)
      const double i0 = have >= 1 ? P->pool[P->fc_arg_off[f]] : NAN;
      if (!(have >= 1) || !(i0 >= 0) || i0 != std::floor(i0) || i0 > 9.0e15) {
        err = "malformed SAMPLED factor: needs (i0 >= 0, values...)"; return WFK_EINVAL;
      }
      continue;
    }
    if ((want >= 0 && have != want) || (want == -1 && have < 3)) {
      err = "wrong argument count for primitive id " + std::to_string(P->fc_type[f]);
      return WFK_EINVAL;
    }
    const double* a = P->pool + P->fc_arg_off[f];
    if ((P->fc_type[f] == WFK_MOLLIFIER && (a[1] < 0 || a[1] > 12 || a[1] != std::floor(a[1]))) ||
        (P->fc_type[f] == WFK_D_GAUSSIAN && (a[1] < 0 || a[1] > 64 || a[1] != std::floor(a[1])))) {
      err = "derivative order out of range"; return WFK_EINVAL;
    }
  }
  return WFK_OK;
}

// ---- searchsorted per member, then the geometry: short tier? -------------------------------------
// Writes H.member_idx and H.mean_piece_len; returns whether the plan is compiled for the short tier.
static bool search_members(const wfk_program* P, const TimeAxis& ax, const CompileEnv& env, const Attempt& at, HostPlan& H) {
  H.member_idx.resize(P->n_members);
  for (int32_t c = 0; c < P->n_channels; ++c)
    for (int32_t m = P->ch_member_off[c]; m < P->ch_member_off[c + 1]; ++m) {
      auto& idx = H.member_idx[m];
      for (int32_t p = P->mb_piece_off[m]; p < P->mb_piece_off[m + 1]; ++p)
        idx.push_back(ax.search_left(P->ch_tshift[c], P->pc_bound[p]));
    }
  // Mean length of the live member pieces (samples).  Below WFK_SH_MAXLEN the plan is compiled for
  // the contiguous-lane geometry: lane stride = one sample, WFK_SH_R samples per lane.
  // (the tier's records and the fir_short window entries hold sample indices as 32-bit words: a row of
  // 2^31 samples or more stays on the standard tiers, which index in 64 bits)
  if (at.want_short == 0 || !ax.g || env.disable_fast || at.ns_override != 0 || ax.n <= 0 || ax.n >= ((int64_t)1 << 31))
    return false;
  int64_t live = 0, live_samples = 0;
  for (int32_t m = 0; m < P->n_members; ++m) {
    const auto& idx = H.member_idx[m];
    int64_t prev = 0;
    for (size_t k = 0; k < idx.size(); ++k) {
      const int32_t p = P->mb_piece_off[m] + (int32_t)k;
      if (idx[k] > prev && P->pc_term_off[p + 1] > P->pc_term_off[p]) { ++live; live_samples += idx[k] - prev; }
      prev = std::max(prev, idx[k]);
    }
  }
  H.mean_piece_len = live > 0 ? (double)live_samples / (double)live : 0.0;
  return env.short_mode != 0 && live > 0 && (env.short_mode == 1 || live_samples < env.short_maxlen * live);
}

// ---- workgroup chunking ------------------------------------------------------
static void chunking(const HostPlan& H, const ChunkRule& R, bool lean_geom, int32_t& tile, int32_t& tiles_per_chunk,
                     int64_t& chunks_per_ch, std::vector<int32_t>& chunk_first, int lean_cap = WFK_LEAN_TPC, int64_t lean_div = 2048) {
  tile = (lean_geom ? 64 : WFK_WG) * H.ns;
  const int64_t tiles_per_ch = (H.n + tile - 1) / tile;
  const int64_t total_tiles = tiles_per_ch * R.total_channels;
  // lean: one wave per workgroup; ~2-3k workgroups already fill 256 CUs x 12 waves.  Longer
  // chunks amortise the exact seeds, shorter ones keep the set of regions being written at
  // any moment compact, which is what the HBM write rate depends on:
  // measured best at 8 tiles (= one seed per chunk) on the headline config while a degree-1 op cost
  // 12 instructions per sample, at 5 since the phasor fold (8: same box 3.19 / 6: 3.11 / 5: 3.07 / 4: 3.16 ms);
  // 4 on C2.
  // Pieces of many ops (multi-tone pulses): a chunk's first tile seeds EVERY op exactly (libm: ~200 instructions
  // each), which at 5 tiles per chunk is as much work as the ops' own arithmetic -- longer chunks there
  // (ten tones per pulse, same box: 5 / 10 / 20 / 40 tiles 2.16 / 1.95 / 1.87 / 1.84 ms; four tones 1.34 / 1.27 / 1.22)
  if (lean_geom && lean_cap == WFK_LEAN_TPC && R.lean_units_max >= 5 && R.has_bank) lean_cap = 20;
  const int64_t tpc = total_tiles / (lean_geom ? lean_div : 8192);
  tiles_per_chunk = (int32_t)std::min<int64_t>(lean_geom ? lean_cap : 16, std::max<int64_t>(1, tpc));
  if (R.tpc) tiles_per_chunk = R.tpc;   // tuning override (WFK_TPC)
  chunks_per_ch = (tiles_per_ch + tiles_per_chunk - 1) / tiles_per_chunk;
  chunk_first.assign((size_t)(chunks_per_ch * H.n_channels), 0);
  const int64_t chunk_samples = (int64_t)tiles_per_chunk * tile;
  for (int32_t c = 0; c < H.n_channels; ++c) {
    int32_t p = H.channels[c].piece_begin;
    for (int64_t k = 0; k < chunks_per_ch; ++k) {
      int64_t g0 = k * chunk_samples;
      while (p < H.channels[c].piece_end - 1 && H.pieces[p].stop <= g0) ++p;
      chunk_first[(size_t)(c * chunks_per_ch + k)] = p;
    }
  }
}

// ---- the plan builder: one compile's state by lifetime, and the piece loop in named steps ----
#include "wfk_compile_builder.h"
#include "wfk_compile_factor.h"
#include "wfk_compile_fuse.h"
#include "wfk_compile_short.h"
#include "wfk_compile_piece.h"

// One compile.  Returns WFK_RETRY_STD when the short geometry was chosen but some piece cannot run in it.
static int compile_impl(const wfk_program* P, const wfk_grid* grid, const double* tlist, int64_t n_tlist, HostPlan& H,
                        std::string& err, const CompileRequest& req, const Attempt& at, const CompileEnv& env) {
  PhaseTimer ptimer;
  if (!P || (!grid && !tlist && n_tlist != 0)) { err = "null program or time axis"; return WFK_EINVAL; }
  if (P->n_channels < 0 || P->n_members < 0) { err = "negative counts"; return WFK_EINVAL; }
  TimeAxis ax{grid, tlist, grid ? grid->n : n_tlist};
  if (ax.n < 0) { err = "negative sample count"; return WFK_EINVAL; }
  H = HostPlan();
  H.tlist = grid == nullptr;
  H.n_channels = P->n_channels;
  H.n = ax.n;
  if (grid) {
    H.t0 = grid->t0; H.step = grid->step; H.last = grid->last; H.has_last = grid->has_last; H.i0 = grid->i0;
    if (grid->i0 < 0) { err = "negative grid.i0"; return WFK_EINVAL; }
    if (ax.n > 1 && !(grid->step > 0)) { err = "grid step must be positive"; return WFK_EINVAL; }
  }
  H.ns = H.tlist ? (req.tlist_ns > 0 ? req.tlist_ns : (ax.n < WFK_TLIST_SMALL_N ? WFK_NS_TLIST_SMALL : WFK_NS_TLIST)) : WFK_NS_GRID;
  if (at.ns_override > 0 && !H.tlist) H.ns = at.ns_override;
  H.tile = WFK_WG * H.ns;
  if (!req.program_validated)
    if (const int rc = validate_program(P, err)) return rc;
  ptimer.mark("validate");
  const bool shortm = search_members(P, ax, env, at, H);   // the plan is compiled for the short tier
  ptimer.mark("searchsorted");
  PlanBuilder PB(P, ax, H, err, req, at, env, shortm);
  ptimer.mark("setup");
  H.channels.resize(P->n_channels);
  H.channel_complex.assign(P->n_channels, 0);
  for (int32_t c = 0; c < P->n_channels; ++c)
    if (const int rc = PB.build_channel(c)) return rc;

  ptimer.mark("pieces+fusion");
  // ---- workgroup chunking ------------------------------------------------------
  // general kernel: workgroup = 4 waves, tile = 256*NS samples, chunk = tiles_per_chunk tiles
  // lean kernel   : workgroup = 1 wave,  tile = 64*NS samples (a wave owns a contiguous span)
  H.lean = PB.lean_ok && !PB.nolean && H.n_fused > 0 && !H.tlist;     // (time lists: fused ops run pointwise in the general kernel)
  // mixed plans: some pieces are lean, some are not (the erf edges of a flat-top pulse next to its
  // multi-tone plateau).  Two launches over the same output: the lean kernel takes the lean and the
  // zero pieces, the general kernel the rest -- every sample is still written exactly once.
  H.mixed = !H.lean && !H.tlist && PB.can_fuse && !PB.nolean && PB.n_lean_pieces > 0 && at.ns_override == 0 && !env.disable_mixed;
  // time lists: fully fused pieces on the pointwise build, the others on the build with the direct tier
  // (same chunking for both launches); all of one kind: a single launch of that build
  const bool tl_mixed = H.tlist && PB.n_lean_pieces > 0 && !PB.lean_ok;
  if (tl_mixed) H.mixed = true;
  H.lean_par = std::max(256, (H.lean_par + 63) / 64 * 64);      // >= the 2 KB every plan had so far
  const int32_t lean_units_max = H.lean_ops;                     // most state units of a lean piece (phasors + envelopes)
  H.lean_ops = std::max(8, H.lean_ops);                          // likewise: 8 units = 8 KB of state
  const ChunkRule R = {req.block_total_channels > 0 ? req.block_total_channels : P->n_channels, lean_units_max, PB.plan_has_bank, env.tpc};
  ptimer.mark("chunking");
  if (shortm) return short_tier_tables(H, {PB.n_short_pieces, PB.n_foreign_pieces, PB.n_short_samples, PB.n_foreign_samples}, R, env);

  chunking(H, R, H.lean, H.tile, H.tiles_per_chunk, H.chunks_per_ch, H.chunk_first);
  if (H.mixed && !H.tlist) chunking(H, R, true, H.lean_tile, H.lean_tiles_per_chunk, H.lean_chunks_per_ch, H.lean_chunk_first);
  if ((H.lean || H.mixed) && at.ns_override == 0 && !H.tlist) {
    // the lean launch's chunking for float outputs (longer chunks, see HostPlan)
    int32_t tile32 = 0;
    const int cap32 = env.tpc_f32 ? env.tpc_f32 : WFK_LEAN_TPC_F32;   // (tuning override)
    // (beyond the double table's 8 tiles only where at least ~8 chunks per resident wave remain: C3's
    //  250 k tiles run best at 8-10 tiles per chunk -- 0.201 ms against 0.219 at 20 -- the 2.5 M tiles of
    //  256 x 1e7 at 16-20)
    chunking(H, R, true, tile32, H.f32_tiles_per_chunk, H.f32_chunks_per_ch, H.f32_chunk_first, cap32, 24576);
    if (H.f32_tiles_per_chunk <= (H.mixed ? H.lean_tiles_per_chunk : H.tiles_per_chunk)) {
      H.f32_chunk_first.clear();      // nothing to gain: the double table serves
      H.f32_tiles_per_chunk = 0;
    }
  }
  H.pool_real = !H.pool.empty();
  if (H.pool.empty()) H.pool.push_back(0.0);
  if (H.params.empty()) H.params.push_back(0.0);
  return WFK_OK;
}

// Grid plan for another evaluation geometry: lanes `lane_stride` samples apart, `ns` samples per
// lane (the sampler fused into the FIR transform walks a window with stride 256, wfk_fir_sampled.hip).
// Only the piece / parameter tables are meaningful in the result; H.lean tells whether every piece
// is one block of fused ops (the only form that kernel evaluates).
int wfk_compile_geom(const wfk_program* P, const wfk_grid* grid, int lane_stride, int ns, HostPlan& H, std::string& err) {
  const Attempt geom = {/*allow_corr*/ false, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ false, lane_stride, ns};
  return compile_impl(P, grid, nullptr, 0, H, err, CompileRequest(), geom, CompileEnv());
}

// The retry ladder: a plan is compiled for the most specific tier first, and again for a more general one where it does not fit.
//  * Carriers whose phase is sensitive to NumPy's grid rounding (far from t = 0) stay fused with a
//    first-order per-sample correction, which only the lean kernel implements.  A plan that turns
//    out not to be lean is compiled again with such carriers on the exact (libm) path.
//  * Plans whose live pieces are short (AWG sample rates: tens to hundreds of samples per pulse) are
//    compiled for the contiguous-lane geometry of wfk_short.hip first; a piece that tier cannot take
//    (generic terms, erf edges, corrected carriers) sends the whole plan back to the standard tiers.
static int compile_ladder(const wfk_program* P, const wfk_grid* grid, const double* tlist, int64_t n_tlist, HostPlan& H,
                          std::string& err, const CompileRequest& req, const CompileEnv& env) {
  auto attempt = [&](HostPlan& out, std::string& e, const Attempt& at) { return compile_impl(P, grid, tlist, n_tlist, out, e, req, at, env); };
  int rc = attempt(H, err, {/*allow_corr*/ true, /*want_short*/ -1, /*no_short_corr*/ false, /*no_chirp*/ false});
  if (rc == WFK_OK && H.shortp && H.short_corr && H.short_fam != 6) {
    // corrected carriers next to closing ops / chirps / tables: no family of the short tier holds both -- the attempt
    // again without the tier's correction (those carriers' pieces then go the way they went before family 6)
    H = HostPlan();
    rc = attempt(H, err, {/*allow_corr*/ true, /*want_short*/ -1, /*no_short_corr*/ true, /*no_chirp*/ false});
  }
  const bool gave_up = rc == WFK_RETRY_STD;
  const double mean_len = H.mean_piece_len;      // (of the first compile: the later ones do not take the short-tier decision)
  if (rc == WFK_RETRY_STD)
    rc = attempt(H, err, {/*allow_corr*/ true, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ false});
  else if (rc == WFK_OK && H.shortp && H.short_needs_corr) {
    // far from t = 0 fast carriers need the per-sample rounding correction, which only the lean kernel
    // has: where the standard tiers can run the plan lean (pieces long enough for its recurrences) they
    // win; otherwise the short tier keeps what it can take and libm serves those carriers either way
    HostPlan S; std::string e2;
    const int rcs = attempt(S, e2, {/*allow_corr*/ true, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ false});
    if (rcs == WFK_OK && (S.lean || S.mixed)) H = std::move(S);
  }
  if (rc == WFK_OK && !H.shortp && H.n_corr > 0 && !H.lean && !H.mixed)
    rc = attempt(H, err, {/*allow_corr*/ false, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ false});
  if (rc == WFK_OK && !H.shortp && H.n_corr > 0 && H.lean_fam >= 2) {
    // corrected carriers (far from t = 0) and fused chirps in one plan: the lean kernel is not instantiated
    // for that combination; the chirps take the general path
    rc = attempt(H, err, {/*allow_corr*/ true, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ true});
    if (rc == WFK_OK && H.n_corr > 0 && !H.lean && !H.mixed)
      rc = attempt(H, err, {/*allow_corr*/ false, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ true});
  }
  // pieces of AWG-rate length that the short tier could not take: the standard tiers walk every piece over whole wave
  // tiles of 1024 samples (wfk_api.cpp: such grid plans are evaluated pointwise instead)
  // (not where the standard compile came out lean: chirp pulses stay on the lean kernel's chirp family, measured
  //  12.6 ms against 17.6 pointwise on 2048 x 1e5 at 2 GS/s; and only for pieces well below a wave tile: from a few
  //  hundred samples per piece on, the general kernel's per-factor fast paths cost less than pointwise libm)
  if (rc == WFK_OK) H.short_gave_up = gave_up && grid != nullptr && !H.lean && !H.mixed && mean_len > 0.0 && mean_len < 192.0;
  // A short plan that hands more than a few per cent of its samples on: on 2e8 samples the general kernel's launch over those
  // pieces costs ~1.25 ms per per cent (every piece over a wave tile) next to 0.4 ms for the short pieces; evaluated pointwise
  // the fused pieces take ~4.5 ms and the rest 0.34 ms per per cent (rocprofv3 --stats, one exponential chirp in ten
  // pulses: 12.9 -> 7.9 ms) -- break-even near 4.5 %
  if (rc == WFK_OK && grid && H.shortp && H.mixed && H.foreign_frac >= 0.05 && mean_len > 0.0 && mean_len < 192.0 &&
      !req.keep_mixed_short && !env.keep_mixed_short)
    H.short_gave_up = true;
  return rc;
}

int wfk_compile(const wfk_program* P, const wfk_grid* grid, const double* tlist, int64_t n_tlist, HostPlan& H, std::string& err, const CompileRequest& req) {
  return compile_ladder(P, grid, tlist, n_tlist, H, err, req, CompileEnv());
}

// ---- big batches: channel blocks compiled on host threads ---------------------------------------
// The compile is O(#pieces) of scalar work with long-double seeds per op (2 us per piece): a fresh AWG sequence of
// 2048 rows x 1668 pulses is 7 s on one core.  Channels are independent (reference: one Waveform per channel,
// waveforms/waveform.py:529-563), so the job is cut into contiguous channel blocks, every block is compiled by
// compile_ladder on its own thread into its own HostPlan, and the plans are concatenated (indices rebased).  Taken for the
// two bulk shapes -- pure short-tier plans (their tables move with them) and pure lean plans without pool tables; anything
// else (mixed tiers, lean plans with INTERP / mollifier / SAMPLED tables, blocks that chose different tiers) returns WFK_RETRY_STD and the caller compiles in one piece.
int wfk_compile_blocks(const wfk_program* P, const wfk_grid* grid, int nthreads, HostPlan& H, std::string& err,
                       const CompileRequest& req) {
  if (!P || !grid || nthreads < 2 || P->n_channels < 2 * nthreads) return WFK_RETRY_STD;
  const CompileEnv env;
  {
    // validate the whole program once, here (a block skips it): a grid of zero points is enough for that (a whole compile, not
    // validate_program alone: compile_impl's own refusals of negative counts and of a negative grid.i0 are reached on zero points too)
    HostPlan V;
    wfk_grid g0 = *grid;
    g0.n = 0; g0.has_last = 0;
    const int rc = compile_impl(P, &g0, nullptr, 0, V, err, req,
                                {/*allow_corr*/ true, /*want_short*/ 0, /*no_short_corr*/ false, /*no_chirp*/ false}, env);
    if (rc != WFK_OK && rc != WFK_RETRY_STD) return rc;
  }
  const int K = nthreads;
  std::vector<HostPlan> parts((size_t)K);
  std::vector<std::string> errs((size_t)K);
  std::vector<int> rcs((size_t)K, WFK_OK);
  std::vector<int32_t> first((size_t)K + 1);
  for (int k = 0; k <= K; ++k) first[k] = (int32_t)((int64_t)P->n_channels * k / K);
  // a block: the program's channel arrays are views into the job's (ch_member_off does not start at 0), the job was
  // validated above, and the launch geometry (tiles per chunk) is decided on the job's channel count
  CompileRequest block = req;
  block.block_total_channels = P->n_channels;
  block.program_validated = true;
  auto work = [&](int k) {
    wfk_program Q = *P;
    const int32_t a = first[k];
    Q.n_channels = first[k + 1] - a;
    Q.ch_member_off += a; Q.ch_offset += a; Q.ch_tshift += a; Q.ch_clip_lo += a; Q.ch_clip_hi += a;
    try {
      rcs[k] = compile_ladder(&Q, grid, nullptr, 0, parts[k], errs[k], block, env);
    } catch (...) {
      rcs[k] = WFK_ENOMEM;
      errs[k] = "out of host memory while compiling a channel block";
    }
  };
  {
    std::vector<std::thread> th;
    int started = 1;
    try {
      for (; started < K; ++started) th.emplace_back(work, started);
    } catch (...) {
    }
    work(0);
    for (auto& t : th) t.join();
    for (int k = started; k < K; ++k) work(k);               // (threads that could not be had)
  }
  for (int k = 0; k < K; ++k)
    if (rcs[k] != WFK_OK) { err = errs[k]; return rcs[k] == WFK_ENOMEM ? WFK_ENOMEM : WFK_RETRY_STD; }
  const HostPlan& A = parts[0];
  if (A.tlist || A.mixed || A.grid_as_tlist || !(A.shortp || A.lean)) return WFK_RETRY_STD;
  for (const HostPlan& B : parts)
    if (B.shortp != A.shortp || B.lean != A.lean || B.mixed || (B.pool_real && !B.shortp) || B.short_gave_up || B.ns != A.ns || B.tile != A.tile ||
        B.tiles_per_chunk != A.tiles_per_chunk || B.chunks_per_ch != A.chunks_per_ch ||
        B.f32_tiles_per_chunk != A.f32_tiles_per_chunk || B.f32_chunks_per_ch != A.f32_chunks_per_ch ||
        (B.n_corr > 0) != (A.n_corr > 0))
      return WFK_RETRY_STD;
  {
    // corrected carriers (family 6) in one block, closing ops / tables (families 1, 2, 4) in another: no build has both
    bool any_corr = false, any_other = false;
    for (const HostPlan& B : parts) {
      any_corr = any_corr || B.short_corr;
      any_other = any_other || (B.shortp && B.short_fam != 0 && B.short_fam != 6);
    }
    if (any_corr && any_other) return WFK_RETRY_STD;
  }
  H = HostPlan();
  H.tlist = false; H.n_channels = P->n_channels; H.n = A.n;
  H.t0 = A.t0; H.step = A.step; H.last = A.last; H.has_last = A.has_last; H.i0 = A.i0;
  H.ns = A.ns; H.tile = A.tile; H.tiles_per_chunk = A.tiles_per_chunk; H.chunks_per_ch = A.chunks_per_ch;
  H.lean = A.lean; H.shortp = A.shortp; H.mixed = false;
  H.f32_tiles_per_chunk = A.f32_tiles_per_chunk; H.f32_chunks_per_ch = A.f32_chunks_per_ch;
  H.lean_tile = A.lean_tile; H.lean_tiles_per_chunk = A.lean_tiles_per_chunk; H.lean_chunks_per_ch = A.lean_chunks_per_ch;
  H.member_idx.resize((size_t)P->n_members);
  double len_sum = 0.0, frac_sum = 0.0;
  for (int k = 0; k < K; ++k) {
    HostPlan& B = parts[k];
    if (H.params.size() & 1) H.params.push_back(0.0);
    const int64_t po = (int64_t)H.params.size();             // even: records keep their 16-byte alignment
    const int32_t pc = (int32_t)H.pieces.size(), so = (int32_t)H.s_slots.size();
    for (DevChannel c : B.channels) { c.piece_begin += pc; c.piece_end += pc; H.channels.push_back(c); }
    if (B.pool_real) {
      // short plans with tables (INTERP envelopes, sampled flat-top edges): the block's pool goes behind the others', and
      // the ops that name a table -- own-term ops over a table, closing table multipliers: [9], in 16-byte entries -- move with it
      if (H.pool.size() & 1) H.pool.push_back(0.0);
      const double tb = (double)(H.pool.size() / 2);
      H.pool.insert(H.pool.end(), B.pool.begin(), B.pool.end());
      for (const DevPiece& d : B.pieces) {
        if (d.n_blk <= 0 || !(d.flags & WFK_PF_SHORT)) continue;
        for (int32_t r = 0; r < d.n_blk; ++r) {
          double* o = B.params.data() + d.par_off + (int64_t)r * d.first_len;
          double* const end = o + d.first_len;
          while (o < end) {
            uint64_t word;
            std::memcpy(&word, o, sizeof word);
            const uint32_t w = (uint32_t)word;
            if (((w >> 4) & 3) == 3 && ((w & 128) ? !(w & 256) : (!(w & 1024) && (w & 3) == 2))) o[9] += tb;
            if (w & WFK_SH_LAST) break;
            o += (w & 3) > 1 ? WFK_SH_OP3 : WFK_SH_OP1;
          }
        }
      }
    }
    for (DevPiece d : B.pieces) { if (d.n_blk > 0) d.par_off += po; else d.par_off = po; H.pieces.push_back(d); }
    H.params.insert(H.params.end(), B.params.begin(), B.params.end());
    for (int32_t v : B.chunk_first) H.chunk_first.push_back(v + pc);
    for (int32_t v : B.f32_chunk_first) H.f32_chunk_first.push_back(v + pc);
    H.channel_complex.insert(H.channel_complex.end(), B.channel_complex.begin(), B.channel_complex.end());
    for (ShortUnit u : B.s_units) { u.ch += first[k]; u.slot0 += so; u.rec0 += po / 2; H.s_units.push_back(u); }
    H.s_slots.insert(H.s_slots.end(), B.s_slots.begin(), B.s_slots.end());
    for (size_t m = 0; m < B.member_idx.size(); ++m)
      if (!B.member_idx[m].empty()) H.member_idx[m] = std::move(B.member_idx[m]);
    H.n_fast += B.n_fast; H.n_direct += B.n_direct; H.n_fused += B.n_fused; H.n_generic += B.n_generic; H.n_corr += B.n_corr;
    H.lean_fam = std::max(H.lean_fam, B.lean_fam);
    H.lean_par = std::max(H.lean_par, B.lean_par); H.lean_ops = std::max(H.lean_ops, B.lean_ops);
    H.max_block_len = std::max(H.max_block_len, B.max_block_len);
    H.s_lds_samples = std::max(H.s_lds_samples, B.s_lds_samples);
    H.short_has_fmul = H.short_has_fmul || B.short_has_fmul;
    H.short_fam = std::max(H.short_fam, B.short_fam);
    H.short_needs_corr = H.short_needs_corr || B.short_needs_corr;
    H.short_corr = H.short_corr || B.short_corr;
    len_sum += B.mean_piece_len * (double)B.n_channels; frac_sum += B.foreign_frac * (double)B.n_channels;
  }
  H.mean_piece_len = len_sum / (double)P->n_channels;
  H.foreign_frac = frac_sum / (double)P->n_channels;
  H.pool_real = !H.pool.empty();
  if (H.pool.empty()) H.pool.assign(1, 0.0);
  if (H.shortp) short_chunks(H, env);
  return WFK_OK;
}

// ---- uniform-grid detection -----------------------------------------------------------------
// Waveform.__call__(x) takes any sorted array (reference waveform.py:529-563), but scripts
// almost always pass np.linspace / np.arange output.  If x is BIT-IDENTICAL to the grid formula
// t[i] = fl(fl(i*step) + t0) (optionally with the last element overridden, np.linspace
// endpoint=True) the plan can be compiled in grid mode -- fused ops instead of one libm call per
// factor and sample, no upload of x -- and the device regenerates exactly the caller's times.
// The check is exact (every element is compared); anything else stays in tlist mode.
namespace {

struct GridProbe {
  const double* t;
  int64_t n;
  double t0;
  // (this file is built with -ffp-contract=off: the product rounds before the sum, as NumPy's does)
  double at(int64_t i, double step) const { return (double)i * step + t0; }
  // first index in [a, b) where the formula differs from t, or -1; *sign = formula - t there
  int64_t first_mismatch(double step, int64_t a, int64_t b, int* sign) const {
    for (int64_t c = a; c < b; c += 1024) {       // branch-free blocks (vectorisable), then locate
      const int64_t e = std::min(b, c + 1024);
      int bad = 0;
      const double dc = (double)c;                // c + k is exact in double (indices < 2^53)
      const double* tc = t + c;
      const int len = (int)(e - c);
      for (int k = 0; k < len; ++k) bad |= ((dc + (double)k) * step + t0) != tc[k];
      if (!bad) continue;
      for (int64_t i = c; i < e; ++i) {
        const double g = at(i, step);
        if (g != t[i]) {
          if (sign) *sign = g < t[i] ? -1 : 1;   // (a NaN in t lands in +1: never bracketed)
          return i;
        }
      }
    }
    return -1;
  }
  int64_t verify(double step, int64_t count, int* sign) const {
    if (count < (int64_t(1) << 20)) return first_mismatch(step, 0, count, sign);
    constexpr int nt = 8;
    std::atomic<int64_t> worst(INT64_MAX);
    int signs[nt] = {0};
    int64_t at_[nt];
    for (int k = 0; k < nt; ++k) at_[k] = -1;
    std::vector<std::thread> th;
    auto work = [&](int k) {
        const int64_t a = count * k / nt, b = count * (k + 1) / nt;
        // blocks of 64k so that a thread stops early once an earlier mismatch is known
        for (int64_t s0 = a; s0 < b && s0 < worst.load(std::memory_order_relaxed); s0 += 65536) {
          const int64_t m = first_mismatch(step, s0, std::min(b, s0 + 65536), &signs[k]);
          if (m >= 0) {
            at_[k] = m;
            int64_t w = worst.load();
            while (m < w && !worst.compare_exchange_weak(w, m)) {}
            break;
          }
        }
    };
    // (no exception may cross the C boundary: if threads cannot be had the slices run here)
    int started = 0;
    try {
      for (; started < nt - 1; ++started) th.emplace_back(work, started);
    } catch (...) {
    }
    for (int k = started; k < nt; ++k) work(k);
    for (auto& x : th) x.join();
    for (int k = 0; k < nt; ++k)
      if (at_[k] >= 0) { if (sign) *sign = signs[k]; return at_[k]; }   // lowest thread = lowest index
    return -1;
  }
};

}  // namespace

extern "C" int wfk_grid_detect(const double* t, int64_t n, wfk_grid* out) {
  if (!t || !out || n < 16) return 0;
  GridProbe P{t, n, t[0]};
  if (!(t[n - 1] > t[0]) || !std::isfinite(t[0]) || !std::isfinite(t[n - 1])) return 0;
  auto accept = [&](double step, int has_last) {
    out->t0 = t[0]; out->step = step; out->n = n; out->has_last = has_last; out->i0 = 0;
    out->last = has_last ? t[n - 1] : 0.0;
    return 1;
  };
  // np.linspace(a, b, n) (endpoint=True): step = (b - a) / (n - 1), last element := b
  {
    const double step = (t[n - 1] - t[0]) / (double)(n - 1);
    if (step > 0 && P.first_mismatch(step, 1, 16, nullptr) < 0 && P.verify(step, n - 1, nullptr) < 0)
      return accept(step, 0 + 1);
  }
  // np.arange(start, stop, d): t[1] - t[0] is the element step itself
  {
    const double step = t[1] - t[0];
    if (step > 0 && P.first_mismatch(step, 1, 16, nullptr) < 0 && P.verify(step, n, nullptr) < 0)
      return accept(step, 0);
  }
  // np.linspace(..., endpoint=False) and anything else of the same form: the step is not one of
  // the two above, but fl(fl(i*s) + t0) is monotone in s, so it is found by bisection over the
  // doubles between two brackets, on a subset of indices that grows with every counter-example.
  std::vector<int64_t> probe;
  for (int64_t i = n - 1; i >= 1; i = i * 7 / 8 - (i < 8 ? 1 : 0)) probe.push_back(i);
  auto classify = [&](double s) {   // -1: too small, +1: too big, 0: fits the subset, 2: contradiction
    bool lo = false, hi = false;
    for (int64_t i : probe) {
      const double g = P.at(i, s);
      lo = lo || g < t[i];
      hi = hi || g > t[i];
    }
    return lo && hi ? 2 : (lo ? -1 : (hi ? 1 : 0));
  };
  const double est = (t[n - 1] - t[0]) / (double)(n - 1);
  const double slack = 8.0 * (std::fabs(t[0]) + std::fabs(t[n - 1])) * 2.3e-16 / (double)(n - 1) + est * 1e-15;
  double lo = est - slack, hi = est + slack;
  if (!(lo > 0) || classify(lo) != -1 || classify(hi) != 1) return 0;
  for (int iter = 0; iter < 400; ++iter) {
    const double mid = lo + (hi - lo) / 2;
    if (!(mid > lo && mid < hi)) return 0;            // adjacent doubles: no step reproduces x
    const int c = classify(mid);
    if (c == 2) return 0;
    if (c < 0) { lo = mid; continue; }
    if (c > 0) { hi = mid; continue; }
    int sign = 0;
    const int64_t bad = P.verify(mid, n, &sign);
    if (bad < 0) return accept(mid, 0);
    probe.push_back(bad);                             // the counter-example narrows the bracket
    if (sign < 0) lo = mid; else hi = mid;
  }
  return 0;
}

// A sorted x that is several NumPy grids back to back -- np.concatenate of the chunks of a chunked job
// (waveforms/waveform.py:232: one np.linspace(..., endpoint=False) per chunk), a sequence sampled at two
// rates -- splits into runs that each pass wfk_grid_detect.  Run boundaries are where the spacing changes by
// more than the rounding of the grid formula can explain; every run is then verified element by element.
// -> number of runs (starts[k], grids[k]; the last run ends at n), 0 if x is not such a concatenation
//    (a run shorter than `min_len`, more than `max_runs` runs, one element off anywhere).
extern "C" int wfk_grid_detect_runs(const double* t, int64_t n, int64_t min_len, int32_t max_runs,
                                    int64_t* starts, wfk_grid* grids) {
  if (!t || !starts || !grids || n < 32 || max_runs < 1) return 0;
  if (min_len < 16) min_len = 16;
  std::vector<int64_t> cuts = {0};
  const double scale = 8.0 * 2.3e-16 * (std::max(std::fabs(t[0]), std::fabs(t[n - 1])) + std::fabs(t[n - 1] - t[0]));
  double prev = t[1] - t[0];
  int64_t run0 = 0;
  for (int64_t i = 1; i + 1 < n; ++i) {
    const double d = t[i + 1] - t[i];
    // within a grid the spacing wobbles by a few ulp of |t| (two roundings per element); a new grid starts
    // with a jump or with another step
    // (a few ulp of the largest |t| or |i * step| of ANY run: near t = 0 a grid's own wobble is that of
    //  its fl(i * step), not of the tiny t)
    const double tol = scale + 1e-12 * std::fabs(prev);
    if (!(std::fabs(d - prev) <= tol)) {
      // t[i + 1] opens a new run (the odd spacing is the gap between the runs) -- unless the run so far is
      // a single gap itself, i.e. two breaks in a row
      if (i + 1 - run0 < min_len) return 0;
      cuts.push_back(i + 1);
      if ((int64_t)cuts.size() > max_runs) return 0;
      run0 = i + 1;
      if (i + 2 < n) { prev = t[i + 2] - t[i + 1]; ++i; } else break;
    } else {
      prev = d;
    }
  }
  if (n - run0 < min_len) return 0;
  for (size_t k = 0; k < cuts.size(); ++k) {
    const int64_t a = cuts[k], b = k + 1 < cuts.size() ? cuts[k + 1] : n;
    if (!wfk_grid_detect(t + a, b - a, &grids[k])) return 0;
    starts[k] = a;
  }
  return (int)cuts.size();
}

// ---- sampler fused into the FIR transform at AWG rates: half-window entry lists ----------------------
// (reference chain: waveform.py:190-192 -> distortion.py:329-337; consumer: fir_short, wfk_fir_sampled.hip)
int wfk_chain_windows(const HostPlan& H, int64_t n, int64_t hop, int64_t lead, int64_t half_len, int64_t npairs,
                      std::vector<ShortWin>& wins, std::vector<uint32_t>& ents, std::string& bad) {
  bad.clear();
  if (!H.shortp) { bad = "not a short plan"; return WFK_EINVAL; }
  if (H.short_has_fmul) { bad = "table / mollifier envelopes (closing multipliers the fused chain does not evaluate)"; return WFK_EINVAL; }
  if (H.short_corr) { bad = "carriers with the grid-rounding correction (family 6 of the short tier: fir_short does not evaluate them)"; return WFK_EINVAL; }
  if (half_len <= 0 || half_len > 4096 || hop <= 0 || npairs < 0) { bad = "window geometry"; return WFK_EINVAL; }
  const int32_t nch = (int32_t)H.channels.size();
  wins.assign((size_t)npairs * nch * 2, ShortWin{});
  ents.clear();
  ents.reserve((size_t)(n / 12) * nch);
  for (int32_t c = 0; c < nch && bad.empty(); ++c) {
    const int32_t pe = H.channels[c].piece_end;
    int32_t q = H.channels[c].piece_begin;
    for (int64_t pr = 0; pr < npairs && bad.empty(); ++pr) {
      const int64_t s1 = 2 * pr * hop - lead;
      while (q < pe - 1 && H.pieces[q].stop <= s1) ++q;
      for (int hf = 0; hf < 2; ++hf) {
        const int64_t h0 = s1 + half_len * hf;
        const int64_t w0 = std::max<int64_t>(h0, 0), w1 = std::min<int64_t>(h0 + half_len, n);
        ShortWin W{};
        W.rec0 = -1;
        W.e0 = (int64_t)ents.size();
        for (int32_t qq = q; qq < pe && H.pieces[qq].start < w1; ++qq) {
          const DevPiece& D = H.pieces[qq];
          if (D.n_blk == 0 || D.stop <= w0) continue;          // zero stretch (the prefill) / before the half
          if (!(D.flags & WFK_PF_SHORT)) continue;             // the general kernel's piece: copied, below
          const int64_t a0 = std::max(D.start, w0), b0 = std::min(D.stop, w1);
          for (int64_t m = (a0 - D.start) / WFK_SH_SUB; D.start + m * WFK_SH_SUB < b0; ++m) {
            const int64_t r0 = D.start + m * WFK_SH_SUB, r1 = std::min<int64_t>(r0 + WFK_SH_SUB, D.stop);
            const int64_t aa = std::max(a0, r0), bb = std::min(b0, r1), len = bb - aa;
            if (len <= 0) continue;
            const int64_t rec16 = (D.par_off + m * (int64_t)D.first_len) / 2;
            if (W.rec0 < 0) W.rec0 = rec16;
            if (rec16 - W.rec0 > 0xffff) { bad = "op records of one window span more than 1 MB"; break; }
            const int64_t nsg = (len + WFK_SH_R - 1) / WFK_SH_R, bl = len / nsg, rem = len % nsg;
            int64_t k0 = 0;
            for (int64_t sg = 0; sg < nsg; ++sg) {
              const int64_t sl = bl + (sg < rem ? 1 : 0);
              ents.push_back(WFK_CW_ENTRY(rec16 - W.rec0, aa + k0 - h0, sl));
              k0 += sl;
            }
          }
          if (!bad.empty()) break;
        }
        if (W.rec0 < 0) W.rec0 = 0;
        W.cnt = (int32_t)((int64_t)ents.size() - W.e0);
        {
          // LDS layout of the half: per wave of 64 entries, the fullest of the 16 bank pairs the runs'
          // first elements fall into, plain vs padded
          int64_t cp = 0, cq = 0;
          for (int64_t e = W.e0; e < (int64_t)ents.size(); e += 64) {
            int plain[16] = {0}, padded[16] = {0}, wp = 0, wq = 0;
            for (int64_t k = e; k < std::min<int64_t>(e + 64, (int64_t)ents.size()); ++k) {
              const int o = (int)((ents[(size_t)k] >> 16) & 0xfff);
              wp = std::max(wp, ++plain[o & 15]);
              wq = std::max(wq, ++padded[(o + (o >> 4)) & 15]);
            }
            cp += wp; cq += wq;
          }
          W.pad = cq < cp ? 1 : 0;
        }
        if (H.mixed) {
          for (int32_t qq = q; qq < pe && H.pieces[qq].start < w1; ++qq) {
            const DevPiece& D = H.pieces[qq];
            if (D.n_blk == 0 || D.stop <= w0 || (D.flags & WFK_PF_SHORT)) continue;
            const int64_t a0 = std::max(D.start, w0), b0 = std::min(D.stop, w1);
            for (int64_t at = a0; at < b0; at += WFK_SH_R)
              ents.push_back(WFK_CW_ENTRY(0, at - h0, std::min<int64_t>(WFK_SH_R, b0 - at)));
          }
          W.ccnt = (int32_t)((int64_t)ents.size() - W.e0 - W.cnt);
        }
        wins[((size_t)c * npairs + pr) * 2 + hf] = W;
      }
    }
  }
  return bad.empty() ? WFK_OK : WFK_EINVAL;
}

// diagnostics (tools/): piece statistics of a plan compiled for another geometry -- out[0] pieces, out[1] live pieces,
// out[2] shortest / out[3] longest live piece (samples), out[4] lean, out[5] largest first_len
extern "C" int wfk_internal_geom_stats(const wfk_program* P, const wfk_grid* grid, int lane_stride, int ns, int64_t* out) {
  HostPlan H;
  std::string err;
  const int rc = wfk_compile_geom(P, grid, lane_stride, ns, H, err);
  if (rc) return rc;
  int64_t live = 0, lo = INT64_MAX, hi = 0, fl = 0;
  for (const DevPiece& p : H.pieces)
    if (p.n_blk > 0) {
      ++live;
      lo = std::min(lo, p.stop - p.start);
      hi = std::max(hi, p.stop - p.start);
      fl = std::max<int64_t>(fl, p.first_len);
    }
  out[0] = (int64_t)H.pieces.size(); out[1] = live; out[2] = live ? lo : 0; out[3] = hi; out[4] = H.lean; out[5] = fl;
  return 0;
}

