// wfk_compile_piece.h -- the piece loop of the host plan compiler: a channel's members merged into disjoint
// device pieces, and every piece built in named steps (PlanBuilder, wfk_compile_builder.h).
// Included by wfk_compile.cpp only.
#pragma once

namespace {

// ---- merge members into disjoint device pieces -----------------------------
int PlanBuilder::build_channel(int32_t c) {
  DevChannel& C = H.channels[c];
  C.offset = P->ch_offset[c]; C.tshift = P->ch_tshift[c];
  C.clip_lo = P->ch_clip_lo[c]; C.clip_hi = P->ch_clip_hi[c];
  C.do_clip = (C.clip_lo != -INFINITY || C.clip_hi != INFINITY) ? 1 : 0;
  C.pad = 0;
  C.piece_begin = (int32_t)H.pieces.size();
  ch = c;
  tshift = C.tshift;
  const int32_t m0 = P->ch_member_off[c], m1 = P->ch_member_off[c + 1];
  std::vector<int64_t> cuts = {0, ax.n};
  for (int32_t m = m0; m < m1; ++m)
    cuts.insert(cuts.end(), H.member_idx[m].begin(), H.member_idx[m].end());
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
  std::vector<int32_t> cur(m1 - m0, 0);  // per member: current piece (relative)
  for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
    s0 = cuts[ci]; s1 = cuts[ci + 1];
    if (s0 < 0 || s1 > ax.n || s0 >= s1) continue;
    collect_live(m0, m1, cur);
    if (const int rc = build_piece()) return rc;
    // fuse adjacent zero pieces
    if (D.n_blk == 0 && (int32_t)H.pieces.size() > C.piece_begin &&
        H.pieces.back().n_blk == 0 && H.pieces.back().stop == s0) {
      H.pieces.back().stop = s1;
    } else {
      H.pieces.push_back(D);
    }
  }
  C.piece_end = (int32_t)H.pieces.size();
  return WFK_OK;
}

// step 1: the live member pieces over [s0, s1), and the jitter budget their terms share
void PlanBuilder::collect_live(int32_t m0, int32_t m1, std::vector<int32_t>& cur) {
  live.clear();
  for (int32_t m = m0; m < m1; ++m) {
    const auto& idx = H.member_idx[m];
    int32_t& k = cur[m - m0];
    while (k < (int32_t)idx.size() - 1 && idx[k] <= s0) ++k;
    if (idx[k] <= s0) continue;  // past the last bound cannot happen (idx.back()==n)
    int32_t p = P->mb_piece_off[m] + k;
    if (P->pc_term_off[p + 1] > P->pc_term_off[p]) live.push_back(p);
  }
  int64_t nt = 0;
  for (int32_t p : live) nt += P->pc_term_off[p + 1] - P->pc_term_off[p];
  jtol = WFK_JITTER_TOL / std::max(1.0, (double)nt);
}

// One device piece.  It is built at most twice: the corrected (far-from-origin) carriers, the fused chirps and the
// stateless multipliers exist in the lean kernel only, so a piece that turns out NOT to be lean is built again
// without them; a short piece the tier cannot take is built again for the general kernel; a time-list piece is
// fused completely or not at all.  attempt_outcome holds every such exit.
int PlanBuilder::build_piece() {
  D = DevPiece{};
  D.start = s0; D.stop = s1; D.n_blk = 0; D.flags = 0; D.first_len = 0; D.pad = 0;
  if (H.params.size() & 1) H.params.push_back(0.0);
  D.par_off = (int64_t)H.params.size();
  snap = Snap{H.params.size(), H.pool.size(), H.n_fast, H.n_direct, H.n_fused, H.n_generic, H.n_corr, sampled_at, D};
  bool done = false;
  for (int a = 0; a < 2 && !live.empty() && !done; ++a) {
    begin_attempt(a);
    order_terms();
    fuse_terms();
    Outcome out = attempt_outcome(Stage::Fused);
    if (out == Outcome::Accept) {
      arrange_modulated();
      factor_shared_gaussian();
      mark_tone_banks();
      if (cur_short) {
        out = attempt_outcome(Stage::Arranged);
        if (out == Outcome::Accept) emit_short();
      } else {
        if (const int rc = emit_standard_piece()) return rc;
        out = attempt_outcome(Stage::Emitted);
        if (out == Outcome::Accept) classify_lean();
      }
    }
    switch (out) {
      case Outcome::Accept:
        done = true;
        break;
      case Outcome::AgainUnfused:
        restore(snap);
        piece_fuse_ok = false;
        break;
      case Outcome::AgainStandard:
        restore(snap);
        set_geom(false);
        ++n_foreign_pieces;
        n_foreign_samples += s1 - s0;
        break;
      case Outcome::AgainWithoutLeanOps:
        restore(snap);
        piece_corr_ok = false;
        piece_chirp_ok = false;
        piece_fmul_ok = false;
        break;
    }
  }
  piece_corr_ok = true;
  piece_chirp_ok = true;
  piece_fmul_ok = true;
  piece_fuse_ok = true;
  if (shortm) set_geom(true);
  return WFK_OK;
}

void PlanBuilder::begin_attempt(int attempt_no) {
  static_cast<TryState&>(*this) = TryState();
  attempt = attempt_no;
  corr_before = H.n_corr;
  // (a short plan: in its short pieces only -- the pieces that tier hands on run on the general kernel, which has no chirp op)
  chirp_ok = chirp_base && piece_chirp_ok && can_fuse && (!shortm || (cur_short && !req.no_short_fmul && !env.no_short_chirp));
  D.flags |= WFK_PF_HAS_TERMS;
  B = BlockBuilder();
}

// Takes back what an attempt at a piece wrote into the plan: H.params, H.pool, the five counters, sampled_at and
// the DevPiece go back to the snapshot.  fmul_tables and erf_tabs do NOT: an entry of theirs may then point past
// the end of the pool, or at what a later piece wrote there -- which is safe because their users (fmul_table,
// erf_table) check an entry against the pool's current size and contents before they trust it.
void PlanBuilder::restore(const Snap& snap) {
  H.params.resize(snap.params); H.pool.resize(snap.pool);
  H.n_fast = snap.nf; H.n_direct = snap.nd; H.n_fused = snap.nu; H.n_generic = snap.ng; H.n_corr = snap.nc;
  sampled_at = snap.sampled;
  D = snap.D;
}

// What becomes of the attempt: every tier-admission exit of a piece.  Asked where the facts are in: after the fuse
// pass, before a short piece is emitted, after a standard piece is.
Outcome PlanBuilder::attempt_outcome(Stage stage) {
  if (stage == Stage::Fused) {
    // Time lists evaluate fused ops pointwise in a build of the general kernel that holds nothing else
    // (with every libm shape of the direct tier next to them the kernel spills: measured 1.2 -> 2.3 ms on
    // flat-top pulses).  A piece is therefore either fused completely or not at all; a plan with both
    // kinds runs as two launches over disjoint pieces (H.mixed).
    if (H.tlist && !generic.empty() && !groups.empty() && attempt == 0) return Outcome::AgainUnfused;
    return Outcome::Accept;
  }
  if (stage == Stage::Arranged) {
    // compact records of the short tier (WFK_SH_*): one per <= WFK_SH_SUB samples of the piece.  A
    // piece that tier cannot take (generic terms: erf edges, chirps, ...) is built again for the
    // general kernel, in the standard geometry: the plan then runs as two launches (mixed).
    bool ok = generic.empty() && !groups.empty() && groups.size() <= 255 && !multi_bad;
    for (const FceGroup& G : groups)
      ok = ok && !(G.corr && (G.deg > 1 || G.chirp || G.fmul || G.erfmul || G.envmul || tshift != 0.0)) && !(G.chirp && G.deg > 1);
    return ok ? Outcome::Accept : Outcome::AgainStandard;
  }
  // Stage::Emitted: roll back and build the piece again without corrected carriers / fused chirps (lean kernel only)
  if ((!piece_lean && (H.n_corr > corr_before || piece_has_chirp || piece_has_fmul) && attempt == 0) ||
      ((multi_bad || (piece_has_fmul && H.n_corr > corr_before)) && attempt == 0))
    return Outcome::AgainWithoutLeanOps;
  return Outcome::Accept;
}

// step 2: the terms of the live member pieces, in the order they are fused
void PlanBuilder::order_terms() {
  groups.clear();
  generic.clear();
  order.clear();
  for (int32_t p : live)
    for (int32_t k = P->pc_term_off[p]; k < P->pc_term_off[p + 1]; ++k) order.push_back(k);
  if (can_fuse && corr_enabled) {
    // where a carrier needs the rounding correction the HEAVIEST term must found the group
    // (its COS factor is the one mimicked): visit the terms by descending amplitude there
    bool any = false;
    for (int32_t k : order)
      for (int32_t f = P->tm_factor_off[k]; f < P->tm_factor_off[k + 1] && !any; ++f)
        any = P->fc_type[f] == WFK_COS && !rate_safe_n(P->pool[P->fc_arg_off[f]], s0, s1);
    if (any) {
      auto weight_of = [&](int32_t k) {   // |amp| * max |LINEAR factors| over the piece
        double wgt = std::hypot(P->tm_amp_re[k], P->tm_amp_im[k]);
        for (int32_t f = P->tm_factor_off[k]; f < P->tm_factor_off[k + 1]; ++f)
          if (P->fc_type[f] == WFK_LINEAR) {
            const double ua = (ax.at(s0) - tshift) - P->fc_shift[f], ub = (ax.at(s1 - 1) - tshift) - P->fc_shift[f];
            wgt *= std::pow(std::max(std::fabs(ua), std::fabs(ub)), P->fc_power[f]);
          }
        return wgt;
      };
      std::stable_sort(order.begin(), order.end(),
                       [&](int32_t x, int32_t y) { return weight_of(x) > weight_of(y); });
    }
  }
}

bool PlanBuilder::same_mod(int32_t a_, int32_t b_) {
  const int64_t na = P->fc_arg_off[a_ + 1] - P->fc_arg_off[a_];
  if (P->fc_type[a_] != P->fc_type[b_] || P->fc_shift[a_] != P->fc_shift[b_] || na != P->fc_arg_off[b_ + 1] - P->fc_arg_off[b_]) return false;
  return P->fc_arg_off[a_] == P->fc_arg_off[b_] ||
         std::memcmp(P->pool + P->fc_arg_off[a_], P->pool + P->fc_arg_off[b_], (size_t)na * sizeof(double)) == 0;
}

// a term's ONE factor of a kind the closing multipliers take (power 1); -1: none, or not admissible here
// Short pieces may hold SEVERAL envelopes (overlapping pulses of different shapes: crosstalk-compensated channels),
// as long as each stands over one plain carrier: every such term is an own-term op, acc += F (A cos + B sin).
int32_t PlanBuilder::fmul_factor_of(int32_t k, int& kind_out) {
  if (!fmul_now || mod_kind == 1) return -1;
  fslot = 0;
  int32_t at = -1;
  for (int32_t f = P->tm_factor_off[k]; f < P->tm_factor_off[k + 1]; ++f)
    if (P->fc_type[f] == WFK_INTERP || P->fc_type[f] == WFK_MOLLIFIER ||
        (cur_short && !env.no_short_xchirp && (P->fc_type[f] == WFK_EXPONENTIALCHIRP || P->fc_type[f] == WFK_HYPERBOLICCHIRP))) {
      if (at >= 0 || P->fc_power[f] != 1.0) return -1;
      at = f;
    } else if (P->fc_type[f] == WFK_ERF) return -1;
  if (at < 0) return -1;
  const double* fa = P->pool + P->fc_arg_off[at];
  const int64_t na = P->fc_arg_off[at + 1] - P->fc_arg_off[at];
  const double sh = P->fc_shift[at];
  if (!std::isfinite(sh)) return -1;
  const int kind = P->fc_type[at] == WFK_INTERP ? 2 : (P->fc_type[at] == WFK_MOLLIFIER ? 3 :
                   (P->fc_type[at] == WFK_EXPONENTIALCHIRP ? 4 : 5));
  if (kind >= 4) {
    // Exponential / hyperbolic chirps at AWG rates (short pieces only): sin(phi0 + 2 pi f0 (exp(alpha u) - 1) / alpha) and
    // sin(phi0 + 2 pi f0 / k log(1 + k u)) (reference _waveform.pyx:326-332) have no recurrence form -- the phase does not
    // advance by a constant -- but as a MULTIPLIER of what the piece's other factors fuse to they cost one inline
    // exp step + one sine per sample (wfk_short_dev.h: short_xchirpmul) instead of a trip through the term interpreter
    // with device libm (one sample per lane: 10.6 ms for 2048 x 1e5 at 2 GS/s).  One such factor per piece.
    if (mod_f >= 0) { if (same_mod(at, mod_f)) { kind_out = kind; return at; } return -1; }
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(fa[i])) return -1;
    const double ua = (ax.at(s0) - tshift) - sh, ub = (ax.at(s1 - 1) - tshift) - sh;
    double wmax;
    if (kind == 4) {
      if (fa[1] == 0.0 || !(std::fabs(fa[1]) * std::max(std::fabs(ua), std::fabs(ub)) <= 600.0)) return -1;
      wmax = 6.283185307179586 * std::fabs(fa[0]) * std::exp(std::max(fa[1] * ua, fa[1] * ub));
    } else {
      const double la = 1.0 + fa[1] * ua, lb = 1.0 + fa[1] * ub;
      if (fa[1] == 0.0 || !(la > 1e-6) || !(lb > 1e-6)) return -1;
      wmax = 6.283185307179586 * std::fabs(fa[0]) / std::min(la, lb);
    }
    // (the phase itself is evaluated in double: its size times 2^-52 must stay inside the budget too)
    const double phmax = kind == 4 ? 6.283185307179586 * std::fabs(fa[0] / fa[1]) * (1.0 + std::exp(std::max(fa[1] * ua, fa[1] * ub)))
                                   : 6.283185307179586 * std::fabs(fa[0] / fa[1]) * std::max(std::fabs(std::log(1.0 + fa[1] * ua)), std::fabs(std::log(1.0 + fa[1] * ub)));
    if (!std::isfinite(wmax) || !rate_safe_n(wmax, s0, s1) || !(4.5e-16 * (phmax + std::fabs(fa[2])) <= jtol)) return -1;
    kind_out = kind;
    return at;
  }
  if (mod_f >= 0) {
    // one multiplier per piece: the same primitive, arguments and shift as the first term's
    if (same_mod(at, mod_f)) { kind_out = kind; return at; }
    if (!multi_ok) return -1;
    for (size_t i = 0; i < xmods.size(); ++i)
      if (same_mod(at, xmods[i].f)) { fslot = (int)i + 1; kind_out = kind; return at; }
    fslot = (int)xmods.size() + 1;      // a new envelope: admitted below
  }
  if (kind == 2) {
    // a finite table on increasing linspace knots, slopes inside the grid-rounding budget (as WFK_M_INTERP_LIN)
    const int64_t m = na - 2;
    const double start = fa[0], stop = fa[1];
    if (m < 2 || m > (int64_t(1) << 24) || !(stop > start) || !std::isfinite(start) || !std::isfinite(stop)) return -1;
    const double inv = (double)(m - 1) / (stop - start);
    if (!std::isfinite(inv)) return -1;
    double dmax = 0.0;
    for (int64_t j = 0; j < m; ++j) {
      if (!std::isfinite(fa[2 + j])) return -1;
      if (j + 1 < m) dmax = std::max(dmax, std::fabs(fa[3 + j] - fa[2 + j]));
    }
    if (!std::isfinite(dmax) || !rate_safe(4.0 * dmax * inv, s0, s1)) return -1;
    // the position in knot units, q = (x - start) * inv advanced by a tile's worth of additions: its
    // rounding (<= 2.5e-15 of the index range) times the largest step
    if (dmax * (double)m * 2.5e-15 > WFK_JITTER_TOL) return -1;
  } else {
    if (!(fa[1] == 0.0) || !std::isfinite(fa[0]) || !(fa[0] > 0.0) || !rate_safe(4.0 / fa[0], s0, s1)) return -1;
  }
  kind_out = kind;
  return at;
}

int32_t PlanBuilder::erf_factor_of(int32_t k, double& sg_out, double& sh_out) {
  if (!erfmod_base || mod_kind >= 2) return -1;
  int32_t at = -1;
  for (int32_t f = P->tm_factor_off[k]; f < P->tm_factor_off[k + 1]; ++f)
    if (P->fc_type[f] == WFK_ERF) {
      if (at >= 0 || P->fc_power[f] != 1.0) return -1;
      at = f;
    }
  if (at < 0) return -1;
  const double sg = P->pool[P->fc_arg_off[at]], sh = P->fc_shift[at];
  if (!std::isfinite(sg) || sg == 0.0 || !std::isfinite(sh)) return -1;
  if (!rate_safe(1.13 / sg, s0, s1)) return -1;
  if (!cur_short) {
    // lean kernel: the erf advances by its own Taylor step along the lane stride (fine grids only);
    // the short tier evaluates erf itself at every sample of the (short) edge piece
    if (!(std::fabs(dstride / sg) <= 0.09)) return -1;
    bool ok64, ok32;
    gauss_range(sg, sh, tshift, s0, s1, ok64, ok32);
    if (!ok64) return -1;
  }
  if (mod_on && (mod_sigma != sg || mod_shift != sh)) return -1;
  sg_out = sg; sh_out = sh;
  return at;
}

// step 3 (pass 1): fuse eligible terms into carrier-envelope groups; what does not fuse is left in `generic`.
// Terms with ONE erf factor (the edge of a flat-top pulse: square(width, edge), 0.5 + 0.5 erf)
// whose other factors fuse: the rest goes into a second group list, and a closing op multiplies
// what those groups accumulated by the erf (advanced by its own Taylor step, see emit_group);
// the unmodulated groups follow it.  One erf (sigma, shift) per piece.
void PlanBuilder::fuse_terms() {
  mgroups.clear();
  // (a short plan: in its short pieces only -- the pieces that tier hands on go to the general kernel)
  fmul_now = fmul_base && piece_fmul_ok && (!shortm || (cur_short && !req.no_short_fmul)) && std::isfinite(ax.at(s0)) && std::isfinite(ax.at(s1 - 1));
  multi_ok = !(cur_short ? env.no_short_multi : env.no_lean_multi);
  for (int32_t k : order) {
    if (P->tm_amp_im[k] != 0.0) H.channel_complex[ch] = 1;
    double esg = 0, esh = 0;
    const bool fuse_now = can_fuse && piece_fuse_ok;
    const int32_t fe = fuse_now ? erf_factor_of(k, esg, esh) : -1;
    int fkind = 0;
    const int32_t ff = fuse_now && fe < 0 ? fmul_factor_of(k, fkind) : -1;
    if (fe >= 0 && fuse_term(mgroups, k, tshift, s0, s1, fe)) {
      mod_on = true; mod_sigma = esg; mod_shift = esh; mod_kind = 1;
      ++H.n_fused;
    } else if (ff >= 0 && fslot == 0 && fuse_term(mgroups, k, tshift, s0, s1, ff)) {
      mod_on = true; mod_kind = fkind;
      if (mod_f < 0) mod_f = ff;
      ++H.n_fused;
    } else if (ff >= 0 && fslot >= 1 && fslot <= (int)xmods.size() && fuse_term(xmods[(size_t)fslot - 1].g, k, tshift, s0, s1, ff)) {
      ++H.n_fused;
    } else if (ff >= 0 && fslot == (int)xmods.size() + 1 && [&] {
                 XMod x{fkind, ff, {}};
                 if (!fuse_term(x.g, k, tshift, s0, s1, ff)) return false;
                 xmods.push_back(std::move(x));
                 return true;
               }()) {
      ++H.n_fused;
    } else if (fuse_now && fuse_term(groups, k, tshift, s0, s1)) ++H.n_fused;
    else generic.push_back(k);
  }
}

// step 4: the modulated groups, their closing multiplier(s) and the rest, in the order they are emitted
void PlanBuilder::arrange_modulated() {
  if (mod_on && mod_kind >= 2 && !xmods.empty()) arrange_envelopes();
  else if (mod_on && mod_kind >= 2) arrange_multiplier();
  else if (mod_on) arrange_erf_edge();
}

// several envelopes: each over ONE plain group (degree 0, no envelope of its own), emitted as own-term ops
void PlanBuilder::arrange_envelopes() {
  auto simple = [](const std::vector<FceGroup>& g) {
    return g.size() == 1 && g[0].deg == 0 && !g[0].has_env && !g[0].has_exp && !g[0].chirp && !g[0].corr;
  };
  multi_bad = !simple(mgroups);
  for (const XMod& x : xmods) multi_bad = multi_bad || !simple(x.g);
  std::vector<FceGroup> all;
  if (!multi_bad) {
    FceGroup E;
    E.fmul = mod_kind; E.fmul_f = mod_f; E.fmul_own = true;
    all.push_back(mgroups[0]); all.push_back(E);
    for (const XMod& x : xmods) {
      FceGroup Ex;
      Ex.fmul = x.kind; Ex.fmul_f = x.f; Ex.fmul_own = true;
      all.push_back(x.g[0]); all.push_back(Ex);
    }
    all.insert(all.end(), groups.begin(), groups.end());
    groups.swap(all);
  }
}

// out = F S1 + S0: the groups of the modulated terms, the closing multiplier, then the rest
void PlanBuilder::arrange_multiplier() {
  FceGroup E;
  E.fmul = mod_kind; E.fmul_f = mod_f;
  mgroups.push_back(E);
  mgroups.insert(mgroups.end(), groups.begin(), groups.end());
  groups.swap(mgroups);
}

// out = S0 + erf S1.  Where every group of S1 has a twin in S0 with the same coefficients
// times ONE ratio rho (0.5 cos + 0.5 erf cos), the twins go: out = (rho + erf) S1 + rest.
void PlanBuilder::arrange_erf_edge() {
  FceGroup E;
  E.erfmul = true; E.sigma = mod_sigma; E.sg = mod_shift; E.m0 = 0.0; E.m1 = 1.0;
  std::vector<int> twin(mgroups.size(), -1);
  bool all = !groups.empty();
  long double rho = 0;
  for (size_t i = 0; i < mgroups.size() && all; ++i) {
    const FceGroup& m = mgroups[i];
    int big = -1;                       // the largest coefficient of the modulated group
    long double bigv = 0;
    for (int j = 0; j < 8; ++j) {
      const long double v = fabsl(j < 4 ? m.A[j] : m.B[j - 4]);
      if (v > bigv) { bigv = v; big = j; }
    }
    if (big < 0) { all = false; break; }
    for (size_t j = 0; j < groups.size() && twin[i] < 0; ++j) {
      const FceGroup& g = groups[j];
      if (std::find(twin.begin(), twin.end(), (int)j) != twin.end()) continue;
      if (g.W != m.W || g.imag != m.imag || g.has_env != m.has_env || g.has_exp != m.has_exp || g.sigma != m.sigma || g.sg != m.sg ||
          g.sref != m.sref || g.psi_ref != m.psi_ref || g.has_lin != m.has_lin || g.slin != m.slin ||
          g.deg != m.deg || g.corr != m.corr || g.wm != m.wm || g.sm != m.sm)
        continue;
      const long double r = (big < 4 ? g.A[big] : g.B[big - 4]) / (big < 4 ? m.A[big] : m.B[big - 4]);
      bool same = true;
      for (int q = 0; q < 8 && same; ++q) {
        const long double gv = q < 4 ? g.A[q] : g.B[q - 4], mv = q < 4 ? m.A[q] : m.B[q - 4];
        same = fabsl(gv - r * mv) <= 1e-14L * fabsl(r) * bigv;
      }
      if (same && (i == 0 || fabsl(r - rho) <= 1e-14L * fabsl(rho))) {
        if (i == 0) rho = r;
        twin[i] = (int)j;
      }
    }
    all = twin[i] >= 0;
  }
  if (all && std::isfinite((double)rho)) {
    std::vector<bool> gone(groups.size(), false);
    for (int j : twin) gone[(size_t)j] = true;
    std::vector<FceGroup> rest;
    for (size_t j = 0; j < groups.size(); ++j)
      if (!gone[j]) rest.push_back(groups[j]);
    groups.swap(rest);
    E.m0 = (double)rho;
  }
  mgroups.push_back(E);
  mgroups.insert(mgroups.end(), groups.begin(), groups.end());
  groups.swap(mgroups);
}

// step 5: When every carrier of the piece sits under the SAME Gaussian (a frequency-multiplexed
// pulse), the envelope is factored out: the ops run without envelope and one closing
// pseudo-op multiplies the accumulators by it -- 2 instead of 5 FMAs per sample and tone.
// (From four carriers on: the extra op costs a pair of pieces what it saves them.)
// (short pieces too: a tone costs a phasor seed and 7 instructions per sample there instead of the seeds of its own
//  Gaussian and 13; not for the FIR chain's sampler plan, whose fir_short does not know the closing op)
void PlanBuilder::factor_shared_gaussian() {
  if (groups.size() >= 4 && !mod_on && (!cur_short || (!req.no_short_fmul && !env.no_short_envmul))) {
    bool shared = true, e32 = true;
    for (const FceGroup& g : groups) {
      shared = shared && g.has_env && !g.has_exp && g.sigma == groups[0].sigma && g.sg == groups[0].sg;
      e32 = e32 && g.env32;
    }
    if (shared) {
      FceGroup E;
      E.envmul = true; E.has_env = true; E.sigma = groups[0].sigma; E.sg = groups[0].sg; E.env32 = e32;
      for (FceGroup& g : groups) g.has_env = false;
      groups.push_back(E);
    }
  }
}

// step 6: Runs of >= 4 bare carriers (the tones of a multiplexed pulse once their envelope is factored out, CW
// tones): marked for the lean kernel's compact tone loop -- per tone and tile two state reads, the products
// with the amplitude, the phasor advance; no per-op dispatch (wfk_kernels.hip: fce_bank)
void PlanBuilder::mark_tone_banks() {
  if (!cur_short && !H.tlist && at.ns_override == 0 && !env.no_bank) {
    auto bare = [](const FceGroup& g) {
      return g.W != 0.0 && !g.chirp && g.deg == 0 && !g.has_env && !g.has_exp && !g.envmul && !g.erfmul && !g.fmul && !g.corr;
    };
    for (size_t i = 0; i < groups.size();) {
      size_t j = i;
      while (j < groups.size() && bare(groups[j]) && groups[j].imag == groups[i].imag) ++j;
      if (j - i >= 4) { groups[i].bank = (int)(j - i); piece_has_bank = true; }
      i = j > i ? j : i + 1;
    }
  }
}

// step 7, short tier: the piece as compact records
void PlanBuilder::emit_short() {
  const int32_t first = emit_short_piece(groups, tshift, s0, s1, D.n_blk);
  D.first_len = first;
  D.flags |= WFK_PF_SHORT;
  ++n_short_pieces;
  n_short_samples += s1 - s0;
}

// what the groups, as arranged, ask of the lean kernel
void PlanBuilder::survey_groups() {
  piece_lean = generic.empty() && !groups.empty() && groups.size() <= WFK_LEAN_OPS;
  for (const FceGroup& G : groups) {
    piece_has_chirp = piece_has_chirp || G.chirp;
    piece_has_fmul = piece_has_fmul || G.fmul != 0;     // (own multipliers are still separate entries here: fmul set)
    piece_fam = std::max(piece_fam, G.fmul ? 3 : (G.chirp ? 2 : ((G.erfmul || G.envmul) ? 1 : 0)));
  }
  for (size_t gi = 0; gi + 1 < groups.size(); ++gi)
    if (!cur_short && groups[gi + 1].fmul && groups[gi + 1].fmul_own) piece_fam = 4;     // own-term ops: family 4
  if (piece_has_bank) piece_fam = std::max(piece_fam, 1);
  plan_has_bank = plan_has_bank || piece_has_bank;
}

// (lean pieces: a (group, own multiplier) pair is ONE op -- the multiplier's parameters ride in the group's record)
void PlanBuilder::fold_own_multipliers() {
  std::vector<FceGroup> folded;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    if (gi + 1 < groups.size() && groups[gi + 1].fmul && groups[gi + 1].fmul_own) {
      FceGroup g = groups[gi];
      g.own_kind = groups[gi + 1].fmul; g.own_f = groups[gi + 1].fmul_f;
      folded.push_back(g);
      ++gi;
    } else {
      folded.push_back(groups[gi]);
    }
  }
  groups.swap(folded);
}

// room for `need` more doubles in the block being filled: a full block is flushed first (-1: no block could hold them)
int PlanBuilder::room_for(size_t need) {
  if (WFK_BLK_HDR + need + 2 > WFK_LDS_DOUBLES) return -1;
  if (B.n_terms > 0 && B.size() + need > WFK_LDS_DOUBLES) {
    int32_t len = flush_block(B);
    if (D.n_blk == 0) D.first_len = len;
    ++D.n_blk;
  }
  return 0;
}

// step 7, standard geometry: the groups as op records, then (pass 2) whatever is left, factor by factor
int PlanBuilder::emit_standard_piece() {
  survey_groups();
  if (!cur_short) fold_own_multipliers();
  for (FceGroup& G : groups) {
    if (room_for(WFK_FCE_REC + 2 * (NS + 1)) < 0) { err = "LDS parameter buffer too small"; return WFK_EINVAL; }
    if (H.tlist) {
      const double ta = ax.at(s0) - tshift, tb = ax.at(s1 - 1) - tshift;
      G.tl_thmax = std::fabs(G.W) * std::max(std::fabs(ta - G.sref), std::fabs(tb - G.sref)) + 4.0;
    }
    emit_group(B, G);
    ++B.n_terms;
    piece_units = B.state_units;
  }
  for (int32_t k : generic) {
    const int32_t f0 = P->tm_factor_off[k], f1 = P->tm_factor_off[k + 1];
    // conservative size of this term: header + records + one table per COS
    size_t need = WFK_TERM_HDR + (size_t)(f1 - f0) * (WFK_FREC + 2 * (NS + 1));
    if (room_for(need) < 0) {
      err = "a single term with " + std::to_string(f1 - f0) + " factors exceeds the LDS parameter buffer";
      return WFK_EINVAL;
    }
    B.body.push_back((double)WFK_OP_TERM);
    B.body.push_back(P->tm_amp_re[k]);
    B.body.push_back(P->tm_amp_im[k]);
    B.body.push_back((double)(f1 - f0));
    for (int32_t f = f0; f < f1; ++f) emit_factor(B, f, tshift, s0, s1);
    ++B.n_terms;
    ++H.n_generic;
  }
  blk_len = flush_block(B);
  if (D.n_blk == 0) D.first_len = blk_len;
  ++D.n_blk;
  piece_lean = piece_lean && D.n_blk == 1 && blk_len <= lean_par_cap && piece_units <= 63;
  return WFK_OK;
}

// step 8: the piece is accepted -- is it the lean kernel's, and what does it ask of that kernel
void PlanBuilder::classify_lean() {
  if (H.tlist) {
    // time lists: "lean" = the piece consists of fused ops only (any number of blocks): pointwise build
    if (generic.empty() && !groups.empty()) { D.flags |= WFK_PF_LEAN; ++n_lean_pieces; }
    else lean_ok = false;
  } else if (piece_lean && !shortm) {
    H.lean_fam = std::max(H.lean_fam, piece_fam);   // (a short plan has no lean launch: its other pieces all go to the general kernel)
    D.flags |= WFK_PF_LEAN;
    ++n_lean_pieces;
    H.lean_ops = std::max<int32_t>(H.lean_ops, piece_units);
    H.lean_par = std::max<int32_t>(H.lean_par, blk_len);
  } else {
    lean_ok = false;
  }
}

}  // namespace
