// wfk_compile_short.h -- the short tier: a piece's compact op records (PlanBuilder::emit_short_piece), and the
// plan's wave units and lane slots.  Included by wfk_compile.cpp only.
#pragma once

namespace {

// ---- short tier: compact op records (WFK_SH_*), referenced to the first sample of each stretch ----
// The group stands for  E(t') (A(u) cos th + B(u) sin th),  th = W t' - psi_ref,  u = t' - s_lin.
// Everything a lane needs to seed the op `koff` samples after the reference sample x_ref:
//   th/pi = th0p + koff dthp,  u' = koff dt (polynomials re-centred on x_ref),
//   Gaussian v = v0 + koff H  (exp: alpha t'' = v0 + koff H)
int32_t PlanBuilder::emit_short_piece(const std::vector<FceGroup>& groups, double tshift, int64_t s0, int64_t s1,
                                      int32_t& n_rec) {
  const long double PIl = 3.141592653589793238462643383279502884L;
  // ONE carrier (or none) under a table / mollifier envelope -- a pulse as mixing() makes it -- is a single
  // 12-double record: the op adds envelope x carrier itself (word bit 7; bit 8: mollifier) instead of a carrier
  // op followed by the closing multiplier in a record of its own (a dependent load per piece)
  const bool one = groups.size() >= 2 && (groups[1].fmul == 2 || groups[1].fmul == 3) && groups[0].deg == 0 && !groups[0].has_env && !groups[0].has_exp &&
                   !groups[0].erfmul && !groups[0].envmul && !groups[0].chirp && !groups[0].fmul && !env.no_short_cmul;
  // (several envelopes in one piece: the host marked every (group, multiplier) pair -- FceGroup::fmul_own)
  auto own_pair = [&](size_t gi) { return gi + 1 < groups.size() && groups[gi + 1].fmul && (groups[gi + 1].fmul_own || (one && gi == 0)); };
  int32_t rec_len = 0;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    if (gi > 0 && own_pair(gi - 1)) continue;
    rec_len += (groups[gi].deg > 1 || groups[gi].fmul || groups[gi].chirp || groups[gi].corr) ? WFK_SH_OP3 : WFK_SH_OP1;
  }
  // one carrier (or a constant) under a flat-top edge of at most WFK_SH_ERFTAB samples: ONE own-term op over the edge's
  // sampled table (erf_table above), read at whole knots -- position k, step 1 (not for the FIR chain's sampler plan:
  // fir_short evaluates the erf closing op only)
  if (groups.size() == 2 && groups[1].erfmul && s1 - s0 <= WFK_SH_ERFTAB && !req.no_short_fmul && !env.no_short_erftab &&
      groups[0].deg == 0 && !groups[0].has_env && !groups[0].has_exp && !groups[0].erfmul && !groups[0].envmul && !groups[0].chirp &&
      !groups[0].fmul && !groups[0].corr) {
    const FceGroup& G = groups[0];
    double x = ax.at(s0);
    if (tshift != 0.0) x = x - tshift;
    const long double x0 = x;
    const size_t at = H.params.size();
    H.params.resize(at + (size_t)WFK_SH_OP1, 0.0);
    double* o = H.params.data() + at;
    const uint64_t word = (uint64_t)(uint32_t)(((G.W != 0.0 ? 1 : 0) << 2) | ((G.imag ? 1 : 0) << 3) | (3 << 4) | WFK_SH_LAST | 128) |
                          ((uint64_t)(uint32_t)s0 << 32);
    std::memcpy(&o[0], &word, sizeof word);
    if (G.W != 0.0) {
      const long double th0 = (long double)G.W * x0 - G.psi_ref;
      o[1] = (double)remainderl(th0 / PIl, 2.0L);
      const long double dth = (long double)G.W * (long double)grid->step;
      o[2] = (double)(dth / PIl);
      o[3] = (double)cosl(dth);
      o[4] = (double)sinl(dth);
    } else {
      o[3] = 1.0;
    }
    o[5] = 0.0;                      // knot of the reference sample
    o[6] = 1.0;                      // knots per sample
    o[7] = (double)(s1 - s0 - 1);
    o[8] = (double)G.A[0];
    o[9] = (double)erf_table(groups[1], tshift, s0, s1);       // (H.pool may move: o points into H.params)
    o[10] = (double)G.B[0];
    H.short_has_fmul = true;
    H.short_fam = std::max(H.short_fam, 2);
    n_rec = 1;
    return WFK_SH_OP1;
  }
  n_rec = 0;
  for (int64_t r0 = s0; r0 < s1; r0 += WFK_SH_SUB, ++n_rec) {
    double x = ax.at(r0);
    if (tshift != 0.0) x = x - tshift;                 // fl(x - shift), as the reference forms it
    const long double x0 = x;
    const size_t at = H.params.size();
    H.params.resize(at + (size_t)rec_len, 0.0);
    double* o = H.params.data() + at;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const FceGroup& G = groups[gi];
      if (gi > 0 && own_pair(gi - 1)) continue;           // (folded into the record of the group in front of it, below)
      if (G.fmul) {
        // stateless closing multiplier (wfk_short_dev.h: short_tabmul / short_mollmul); the word's degree field
        // (2 | 3) names the kind, so the record is stepped over as a 16-double one.  [5] position at the
        // reference sample and [6] its step per sample, in knot units (table) or in units of r (mollifier);
        // table: [8] m - 1, [9] the table's first entry in the pool (16-byte entries)
        const int32_t f = G.fmul_f;
        const double* fa = P->pool + P->fc_arg_off[f];
        // (chirp multipliers: degree field 2 | 3 as well -- the record is stepped over as a 16-double one -- and bit 10)
        const uint64_t word = (uint64_t)(uint32_t)((G.fmul >= 4 ? (G.fmul - 2) | 1024 : G.fmul) | (3 << 4) | (&G == &groups.back() ? WFK_SH_LAST : 0)) | ((uint64_t)(uint32_t)r0 << 32);
        std::memcpy(&o[0], &word, sizeof word);
        const long double u0 = x0 - (long double)P->fc_shift[f];
        if (G.fmul == 4) {
          // phase / pi = ph0 + scale exp(a_k),  a_k = alpha u0 + (koff + k) alpha dt
          const long double al = fa[1];
          o[5] = (double)(al * u0);
          o[6] = (double)(al * (long double)grid->step);
          o[8] = (double)(2.0L * (long double)fa[0] / al);
          o[9] = (double)remainderl(((long double)fa[2] - 2.0L * PIl * (long double)fa[0] / al) / PIl, 2.0L);
        } else if (G.fmul == 5) {
          // phase / pi = ph0 + scale log(l_k),  l_k = 1 + k u0 + (koff + k) k dt
          const long double kk = fa[1];
          o[5] = (double)(1.0L + kk * u0);
          o[6] = (double)(kk * (long double)grid->step);
          o[8] = (double)(2.0L * (long double)fa[0] / kk);
          o[9] = (double)remainderl((long double)fa[2] / PIl, 2.0L);
        } else if (G.fmul == 2) {
          const int64_t m = P->fc_arg_off[f + 1] - P->fc_arg_off[f] - 2;
          const long double inv = (long double)(m - 1) / ((long double)fa[1] - (long double)fa[0]);
          o[5] = (double)((u0 - (long double)fa[0]) * inv);
          o[6] = (double)((long double)grid->step * inv);
          o[8] = (double)(m - 1);
          o[9] = (double)fmul_table(f);
        } else {
          o[5] = (double)(u0 / (long double)fa[0]);
          o[6] = (double)((long double)grid->step / (long double)fa[0]);
        }
        H.short_has_fmul = true;
        H.short_fam = std::max(H.short_fam, G.fmul >= 4 ? 4 : 2);
        o += WFK_SH_OP3;
        continue;
      }
      if (G.envmul) {
        // closing op of a multi-tone piece: everything accumulated so far *= the Gaussian the tones share
        // (word: closing kind 1; [5] v0, [6] H, [7] q as for an op's own Gaussian)
        const uint64_t word = (uint64_t)(uint32_t)(1 | (3 << 4) | (&G == &groups.back() ? WFK_SH_LAST : 0)) | ((uint64_t)(uint32_t)r0 << 32);
        std::memcpy(&o[0], &word, sizeof word);
        const long double Hh = (long double)grid->step / G.sigma;
        o[5] = (double)((x0 - (long double)G.sg) / G.sigma);
        o[6] = (double)Hh;
        o[7] = (double)expl(-2.0L * Hh * Hh);
        H.short_has_fmul = true;      // (an op fir_short does not evaluate)
        H.short_fam = std::max(H.short_fam, 1);
        o += WFK_SH_OP1;
        continue;
      }
      if (G.erfmul) {
        // closing op of a flat-top edge: everything accumulated so far *= m0 + m1 erf(v), v = v0 + koff H
        const uint64_t word = (uint64_t)(uint32_t)((3 << 4) | (&G == &groups.back() ? WFK_SH_LAST : 0)) | ((uint64_t)(uint32_t)r0 << 32);
        std::memcpy(&o[0], &word, sizeof word);
        o[5] = (double)((x0 - (long double)G.sg) / G.sigma);
        o[6] = (double)((long double)grid->step / G.sigma);
        o[8] = G.m0; o[9] = G.m1;
        H.short_fam = std::max(H.short_fam, 1);
        o += WFK_SH_OP1;
        continue;
      }
      const int env = G.has_exp ? 2 : (G.has_env ? 1 : 0);
      // (a chirp: degree field 2 -- a 16-double record -- and bit 9; its polynomials are of degree <= 1)
      // (a corrected carrier: degree field 2 as well -- a 16-double record --, bit 12, [12..15] w_m, s_m, W, x_ref)
      const uint64_t word = (uint64_t)(uint32_t)(((G.chirp || G.corr) ? 2 : (G.deg & 3)) | (((G.W != 0.0 || G.chirp) ? 1 : 0) << 2) | ((G.imag ? 1 : 0) << 3) | (env << 4) |
                                                 (&G == &groups.back() ? WFK_SH_LAST : 0) | (G.chirp ? 512 : 0) | (G.corr ? 4096 : 0)) |
                            ((uint64_t)(uint32_t)r0 << 32);
      std::memcpy(&o[0], &word, sizeof word);
      if (G.chirp) {
        // phase K t'^2 + W t' - psi_ref at sample k after the reference sample x0:
        //   th0 + k d1 + k^2 d2,  th0 = K x0^2 + W x0 - psi_ref,  d1 = (2 K x0 + W) dt,  d2 = K dt^2
        // [1] th0 / pi (reduced), [2] d1 / pi, [12] d2 / pi, [3] / [4] (cos, sin)(2 d2): the constant the step phasor advances by
        const long double dt = (long double)grid->step;
        const long double xo = x0 - G.corg;           // from the origin of the phase polynomial (the chirp's own shift)
        const long double th0 = G.K * xo * xo + G.Wl * xo - G.psi_ref;
        const long double d1 = (2 * G.K * xo + G.Wl) * dt, d2 = G.K * dt * dt;
        o[1] = (double)remainderl(th0 / PIl, 2.0L);
        o[2] = (double)(d1 / PIl);
        o[12] = (double)(d2 / PIl);
        o[3] = (double)cosl(2 * d2);
        o[4] = (double)sinl(2 * d2);
        H.short_has_fmul = true;      // (an op fir_short does not evaluate: the chain's sampler plan keeps such pieces off the short tier)
        H.short_fam = std::max(H.short_fam, 1);
      } else if (G.W != 0.0) {
        // (a corrected carrier is referenced to a time inside its piece with psi_ref = W_exact s_ref: its phase is
        //  W (x - s_ref) with the ROUNDED W the kernel rotates by -- W x0 - psi_ref would put the rounding of W times
        //  |t| into the seed: 1.3e-8 rad at t = -122 s, the far golden case 31)
        const long double th0 = G.corr ? (long double)G.W * (x0 - (long double)G.sref) : (long double)G.W * x0 - G.psi_ref;
        o[1] = (double)remainderl(th0 / PIl, 2.0L);
        const long double dth = (long double)G.W * (long double)grid->step;
        o[2] = (double)(dth / PIl);
        o[3] = (double)cosl(dth);
        o[4] = (double)sinl(dth);
      } else {
        o[3] = 1.0;
      }
      o[7] = 1.0;
      if (env == 1) {
        const long double Hh = (long double)grid->step / G.sigma;
        o[5] = (double)((x0 - (long double)G.sg) / G.sigma);
        o[6] = (double)Hh;
        o[7] = (double)expl(-2.0L * Hh * Hh);
      } else if (env == 2) {
        o[5] = (double)((long double)G.sigma * (x0 - (long double)G.sg));
        o[6] = (double)((long double)G.sigma * (long double)grid->step);
      }
      // A(u), B(u) about u0 = x_ref - s_lin:  P(u0 + w) = sum_i w^i sum_{m >= i} C(m, i) P_m u0^(m - i)
      const long double u0 = G.has_lin ? x0 - (long double)G.slin : 0.0L;
      static const int binom[4][4] = {{1, 0, 0, 0}, {1, 1, 0, 0}, {1, 2, 1, 0}, {1, 3, 3, 1}};
      long double Ar[4] = {0, 0, 0, 0}, Br[4] = {0, 0, 0, 0};
      const long double upow[4] = {1.0L, u0, u0 * u0, u0 * u0 * u0};
      for (int m = 0; m <= 3; ++m)
        for (int i = 0; i <= m; ++i) {
          const long double f = binom[m][i] * upow[m - i];
          Ar[i] += G.A[m] * f;
          Br[i] += G.B[m] * f;
        }
      o[8] = (double)Ar[0]; o[9] = (double)Ar[1]; o[10] = (double)Br[0]; o[11] = (double)Br[1];
      if (own_pair(gi)) {
        // envelope x carrier in one op (wfk_short_dev.h: short_cmul): the carrier fields as above, [5] / [6] the
        // envelope's position at the reference sample and its step per sample (knot units | units of r),
        // table: [7] m - 1, [9] first entry in the pool (16-byte entries)
        const FceGroup& E = groups[gi + 1];
        const int32_t f = E.fmul_f;
        const double* fa = P->pool + P->fc_arg_off[f];
        const uint64_t w2 = (uint64_t)(uint32_t)(((G.W != 0.0 ? 1 : 0) << 2) | ((G.imag ? 1 : 0) << 3) | (3 << 4) |
                                                 (gi + 2 == groups.size() ? WFK_SH_LAST : 0) | 128 | (E.fmul == 3 ? 256 : 0)) |
                            ((uint64_t)(uint32_t)r0 << 32);
        std::memcpy(&o[0], &w2, sizeof w2);
        const long double ue = x0 - (long double)P->fc_shift[f];
        if (E.fmul == 2) {
          const int64_t m = P->fc_arg_off[f + 1] - P->fc_arg_off[f] - 2;
          const long double inv = (long double)(m - 1) / ((long double)fa[1] - (long double)fa[0]);
          o[5] = (double)((ue - (long double)fa[0]) * inv);
          o[6] = (double)((long double)grid->step * inv);
          o[7] = (double)(m - 1);
          o[9] = (double)fmul_table(f);
        } else {
          o[5] = (double)(ue / (long double)fa[0]);
          o[6] = (double)((long double)grid->step / (long double)fa[0]);
        }
        H.short_has_fmul = true;
        H.short_fam = std::max(H.short_fam, 2);
        o += WFK_SH_OP1;
        continue;
      }
      if (G.corr) {
        o[12] = G.wm; o[13] = G.sm; o[14] = G.W; o[15] = x;
        H.short_corr = true;
        o += WFK_SH_OP3;
      } else if (G.chirp) {
        o += WFK_SH_OP3;
      } else if (G.deg > 1) {
        o[12] = (double)Ar[2]; o[13] = (double)Ar[3]; o[14] = (double)Br[2]; o[15] = (double)Br[3];
        o += WFK_SH_OP3;
      } else {
        o += WFK_SH_OP1;
      }
    }
  }
  return rec_len;
}

}  // namespace

// ---- short tier: wave units and lane slots ------------------------------------
static void short_chunks(HostPlan& H, const CompileEnv& env) {   // workgroup = one wave walking `units_per_chunk` consecutive units
  if (H.s_slots.empty()) H.s_slots.push_back(0);
  H.s_units_per_chunk = env.sh_upc ? env.sh_upc : (int32_t)std::min<int64_t>(6, std::max<int64_t>(1, (int64_t)H.s_units.size() / 8192));
}
static int short_tier_tables(HostPlan& H, const ShortCounts& N, const ChunkRule& R, const CompileEnv& env) {
  // Mostly pieces the short tier cannot take (e.g. carriers that need the lean kernel's grid-rounding
  // correction far from t = 0): the standard tiers serve the whole plan better
  if (N.foreign_samples > N.short_samples || (N.short_pieces == 0 && N.foreign_pieces > 0)) return WFK_RETRY_STD;
  H.shortp = true;
  H.lean = false;
  // corrected carriers live in family 6 = family 0 + the correction: with closing ops, chirps or tables in the same plan
  // the carriers go back to the tiers that have both
  if (H.short_corr && H.short_fam != 0) H.short_needs_corr = true;
  if (H.short_corr && H.short_fam == 0) H.short_fam = 6;
  H.mixed = N.foreign_pieces > 0;       // foreign pieces: a second launch of the general kernel
  H.foreign_frac = N.short_samples > 0 ? (double)N.foreign_samples / (double)(N.short_samples + N.foreign_samples) : 0.0;
  H.tile = 64 * WFK_SH_R;
  for (int32_t c = 0; c < H.n_channels; ++c) {
    ShortUnit U{};
    auto fresh = [&](int64_t j0) {
      U = ShortUnit{};
      U.ch = c; U.j0 = j0; U.slot0 = (int32_t)H.s_slots.size(); U.rec0 = -1;
      U.offset = H.channels[c].offset; U.clip_lo = H.channels[c].clip_lo; U.clip_hi = H.channels[c].clip_hi;
      U.do_clip = H.channels[c].do_clip;
    };
    fresh(0);
    auto close = [&](int64_t next_j0) {
      if (U.n_samples > 0) {
        if (U.n_slots > 0) H.s_lds_samples = std::max(H.s_lds_samples, U.n_samples);
        if (U.rec0 < 0) U.rec0 = 0;
        if (U.n_slots > 0) {
          // LDS staging layout of this unit (wfk_short.hip): plain or padded by one element per 16,
          // whichever spreads the lanes' first elements over more of the 16 bank pairs
          int plain[16] = {0}, padded[16] = {0}, wp = 0, wq = 0;
          for (int32_t k = 0; k < U.n_slots; ++k) {
            const int o = (int)((H.s_slots[(size_t)U.slot0 + k] >> 16) & 0x3ff);
            wp = std::max(wp, ++plain[o & 15]);
            wq = std::max(wq, ++padded[(o + (o >> 4)) & 15]);
          }
          if (wq < wp) U.gaps |= 2;
        }
        H.s_units.push_back(U);
      }
      fresh(next_j0);
    };
    for (int32_t pi = H.channels[c].piece_begin; pi < H.channels[c].piece_end; ++pi) {
      const DevPiece& D = H.pieces[pi];
      if (D.n_blk != 0 && !(D.flags & WFK_PF_SHORT)) {   // the general kernel's piece: no unit covers it
        close(D.stop);
        continue;
      }
      if (D.n_blk == 0) {
        // zero stretch: rides in the current unit's range while it fits, long ones as pure-fill units
        int64_t z0 = D.start, left = D.stop - D.start;
        if (U.n_slots > 0) {
          const int64_t take = std::min<int64_t>(left, WFK_SH_LCAP - U.n_samples);
          U.n_samples += (int32_t)take; U.gaps |= 1;
          z0 += take; left -= take;
          if (left > 0) close(z0);
        }
        while (left >= WFK_SH_LCAP / 2) {
          const int64_t take = std::min<int64_t>(left, WFK_SH_FILL);
          if (U.n_samples > 0) close(z0);
          U.n_samples = (int32_t)take;
          z0 += take; left -= take;
          close(z0);
        }
        if (left > 0) { U.n_samples += (int32_t)left; U.gaps |= 1; }
        continue;
      }
      int32_t rec = 0;
      for (int64_t r0 = D.start; r0 < D.stop; r0 += WFK_SH_SUB, ++rec) {
        const int64_t len = std::min<int64_t>(WFK_SH_SUB, D.stop - r0);
        const int64_t nseg = (len + WFK_SH_R - 1) / WFK_SH_R, base = len / nseg, rem = len % nseg;
        const int64_t rec16 = (D.par_off + (int64_t)rec * D.first_len) / 2;
        int64_t k0 = 0;
        for (int64_t sgi = 0; sgi < nseg; ++sgi) {
          const int64_t sl = base + (sgi < rem ? 1 : 0);
          if (U.n_slots == 64 || U.n_samples + sl > WFK_SH_LCAP ||
              (U.rec0 >= 0 && rec16 - U.rec0 > WFK_SH_DREC_MAX)) close(r0 + k0);
          if (U.rec0 < 0) U.rec0 = rec16;
          H.s_slots.push_back(WFK_SH_SLOT(rec16 - U.rec0, U.n_samples, sl));
          ++U.n_slots;
          U.n_samples += (int32_t)sl;
          k0 += sl;
        }
      }
    }
    close(H.n);
  }
  short_chunks(H, env);
  H.chunks_per_ch = 0;
  H.pool_real = !H.pool.empty();
  if (H.pool.empty()) H.pool.push_back(0.0);
  H.params.resize(H.params.size() + 16, 0.0);   // (the kernel reads one op record past the last real one)
  if (H.mixed) {   // the general kernel's launch over the foreign pieces: the grid tier's geometry
    H.ns = WFK_NS_GRID;
    chunking(H, R, false, H.tile, H.tiles_per_chunk, H.chunks_per_ch, H.chunk_first);
  }
  return WFK_OK;
}
