// wfk_compile_factor.h -- PlanBuilder: phasor tables, the grid-jitter rules, factor records of the generic tier,
// parameter blocks.  Included by wfk_compile.cpp only.
#pragma once

namespace {

// MOLLIFIER d>0 polynomial, highest degree first (reference: pyx:365-368)
std::vector<double> mollifier_poly(int d) {
  std::vector<double> p = {0.0, -2.0};  // p[k] = coeff of x^k
  for (int n = 1; n < d; ++n) {
    std::vector<double> nx(p.size() + 3, 0.0);
    for (size_t k = 1; k < p.size(); ++k) {
      double c = (double)k * p[k];
      nx[k - 1 + 4] += c;
      nx[k - 1 + 2] += -2.0 * c;
      nx[k - 1] += c;
    }
    for (size_t k = 0; k < p.size(); ++k) {
      nx[k + 3] += -4.0 * n * p[k];
      nx[k + 1] += (4.0 * n - 2.0) * p[k];
    }
    p.swap(nx);
  }
  std::reverse(p.begin(), p.end());
  return p;
}

// phasor table (C[k], S[k]) = (cos, sin)(k * dphase), k < NS, shared per block
int PlanBuilder::table_for(BlockBuilder& B, double dphase) {
  auto it = B.table_of_w.find(dphase);
  if (it != B.table_of_w.end()) return it->second;
  int table = (int)(B.tables.size() / (2 * (NS + 1)));
  B.table_of_w[dphase] = table;
  // entry NS advances a carried phasor by one tile.  One long-double sincos, then the
  // rotation recurrence in long double (64-bit mantissa: after NS = 16 steps the error is
  // ~1e-18, below half an ulp of the stored doubles) instead of 2 (NS + 1) libm calls per
  // table -- those were most of the plan-creation time of a 100-pulse channel.
  const long double c1 = cosl((long double)dphase), s1 = sinl((long double)dphase);
  long double c = 1.0L, sn = 0.0L;
  for (int k = 0; k <= NS; ++k) {
    B.tables.push_back((double)c);
    B.tables.push_back((double)sn);
    const long double cn = c * c1 - sn * s1;
    sn = sn * c1 + c * s1;
    c = cn;
  }
  return table;
}

// Gaussian recurrence validity over the samples [s0, s1) (+ NS strides of overhang)
void PlanBuilder::gauss_range(double sigma, double shift, double tshift, int64_t s0, int64_t s1,
                              bool& f64_ok, bool& f32_ok) {
  double ua = (ax.at(s0) - tshift) - shift, ub = (ax.at(s1 - 1) - tshift) - shift;
  double umax = std::max(std::fabs(ua), std::fabs(ub));
  double Hs = dstride / std::fabs(sigma);
  double vext = umax / std::fabs(sigma) + NS * Hs;
  f64_ok = std::isfinite(sigma) && sigma != 0.0 && Hs <= 2.0 && vext <= 26.0;
  f32_ok = f64_ok && vext <= 8.0 && 2.0 * vext * Hs + Hs * Hs <= 80.0;
}

// The uniform-grid fast paths evaluate sample j0 + 64 k at t(j0) + k * 64 * step, the reference
// at NumPy's rounded grid value fl(fl(i*step) + t0).  The two differ by up to ~one ulp of
// |i*step| + |t_i|; a carrier turns that into a phase difference W * dt_jitter, a Gaussian into
// (u/sigma^2) * dt_jitter.  Negligible for the BASELINE configs (1e-12), but a waveform sampled
// 16 ms away from t = 0 with a 300 MHz carrier sees 3e-9.  Where the bound exceeds
// WFK_JITTER_TOL the factor keeps the exact per-sample time (device libm) instead.
// (WFK_JITTER_TOL = 2.5e-10: wfk_compile_types.h)
// ... shared by the TERMS that meet in a piece: a factor may use the bound over the number of terms (a pulse as mixing()
// makes it: 3; overlapping pulses, vstacks: more), so that the terms' errors -- grid jitter, and the phase rounding a
// corrected group does not mimic for the terms that merely joined it -- cannot add up past the contract.  Near t = 0
// the jitter is 1e-6 of any budget; tools/fuzz_soak.py awgfar / far -- the random scripts moved 10 us .. 10 ms from
// t = 0 -- had 2 % of their cases at 1.0-2.5e-9 of peak with the flat bound (240-360 terms per channel, every
// corrected group at 1-3e-10), 1 % with the bound over n / 3, none of 6000 above 7.4e-10 with this one.  The price is
// paid where it applies: `also.far` (3-term pieces 1 ms out) 0.84 -> 0.95 ms -- more terms found groups of their own.
// (PieceState::jtol is that bound for the piece being built)
double PlanBuilder::grid_jitter(int64_t s0, int64_t s1) {
  if (s1 <= s0) return 0.0;
  if (!grid) {
    // time list: every sample is evaluated AT its own time; what separates a fused group from the
    // reference there is the rounding of the reference's own phase fl(w fl(t' - shift)) and of the group's
    // W (t' - s_ref): about an ulp of the phase, i.e. of |t'| times the rate
    const double m = std::max(std::fabs(ax.at(s0)), std::fabs(ax.at(s1 - 1)));
    return 2.4e-16 * m;
  }
  const double m = std::max(std::fabs(ax.at(s0)), std::fabs(ax.at(s1 - 1)));
  return 1.2e-16 * (m + std::fabs((double)(grid->i0 + s1 - 1) * grid->step));
}
bool PlanBuilder::rate_safe(double rate, int64_t s0, int64_t s1) {   // |d value / dt| <= rate
  return std::fabs(rate) * grid_jitter(s0, s1) <= WFK_JITTER_TOL;
}
// (carriers: every term brings a phase of its own, their errors add -- the shared budget; an envelope is evaluated
//  once for the terms under it: the flat bound above)
bool PlanBuilder::rate_safe_n(double rate, int64_t s0, int64_t s1) {
  return std::fabs(rate) * grid_jitter(s0, s1) <= jtol;
}

// A carrier beyond that bound can still run fused.  Two things separate the reference from the
// ideal phasor there: (i) it evaluates AT NumPy's rounded grid time x_k, e_k = x_k - ideal_k
// (about an ulp of |t|), and (ii) its phase is the ROUNDED product fl(w * fl(x_k - shift)),
// rho_k = that minus the exact product (up to half an ulp of the phase: 2e-9 rad at 3e7 rad).
// Both are reproduced per sample, to first order: cos(th + d) = cos th - d sin th with
// d_k = W e_k + rho_k, rho_k recomputed for ONE reference COS factor per group (w_m, s_m): the
// factor of the group's heaviest term with the largest phase.  Terms whose own factor differs
// may join only if their weight times the phase noise stays inside the budget; what is left
// after the correction is d^2 / 2.  (fl(x - s_m) is not exact when the carrier is referenced to
// t = 0, as mixing()'s is: what the subtraction rounds away is recovered with a TwoSum.)
bool PlanBuilder::corr_safe(double rate, int64_t s0, int64_t s1) {
  const double x = std::fabs(rate) * grid_jitter(s0, s1);
  return corr_enabled && piece_corr_ok && std::isfinite(x) && 2.0 * x * x <= 1e-11;   // (d <= ~2 W e)
}

// ---- factor record emission -------------------------------------------------
// The reference evaluates every distinct factor of a piece once (_calc's cache,
// _waveform.pyx:135-147); the generic tier evaluates term by term.  For the expensive case --
// a direct (libm) factor shared by consecutive terms, e.g. the erf edge of a flat-top pulse
// under ten multiplexed carriers -- the values the previous term left in the workgroup's LDS
// value buffer are reused: the repeated record is marked (type + WFK_M_REUSE) when its
// signature equals the last direct factor emitted into the same block.
void PlanBuilder::emit_factor(BlockBuilder& B, int32_t f, double tshift, int64_t s0, int64_t s1) {
  const int type = P->fc_type[f];
  const double pw = P->fc_power[f], shift = P->fc_shift[f];
  const double* a = P->pool + P->fc_arg_off[f];
  const int64_t na = P->fc_arg_off[f + 1] - P->fc_arg_off[f];
  double rec[WFK_FREC] = {(double)type, pw, shift, 0, 0, 0, 0, 0, 0, 0};
  int table = -1;
  bool fast = false;
  if (!H.tlist && !nofast && pw == 1.0 && s1 > s0) {
    // time range of the piece on this channel's shifted axis
    double ua = (ax.at(s0) - tshift) - shift, ub = (ax.at(s1 - 1) - tshift) - shift;
    double umax = std::max(std::fabs(ua), std::fabs(ub));
    if (type == WFK_LINEAR && (umax > 0.0 ? rate_safe(1.0 / umax, s0, s1) : grid_jitter(s0, s1) == 0.0)) {
      // (u itself: the jitter must be negligible against the largest |u| of the piece)
      rec[0] = WFK_M_LIN_REC; rec[3] = dstride; fast = true;
    } else if (type == WFK_COS && std::isfinite(a[0]) && rate_safe_n(a[0], s0, s1)) {
      rec[0] = WFK_M_COS_TAB; rec[3] = a[0]; fast = true;
      table = table_for(B, a[0] * dstride);
    } else if (type == WFK_GAUSSIAN) {
      // exp(-((u+k D)/s)^2): v=u/s, H=D/s.  A lane's seed may sit up to NS strides
      // outside the piece, so the range check includes that overhang.
      bool ok64, ok32;
      gauss_range(a[0], shift, tshift, s0, s1, ok64, ok32);
      if (ok64 && rate_safe(0.86 / a[0], s0, s1)) {   // exp(-676) ~ 1e-294: normal fp64
        double Hh = dstride / a[0];
        rec[0] = WFK_M_GAUSS_REC; rec[3] = a[0]; rec[4] = Hh; rec[5] = std::exp(-2.0 * Hh * Hh);
        // fp32 state is safe only while g and r stay inside float's exponent range
        rec[9] = ok32 ? 1.0 : 0.0;
        fast = true;
      }
    } else if (type == WFK_SINC && std::isfinite(a[0]) && a[0] != 0.0 && rate_safe(3.141592653589793 * a[0], s0, s1) &&
               !env.no_sinc_tab) {
      // sin(pi b u) from the phasor table, the argument pi b u advanced by the very same phase step (so the two
      // stay consistent where the argument passes through zero), one reciprocal per sample instead of libm's
      // sin + a division (reference _waveform.pyx:303-305: np.sinc)
      const double dphase = 3.141592653589793 * a[0] * dstride;
      rec[0] = WFK_M_SINC_TAB; rec[3] = a[0]; rec[4] = dphase; fast = true;
      table = table_for(B, dphase);
    } else if (type == WFK_MOLLIFIER && a[1] == 0.0 && std::isfinite(a[0]) && a[0] > 0.0 && rate_safe(4.0 / a[0], s0, s1) &&
               !env.no_moll_rec) {
      // exp(1 / (x^2 - 1) + 1), x = u / r (reference _waveform.pyx:359-363): the exponent is <= 0 inside the
      // support; Newton reciprocal + inline exponential instead of an IEEE division and libm's exp
      rec[0] = WFK_M_MOLL_REC; rec[3] = a[0]; rec[4] = dstride; fast = true;
    } else if (type == WFK_EXP && std::isfinite(a[0]) && rate_safe(a[0], s0, s1)) {
      double ext = std::fabs(a[0]) * (umax + dstride * NS);
      if (ext <= 600.0) {
        rec[0] = WFK_M_EXP_REC; rec[3] = a[0]; rec[4] = std::exp(a[0] * dstride);
        rec[9] = ext <= 80.0 ? 1.0 : 0.0;
        fast = true;
      }
    }
  }
  bool interp_lin = false;
  if (!fast) {
    switch (type) {
      case WFK_INTERP: {
        rec[3] = a[0]; rec[4] = a[1]; rec[5] = (double)(na - 2); rec[6] = (double)H.pool.size();
        H.pool.insert(H.pool.end(), a + 2, a + na);
        // np.interp's per-sample slope (fp[j+1]-fp[j]) / (xp[j+1]-xp[j]) once per knot, in the
        // same IEEE double operations (this file is built -ffp-contract=off), and 1/step for an
        // O(1) knot index: the device then skips the binary search and the division
        const int64_t m = na - 2;
        const double start = a[0], stop = a[1];
        rec[7] = -1.0;
        if (m >= 2 && stop > start && std::isfinite(start) && std::isfinite(stop)) {
          const double step = (stop - start) / (double)(m - 1);
          auto X = [&](int64_t k) {
            if (k == m - 1) return stop;
            volatile double q = (double)k * step;
            return q + start;
          };
          rec[7] = (double)H.pool.size();
          rec[8] = 1.0 / step;
          rec[9] = step;
          const double* fp = a + 2;
          for (int64_t j = 0; j + 1 < m; ++j) {
            volatile double dy = fp[j + 1] - fp[j], dx = X(j + 1) - X(j);
            H.pool.push_back(dy / dx);
          }
          H.pool.push_back(0.0);
          // grid mode: same arithmetic, but the knot/slope loads (L2 latency) of four samples
          // are in flight together instead of one dependent load pair per sample
          if (!H.tlist && !nofast && pw == 1.0 && m < (int64_t(1) << 31) && !env.no_interp_grid) {
            rec[0] = WFK_M_INTERP_GRID;
            // A finite table is a CONTINUOUS piecewise-linear function: next to a knot the two adjoining
            // segments agree to rounding, so the knot index may come straight from the O(1) guess, without
            // the comparisons against the exact knot abscissae that make up most of the exact lookup (an
            // error of one segment there costs |slope difference| x a few ulp of x).  Admitted while
            // max |slope| x (rounding of x) stays inside the jitter budget; counted as a fast factor: the plan
            // then runs the build of the general kernel without the direct tier.
            double smax = 0.0;
            bool finite = true;
            for (int64_t j = 0; j < m && finite; ++j) finite = std::isfinite(fp[j]);
            for (int64_t j = 0; j + 1 < m && finite; ++j) {
              const double sl = H.pool[(size_t)rec[7] + (size_t)j];
              finite = std::isfinite(sl);
              smax = std::max(smax, std::fabs(sl));
            }
            if (finite && s1 > s0 && rate_safe(4.0 * smax, s0, s1) && !env.no_interp_lin) {
              rec[0] = WFK_M_INTERP_LIN;
              interp_lin = true;
            }
          }
        }
        break;
      }
      case WFK_MOLLIFIER: {
        int d = (int)a[1];
        rec[3] = a[0]; rec[4] = d;
        if (d > 0) {
          std::vector<double> poly = mollifier_poly(d);
          rec[5] = (double)(poly.size() - 1); rec[6] = (double)H.pool.size();
          rec[7] = std::pow(a[0], (double)d);
          H.pool.insert(H.pool.end(), poly.begin(), poly.end());
        }
        break;
      }
      case WFK_D_GAUSSIAN:
        rec[3] = a[0]; rec[4] = a[1];
        rec[5] = std::pow(-1.0, a[1]) / std::pow(a[0], a[1]);
        break;
      case WFK_DRAG_SIN: case WFK_DRAG_SINX:
        rec[3] = (double)H.pool.size();
        H.pool.insert(H.pool.end(), a, a + na);
        break;
      case WFK_SAMPLED: {
        // one copy per table, however many device pieces the member piece was cut into
        auto it = sampled_at.find(P->fc_arg_off[f]);
        if (it == sampled_at.end()) {
          it = sampled_at.emplace(P->fc_arg_off[f], (int64_t)H.pool.size()).first;
          H.pool.insert(H.pool.end(), a + 1, a + na);
          if (na == 1) H.pool.push_back(NAN);    // empty table: never indexed, keep the offset valid
        }
        rec[0] = WFK_M_SAMPLED; rec[3] = (double)it->second; rec[4] = a[0]; rec[5] = (double)(na - 1);
        break;
      }
      default:
        for (int64_t k = 0; k < na && k < 6; ++k) rec[3 + k] = a[k];
    }
    if (interp_lin) ++H.n_fast; else ++H.n_direct;
    std::vector<double> sig(rec, rec + WFK_FREC);
    const bool pooled = type == WFK_INTERP || type == WFK_MOLLIFIER || type == WFK_DRAG_SIN ||
                        type == WFK_DRAG_SINX || type == WFK_SAMPLED;             // records point into the pool: never equal
    if (!pooled && rec[0] < 100.0 && sig == last_direct) rec[0] += WFK_M_REUSE;
    else last_direct = pooled || rec[0] >= 100.0 ? std::vector<double>() : sig;
  } else {
    ++H.n_fast;
  }
  size_t at = B.body.size();
  B.body.insert(B.body.end(), rec, rec + WFK_FREC);
  if (table >= 0) B.table_refs.emplace_back(at + WFK_FREC - 1, table);
}

int32_t PlanBuilder::flush_block(BlockBuilder& B) {
  last_direct.clear();   // the value buffer is only trusted within one block
  // [len, n_terms, body..., pad?, tables...]
  size_t tab_off = WFK_BLK_HDR + B.body.size();
  if (tab_off & 1) ++tab_off;  // 16-byte aligned tables
  for (auto& r : B.table_refs) B.body[r.first] = (double)(tab_off + (size_t)r.second * 2 * (NS + 1));
  for (size_t at : B.fce_ats) {   // the table offset also travels in the packed op word ...
    if (!(((int64_t)B.body[at + WFK_FCE_DEG]) & WFK_FCE_CHIRP))      // (a chirp has no table: the slot holds its constant phasor)
      B.body[at + WFK_FCE_DEG] += 256.0 * B.body[at + WFK_FCE_TAB];
    // ... which the device reads as a 32-bit integer (WFK_FCE_WORD): low half of the slot
    const uint64_t word = (uint32_t)(int64_t)B.body[at + WFK_FCE_DEG];
    std::memcpy(&B.body[at + WFK_FCE_DEG], &word, sizeof word);
  }
  size_t len = tab_off + B.tables.size();
  H.max_block_len = std::max<int32_t>(H.max_block_len, (int32_t)len);
  H.params.push_back((double)len);
  H.params.push_back((double)B.n_terms);
  H.params.insert(H.params.end(), B.body.begin(), B.body.end());
  if ((WFK_BLK_HDR + B.body.size()) & 1) H.params.push_back(0.0);
  H.params.insert(H.params.end(), B.tables.begin(), B.tables.end());
  if (H.params.size() & 1) { H.params.push_back(0.0); }  // keep every block start even
  B = BlockBuilder();
  return (int32_t)len;
}

}  // namespace
