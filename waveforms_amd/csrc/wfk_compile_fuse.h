// wfk_compile_fuse.h -- PlanBuilder: fusion of terms into carrier-envelope groups, and the groups' op records.
// Included by wfk_compile.cpp only.
#pragma once

namespace {

// ---- fusion: terms -> carrier-envelope groups ---------------------------------
bool PlanBuilder::fuse_term(std::vector<FceGroup>& groups, int32_t k, double tshift, int64_t s0,
                            int64_t s1, int32_t skip) {   // skip: a factor handled by the caller
  // a complex amplitude a + ib contributes a * (...) to the real part and b * (...) to the
  // imaginary part of the output: two real-coefficient contributions, the second into groups
  // marked `imag` (their op accumulates into the imaginary accumulators)
  const int32_t f0 = P->tm_factor_off[k], f1 = P->tm_factor_off[k + 1];
  int p = 0, ncos = 0;
  // the term's polynomial factor in u = t' - slin: LINEAR powers shift it up, a Gaussian derivative
  // (D_GAUSSIAN) multiplies it by its Hermite polynomial
  long double tp[4] = {1.0L, 0.0L, 0.0L, 0.0L};
  auto poly_times = [&](const long double (&c)[4]) -> bool {   // tp *= c(u), degree <= 3
    long double out[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) out[i + j] += tp[i] * c[j];
    for (int i = 4; i < 7; ++i)
      if (out[i] != 0.0L) return false;
    for (int i = 0; i < 4; ++i) tp[i] = out[i];
    return true;
  };
  bool has_lin = false, has_env = false, env32 = false;
  double slin = 0, sigma = 0, sg = 0;
  double first_cos_shift = 0;
  // c * cos(K u^2 + W u - Psi),  u = t' - o,  t' = t - tshift; o = 0 for every plain carrier (K == 0), a chirp's own
  // shift for a chirp -- and for whatever it has been multiplied with
  struct Car { long double c, W, Psi, K = 0.0L, o = 0.0L; };
  auto rebase = [](Car r, long double o_new) -> Car {     // the same carrier expanded about another origin
    const long double d = o_new - r.o;                    // t' - r.o = (t' - o_new) + d
    return Car{r.c, r.W + 2 * r.K * d, r.Psi - r.K * d * d - r.W * d, r.K, o_new};
  };
  struct ExpV { long double c, a, b; };    // c * exp(a t' + b): EXP factors, COSH / SINH as two of them
  SmallVec<ExpV, 8> evs;
  evs.push_back({1.0L, 0.0L, 0.0L});
  bool has_expf = false;
  struct CosF { double w, sh, thmax; };    // reference COS factors of the term (|w|, shift, largest |phase|)
  SmallVec<CosF, 40> cosf;
  bool has_drag = false;
  const long double PI = 3.141592653589793238462643383279502884L;
  SmallVec<Car, 32> cars;                  // empty: no carrier factor seen yet
  // multiply the running carrier sum by another sum of carriers:
  //   cos a cos b = (cos(a+b) + cos(a-b)) / 2
  auto times = [&](std::initializer_list<Car> f) -> bool {
    if (cars.empty()) { for (const Car& r : f) cars.push_back(r); return true; }
    if (cars.size() * f.size() * 2 > 32) return false;
    SmallVec<Car, 32> nx;
    for (const Car& q0 : cars)
      for (const Car& r0 : f) {
        Car q = q0, r = r0;
        if (q.o != r.o) {                  // (never for plain carriers: both at 0)
          if (q.K != 0.0L) r = rebase(r, q.o);
          else q = rebase(q, r.o);
        }
        nx.push_back({q.c * r.c / 2, q.W + r.W, q.Psi + r.Psi, q.K + r.K, q.o});
        nx.push_back({q.c * r.c / 2, q.W - r.W, q.Psi - r.Psi, q.K - r.K, q.o});
      }
    cars.swap(nx);
    return true;
  };
  for (int32_t f = f0; f < f1; ++f) {
    if (f == skip) continue;
    const double pw = P->fc_power[f], sh = P->fc_shift[f];
    const double* a = P->pool + P->fc_arg_off[f];
    switch (P->fc_type[f]) {
      case WFK_LINEAR: {
        if (!(pw == 1.0 || pw == 2.0 || pw == 3.0)) return false;
        if (has_lin && sh != slin) return false;
        const double ua = (ax.at(s0) - tshift) - sh, ub = (ax.at(s1 - 1) - tshift) - sh;
        const double um = std::max(std::fabs(ua), std::fabs(ub));
        if (!(um > 0.0) || !rate_safe(pw / um, s0, s1)) return false;   // grid jitter vs |u|
        has_lin = true; slin = sh; p += (int)pw;
        long double mono[4] = {0, 0, 0, 0};
        mono[(int)pw] = 1.0L;
        if (!poly_times(mono)) return false;
        break;
      }
      case WFK_D_GAUSSIAN: {
        // (-1/s)^n H_n(u/s) exp(-(u/s)^2), n <= 3: a polynomial times the Gaussian envelope
        // (reference _waveform.pyx:298-300; what gaussian(width, d=n) and second derivatives make)
        const double sgm = a[0];
        const int n = (int)a[1];
        if (pw != 1.0 || has_env || n < 0 || n > 3 || !std::isfinite(sgm) || sgm == 0.0) return false;
        if (has_lin && sh != slin) return false;
        bool ok64;
        gauss_range(sgm, sh, tshift, s0, s1, ok64, env32);
        if (!ok64 || !rate_safe(2.0 * (n + 1) / sgm, s0, s1)) return false;
        has_env = true; sigma = sgm; sg = sh;
        if (n > 0) {
          const long double s2 = (long double)sgm * sgm;
          long double h[4] = {0, 0, 0, 0};
          if (n == 1) { h[1] = -2.0L / s2; }
          else if (n == 2) { h[0] = -2.0L / s2; h[2] = 4.0L / (s2 * s2); }
          else { h[1] = 12.0L / (s2 * s2); h[3] = -8.0L / (s2 * s2 * s2); }
          if (!has_lin) { has_lin = true; slin = sh; }
          p += n;
          if (!poly_times(h)) return false;
        }
        break;
      }
      case WFK_GAUSSIAN: {
        // exp(-(u/s)^2)^p = exp(-(u / (s / sqrt p))^2): a power of a Gaussian is a narrower (p > 1) or wider one
        // (the reference takes np.power of the value: the same number to (u/s)^2 p x 2^-52 <= 2e-13 relative)
        if (!(pw > 0.0) || !std::isfinite(pw) || has_env) return false;
        const double sg_eff = pw == 1.0 ? a[0] : a[0] / std::sqrt(pw);
        if (!std::isfinite(sg_eff) || sg_eff == 0.0) return false;
        bool ok64;
        gauss_range(sg_eff, sh, tshift, s0, s1, ok64, env32);
        if (!ok64 || !rate_safe(0.86 / sg_eff, s0, s1)) return false;
        has_env = true; sigma = sg_eff; sg = sh;
        break;
      }
      case WFK_COS: {
        // cos^2, cos^3: the factor taken two / three times by product-to-sum (no rounding correction then: the
        // reference rounds the phase ONCE and raises the cosine, which the corrected form does not mimic)
        if (!(pw == 1.0 || pw == 2.0 || pw == 3.0) || !std::isfinite(a[0]) || !std::isfinite(sh)) return false;
        if (pw != 1.0) has_drag = true;
        for (int rep = 0; rep < (int)pw; ++rep) {
          if (ncos == 0) first_cos_shift = sh;
          ++ncos;
          if (!times({{1.0L, (long double)a[0], (long double)a[0] * sh}})) return false;
          const double ua = (ax.at(s0) - tshift) - sh, ub = (ax.at(s1 - 1) - tshift) - sh;
          cosf.push_back({std::fabs(a[0]), sh, std::fabs(a[0]) * std::max(std::fabs(ua), std::fabs(ub))});
        }
        break;
      }
      case WFK_EXP: {
        // exp(alpha u)^p = exp(p alpha t' - p alpha shift)
        if (!expfuse || !std::isfinite(a[0]) || !std::isfinite(pw) || !std::isfinite(sh)) return false;
        for (ExpV& e : evs) { e.a += (long double)pw * a[0]; e.b -= (long double)pw * a[0] * sh; }
        has_expf = true;
        break;
      }
      case WFK_COSH: case WFK_SINH: {
        // (e^{w u} +- e^{-w u}) / 2
        if (!expfuse || pw != 1.0 || !std::isfinite(a[0]) || !std::isfinite(sh) || evs.size() > 2) return false;
        const long double sgn = P->fc_type[f] == WFK_COSH ? 1.0L : -1.0L;
        SmallVec<ExpV, 8> nx;
        for (const ExpV& e : evs) {
          nx.push_back({e.c / 2, e.a + a[0], e.b - (long double)a[0] * sh});
          nx.push_back({sgn * e.c / 2, e.a - a[0], e.b + (long double)a[0] * sh});
        }
        evs.swap(nx);
        has_expf = true;
        break;
      }
      case WFK_LINEARCHIRP: {
        // sin(phi0 + 2 pi (a u^2 + f0 u)), a = (f1 - f0) / (2 T), u = t' - shift (reference
        // _waveform.pyx:323-324) = cos(K t'^2 + W t' - Psi): a carrier whose phase is quadratic.  Fused
        // where the piece can run on the lean kernel (its chirp family: the phasor advances by a phasor
        // that itself advances by a constant -- the complex twin of the Gaussian recurrence).
        if (!chirp_ok || pw != 1.0 || !std::isfinite(sh)) return false;
        for (int i = 0; i < 4; ++i)
          if (!std::isfinite(a[i])) return false;
        if (a[2] == 0.0) return false;
        const long double Kq = 2 * PI * ((long double)a[1] - a[0]) / (2 * (long double)a[2]);
        const long double W0 = 2 * PI * (long double)a[0];
        ++ncos;
        ++ncos;      // (never a single COS factor: the group's phase reference is the term's own)
        if (!times({{1.0L, W0, -((long double)a[3] - PI / 2), Kq, (long double)sh}})) return false;
        break;
      }
      case WFK_DRAG: {
        // sin^2(o tau) cos(wt) + Oy sin(wt),  tau = u - t0,  Oy = -b o sin(2 o tau)
        //   = cos(wt)/2 + (-1/4 + b o/2) cos(wt + 2 o tau) + (-1/4 - b o/2) cos(wt - 2 o tau)
        // (reference: _waveform.pyx:343-356): three plain carriers, no libm per sample
        const double t0 = a[0], freq = a[1], width = a[2], delta = a[3], bf = a[4], phase = a[5];
        if (pw != 1.0 || !(width != 0.0) || !std::isfinite(sh)) return false;
        for (int i = 0; i < 6; ++i)
          if (i != 4 && !std::isfinite(a[i])) return false;
        const long double o = PI / width;
        const long double W = 2 * PI * ((long double)freq + delta);
        const long double Psi0 = W * sh + (2 * PI * (long double)delta * t0 + phase);
        const long double Om = 2 * o, Psi1 = Om * ((long double)sh + t0);
        long double bo = 0.0L;
        if (!std::isnan(bf) && bf - delta != 0.0) bo = o / (2 * PI * ((long double)bf - delta));
        ncos += 2;   // reference shift is derived from Psi/W
        has_drag = true;
        if (!times({{0.5L, W, Psi0},
                    {-0.25L + bo / 2, W + Om, Psi0 + Psi1},
                    {-0.25L - bo / 2, W - Om, Psi0 - Psi1}}))
          return false;
        break;
      }
      default:
        return false;
    }
  }
  if (p > 3 || !std::isfinite(P->tm_amp_re[k]) || !std::isfinite(P->tm_amp_im[k])) return false;
  if (cars.empty()) cars.push_back({1.0L, 0.0L, 0.0L});
  const double cs[1] = {first_cos_shift};
  // stage the contributions; commit only if every carrier finds/creates a group
  std::vector<FceGroup>& staged = fuse_staged;       // (scratch kept across terms: no allocation here)
  staged = groups;
  bool any_corr = false;
  const double tpa = ax.at(s0) - tshift, tpb = ax.at(s1 - 1) - tshift;   // the piece on the channel's own axis
  for (const Car& q : cars) {
    if (q.K != 0.0L) {
      // a chirp: largest instantaneous frequency over the piece; no rounding correction for it
      const double wmax = (double)std::max(fabsl(q.W + 2 * q.K * (tpa - q.o)), fabsl(q.W + 2 * q.K * (tpb - q.o)));
      if (!std::isfinite(wmax) || !rate_safe_n(wmax, s0, s1)) return false;
      continue;
    }
    if (!rate_safe_n((double)q.W, s0, s1)) {
      if (shortm && (!cur_short || tshift != 0.0 || p > 1 || env_no_short_corr || !corr_enabled)) {
        // (only the lean kernel corrects these: a shifted channel, a polynomial of degree > 1 -- and a piece of a short
        //  plan that is built again for the GENERAL kernel, which has no correction: 3e-9 on such a piece, found by the
        //  far fuzz)
        H.short_needs_corr = true;
        return false;
      }
      if (!corr_safe((double)q.W, s0, s1)) { if (shortm) H.short_needs_corr = true; return false; }
      any_corr = true;
    }
  }
  // the term's weight and the reference factor whose rounding it mimics (see corr_safe)
  double wm = 0, sm = 0, weight = 0;
  if (any_corr) {
    if (has_drag || cosf.empty()) return false;      // (the DRAG primitive rounds its phase differently)
    size_t im = 0;
    for (size_t i = 1; i < cosf.size(); ++i)
      if (cosf[i].thmax > cosf[im].thmax) im = i;
    wm = cosf[im].w; sm = cosf[im].sh;
    weight = std::fabs(P->tm_amp_re[k]) + std::fabs(P->tm_amp_im[k]);
    if (has_lin) {
      const double ua = (ax.at(s0) - tshift) - slin, ub = (ax.at(s1 - 1) - tshift) - slin;
      weight *= std::pow(std::max(std::fabs(ua), std::fabs(ub)), p);
    }
    for (size_t i = 0; i < cosf.size(); ++i)         // the other factors' own phase noise must not matter
      if (i != im && 2.3e-16 * cosf[i].thmax * weight > jtol) return false;
  }
  // Exponential factors: under a Gaussian they only move its centre and scale it,
  //   exp(-((t'-sg)/s)^2 + a t' + b) = exp(b + a sg + a^2 s^2 / 4) exp(-((t' - sg - a s^2 / 2)/s)^2);
  // alone they are an envelope of their own, exp(a (t' - ref)) with the reference time in the piece
  // (state g = exp(a (x - ref)), constant ratio exp(a D): the Gaussian recurrence with q = 1).
  struct EnvV { long double amp; bool has_env, env32, has_exp; double sigma, sg; };
  SmallVec<EnvV, 8> envs;
  for (const ExpV& e : evs) {
    EnvV v{e.c, has_env, env32, false, sigma, sg};
    if (has_expf && e.a != 0.0L) {
      if (has_env) {
        const long double lg = e.b + e.a * sg + e.a * e.a * (long double)sigma * sigma / 4;
        const double sg2 = (double)((long double)sg + e.a * (long double)sigma * sigma / 2);
        bool ok64, ok32;
        gauss_range(sigma, sg2, tshift, s0, s1, ok64, ok32);
        if (!(fabsl(lg) <= 600.0L) || !std::isfinite(sg2) || !ok64) return false;
        v.amp *= expl(lg); v.sg = sg2; v.env32 = ok32;
      } else {
        const double ref = 0.5 * (ax.at(s0) + ax.at(s1 - 1)) - tshift;
        const double half = 0.5 * std::fabs(ax.at(s1 - 1) - ax.at(s0)) + (NS + 1) * dstride;   // + a tile of overhang
        const long double lg = e.a * ref + e.b;
        const double ar = (double)e.a;
        if (!std::isfinite(ref) || !(fabsl(lg) <= 600.0L) || !(std::fabs(ar) * half <= 600.0) || !rate_safe(ar, s0, s1))
          return false;
        {
          // an exponential of amplitude >> 1 (coshPulse with a small eps is 23 cos - 22 cos cosh, cancelling to O(1))
          // turns the envelope's share of the grid jitter into that many times the value error: 1.5e-9 of peak 1 ms
          // out (tools/fuzz_soak.py awgfar) -- the envelope's rate is weighed with the term's amplitude there
          double wamp = (std::fabs(P->tm_amp_re[k]) + std::fabs(P->tm_amp_im[k])) * (double)fabsl(e.c * expl(lg));
          if (has_lin) {
            const double ua = (ax.at(s0) - tshift) - slin, ub = (ax.at(s1 - 1) - tshift) - slin;
            wamp *= std::pow(std::max(std::fabs(ua), std::fabs(ub)), p);
          }
          wamp *= std::exp(std::fabs(ar) * 0.5 * std::fabs(ax.at(s1 - 1) - ax.at(s0)));      // its largest value over the piece
          if (std::isfinite(wamp) && wamp > 1.0 && !rate_safe_n(2.0 * ar * wamp, s0, s1)) return false;   // (2: seed and sample both rounded)
        }
        v.amp *= expl(lg); v.has_env = true; v.has_exp = true; v.sigma = ar; v.sg = ref;
        v.env32 = std::fabs(ar) * half <= 80.0;
      }
    } else if (has_expf) {
      if (!(fabsl(e.b) <= 600.0L)) return false;
      v.amp *= expl(e.b);                                  // (rates cancelled: a constant)
    }
    envs.push_back(v);
  }
  for (const EnvV& ev : envs) {
  const bool has_env = ev.has_env, env32 = ev.env32, has_exp = ev.has_exp;   // (shadow the term-level ones)
  const double sigma = ev.sigma, sg = ev.sg;
  for (int part = 0; part < 2; ++part) {
  const long double amp_part = (part == 0 ? (long double)P->tm_amp_re[k] : (long double)P->tm_amp_im[k]) * ev.amp;
  if (amp_part == 0.0L) continue;                 // nothing in this part
  const bool imag = part == 1;
  for (Car q : cars) {
    q.c *= amp_part;
    if (q.W < 0 || (q.W == 0 && q.K < 0)) { q.W = -q.W; q.Psi = -q.Psi; q.K = -q.K; }
    const double W = (double)q.W;
    const bool is_chirp = q.K != 0.0L;
    // (a sum/difference frequency is rounded to double: relative error <= 2^-53, the
    //  same class as the reference's own rounding of w*t)
    FceGroup* G = nullptr;
    double thm = 0;
    for (const CosF& cf : cosf) thm = std::max(thm, cf.thmax);
    const bool heavy = 2.3e-16 * thm * weight > jtol;   // its own phase rounding must be mimicked
    for (FceGroup& g : staged)
      if (g.W == W && (double)g.K == (double)q.K && g.corg == q.o && g.imag == imag && g.has_env == has_env && g.has_exp == has_exp &&
          (!has_env || (g.sigma == sigma && g.sg == sg))) {
        // a corrected group mimics ONE reference factor: a heavy term with another factor founds
        // its own group (same carrier, own op) instead of joining
        if (any_corr && heavy && (g.wm != wm || g.sm != sm)) continue;
        G = &g;
        break;
      }
    if (!G) {
      staged.emplace_back();
      G = &staged.back();
      G->W = W; G->has_env = has_env; G->has_exp = has_exp; G->sigma = sigma; G->sg = sg; G->env32 = env32;
      G->imag = imag;
      G->K = q.K; G->chirp = is_chirp; G->Wl = q.W; G->corg = q.o;
      G->corr = !is_chirp && W != 0.0 && !rate_safe_n(W, s0, s1);
      G->wm = wm; G->sm = sm;
      G->sref = W == 0.0 ? 0.0 : (ncos == 1 ? cs[0] : (double)(q.Psi / q.W));
      G->psi_ref = (long double)W * G->sref;
      if (is_chirp) {      // (the founding term's own phase; reference time = middle of the piece)
        G->sref = 0.0; G->psi_ref = q.Psi;
        G->tref = 0.5 * (tpa + tpb);
      }
      if (!is_chirp && W != 0.0 && ncos != 1) {
        // A sum / difference frequency is rounded to double: (W_exact - W) * (x - s_ref) must stay
        // small, so a corrected carrier takes its reference time INSIDE the piece (with s_ref =
        // Psi / W next to t = 0 the rounding of W is multiplied by |x|: 5e-9 rad at 100 s) -- and so does every
        // other such carrier once that product is more than 2e-12 rad (2e-10 rad per group 1 ms out at 300 MHz:
        // the random AWG-rate scripts moved 1-10 ms from t = 0 had grid AND time-list launches at 1-2.5e-9 of peak,
        // tools/fuzz_soak.py awgfar; plans near t = 0 keep their records bit for bit)
        const double mid = 0.5 * (ax.at(s0) + ax.at(s1 - 1)) - tshift;
        if (std::isfinite(mid) && (G->corr || 1.2e-16 * std::fabs(W) * std::fabs(mid - G->sref) > 2e-12)) {
          G->sref = mid;
          G->psi_ref = q.W * (long double)mid;       // q.W: the exact sum (long double)
        }
      }
    }
    if (has_env && !env32) G->env32 = false;
    long double ca, cb;
    if (W == 0.0 && !is_chirp) { ca = q.Psi == 0.0L ? q.c : q.c * cosl(q.Psi); cb = 0.0L; }
    else {
      const long double delta = G->psi_ref - q.Psi;   // cos(th_ref + delta)
      if (delta == 0.0L) { ca = q.c; cb = 0.0L; }     // (the term that founded the group)
      else {
        long double sd, cd;
        sincosl(delta, &sd, &cd);
        ca = q.c * cd;
        cb = -q.c * sd;
      }
    }
    // multiply by u_term^p with u_term = u_group + d
    long double d = 0.0L;
    if (p > 0) {
      // the group's polynomial variable is centred on the piece (u = t' - slin with slin the
      // mid time of [s0, s1)), not on the first term's own origin: |u| stays <= half the piece
      // span, which keeps the float evaluation of A(u), B(u) free of the cancellation a far
      // origin brings (poly() terms have theirs at t = 0)
      if (!G->has_lin) {
        G->has_lin = true;
        G->slin = 0.5 * (ax.at(s0) + ax.at(s1 - 1)) - tshift;
        if (!std::isfinite(G->slin)) G->slin = slin;
      }
      d = (long double)G->slin - slin;
    }
    static const int binom[4][4] = {{1, 0, 0, 0}, {1, 1, 0, 0}, {1, 2, 1, 0}, {1, 3, 3, 1}};
    const long double dpow[4] = {1.0L, d, d * d, d * d * d};
    for (int m = 0; m <= p; ++m) {           // every monomial tp[m] (u_group + d)^m of the term's polynomial
      if (tp[m] == 0.0L) continue;
      for (int i = 0; i <= m; ++i) {
        long double f = tp[m] * binom[m][i] * dpow[m - i];
        G->A[i] += ca * f;
        G->B[i] += cb * f;
      }
    }
    if (p > G->deg) G->deg = p;
    ++G->nterms;
  }
  }
  }
  groups.swap(staged);
  return true;
}

// (f_j, f_{j+1} - f_j) pairs of an INTERP factor's table in the pool, in 16-byte entries; one copy per distinct
// table of the plan (a gate set reuses a few pulse shapes many times), found again by content
int64_t PlanBuilder::fmul_table(int32_t f) {
  const double* fa = P->pool + P->fc_arg_off[f];
  const int64_t m = P->fc_arg_off[f + 1] - P->fc_arg_off[f] - 2;
  const double* fp = fa + 2;
  uint64_t h = 1469598103934665603ull ^ (uint64_t)m;
  for (int64_t j = 0; j < m; ++j) {
    uint64_t b;
    std::memcpy(&b, &fp[j], 8);
    h = (h ^ b) * 1099511628211ull;
  }
  auto range = fmul_tables.equal_range(h);
  for (auto it = range.first; it != range.second; ++it) {
    const size_t at = (size_t)it->second * 2;
    if (at + 2 * (size_t)(m + 1) > H.pool.size()) continue;          // (rolled back with its piece)
    bool same = true;
    for (int64_t j = 0; j < m && same; ++j) {
      const double dj = j + 1 < m ? fp[j + 1] - fp[j] : 0.0;
      same = std::memcmp(&H.pool[at + 2 * (size_t)j], &fp[j], 8) == 0 && std::memcmp(&H.pool[at + 2 * (size_t)j + 1], &dj, 8) == 0;
    }
    same = same && H.pool[at + 2 * (size_t)m + 1] == 0.0 && std::memcmp(&H.pool[at + 2 * (size_t)m], &fp[m - 1], 8) == 0;
    if (same) return it->second;
  }
  if (H.pool.size() & 1) H.pool.push_back(0.0);
  const int64_t at = (int64_t)(H.pool.size() / 2);
  for (int64_t j = 0; j < m; ++j) {
    H.pool.push_back(fp[j]);
    H.pool.push_back(j + 1 < m ? fp[j + 1] - fp[j] : 0.0);
  }
  H.pool.push_back(fp[m - 1]); H.pool.push_back(0.0);
  fmul_tables.emplace(h, at);
  return at;
}

void PlanBuilder::emit_group(BlockBuilder& B, FceGroup& G) {
  double rec[WFK_FCE_REC] = {0};
  long double A0 = G.A[0], B0 = G.B[0];
  double sref = G.sref;
  int deg = G.deg;
  if (G.chirp) {
    if (B0 != 0.0L && deg == 0) deg = 1;   // (a chirp keeps A and B: its loop has no degree-0 form with a folded shift)
  } else if (G.deg == 0 && G.W != 0.0 && G.corr) {
    // (corrected carriers keep A and B: the folded shift s_ref + phi/W would be ROUNDED to a
    //  double next to |s_ref| -- half an ulp of a time 100 s from the origin is 7e-15 s, 3e-9 rad
    //  under a 60 kHz carrier.  The degree-0 loop has no B term: such an op runs as degree 1.)
    if (B0 != 0.0L) deg = 1;
  } else if (G.deg == 0 && G.W != 0.0 && B0 != 0.0L) {
    // A cos(th) + B sin(th) = R cos(th - phi): fold B into the reference shift -- unless the folded shift, ROUNDED to a
    // double next to |s_ref|, would cost more than 1e-12 of the group's amplitude in phase (W ulp(s_ref) / 2: 8e-11 rad
    // at 1 ms under 120 MHz): the op then runs as degree 1 with A and B, like a corrected carrier.  (A group with
    // B == 0 is left alone: folding a NEGATIVE A as phi = pi moved its reference by pi / W for nothing -- 7e-12 of
    // relative error per ms from t = 0 on every term with a negative amplitude, 3e-9 on coshPulse's 23 cos - 22 cos cosh:
    // the far-from-zero fuzz's last class.)
    long double R = hypotl(A0, B0), phi = atan2l(B0, A0);
    const double folded = (double)((long double)G.sref + phi / (long double)G.W);
    const double ulp = std::nextafter(std::fabs(folded), INFINITY) - std::fabs(folded);
    if (G.bank > 0 || G.own_kind || 0.5 * ulp * std::fabs(G.W) * std::max(1.0, (double)R) <= 1e-12) {   // (tone loops and own-term ops are degree 0 by construction)
      sref = folded;
      A0 = R; B0 = 0.0L;
    } else {
      deg = 1;
    }
  }
  if (G.erfmul) {
    // closing erf multiplier (wfk_kernels.hip: fce_erfmul): step series about the midpoint,
    //   2/sqrt(pi) [h + H2 h^3/24 + H4 h^5/1920 + H6 h^7/322560] as a cubic in w = vm^2
    const long double h = (long double)dstride / G.sigma;
    const long double c = 2.0L * h / sqrtl(3.141592653589793238462643383279502884L);
    const long double a2 = h * h / 24, a4 = h * h * h * h / 1920, a6 = h * h * h * h * h * h / 322560;
    rec[0] = WFK_OP_FCE;
    rec[WFK_FCE_DEG] = (double)WFK_FCE_PACK(1, 0, 0, 3, 0);
    rec[WFK_FCE_A] = G.m0; rec[WFK_FCE_A + 1] = G.m1;
    rec[WFK_FCE_B] = (double)(c * (1 - 2 * a2 + 12 * a4 - 120 * a6));
    rec[WFK_FCE_B + 1] = (double)(c * (4 * a2 - 48 * a4 + 720 * a6));
    rec[WFK_FCE_B + 2] = (double)(c * (16 * a4 - 480 * a6));
    rec[WFK_FCE_B + 3] = (double)(c * 64 * a6);
    rec[WFK_FCE_SIGMA] = G.sigma; rec[WFK_FCE_SG] = G.sg;
    rec[WFK_FCE_H] = (double)h; rec[WFK_FCE_Q] = (double)expl(-2.0L * h * h);
    rec[WFK_FCE_D] = dstride;
    rec[WFK_FCE_DEG] += (double)((B.state_units << 19) | WFK_FCE_HAS_CS | WFK_FCE_HAS_GR);
    B.state_units += 2;
    const size_t at = B.body.size();
    B.body.insert(B.body.end(), rec, rec + WFK_FCE_REC);
    B.fce_ats.push_back(at);
    return;
  }
  if (G.fmul) {
    // stateless closing multiplier (wfk_kernels.hip: fce_tabmul / fce_mollmul): no per-lane state, no seed
    const int32_t f = G.fmul_f;
    const double* fa = P->pool + P->fc_arg_off[f];
    rec[0] = WFK_OP_FCE;
    rec[WFK_FCE_DEG] = (double)WFK_FCE_PACK(G.fmul, 0, 0, 3, 0);
    rec[WFK_FCE_SLIN] = P->fc_shift[f];
    rec[WFK_FCE_D] = dstride;
    if (G.fmul == 2) {
      // np.interp on linspace knots (reference _waveform.pyx:309-311) as value + fraction * difference: the
      // table travels as (f_j, f_{j+1} - f_j) pairs -- ONE 16-byte gather per sample -- with a closing
      // (f_{m-1}, 0) entry for x == stop (and one more, should the index guess round up there)
      const int64_t m = P->fc_arg_off[f + 1] - P->fc_arg_off[f] - 2;
      const double start = fa[0], stop = fa[1];
      rec[WFK_FCE_A] = start; rec[WFK_FCE_A + 1] = (double)(m - 1);
      rec[WFK_FCE_A + 2] = (double)(m - 1) / (stop - start);
      rec[WFK_FCE_B] = dstride * rec[WFK_FCE_A + 2];             // the lane stride in knot units
      rec[WFK_FCE_A + 3] = (double)fmul_table(f);                // in 16-byte entries
    } else {
      rec[WFK_FCE_A] = 1.0 / fa[0];
    }
    const size_t at = B.body.size();
    B.body.insert(B.body.end(), rec, rec + WFK_FCE_REC);
    B.fce_ats.push_back(at);
    return;
  }
  rec[0] = WFK_OP_FCE;
  rec[WFK_FCE_W] = G.W;
  rec[WFK_FCE_SREF] = sref;
  rec[WFK_FCE_SLIN] = G.has_lin ? G.slin : 0.0;
  rec[WFK_FCE_DEG] = (double)(WFK_FCE_PACK(deg, (G.W != 0.0 || G.chirp) ? 1 : 0, G.imag ? 1 : 0,
                                           G.envmul ? 3 : (G.has_env ? 1 : 0), G.env32 ? 1 : 0) |
                              (G.corr ? 128 : 0));
  if (G.corr) ++H.n_corr;
  rec[WFK_FCE_A] = (double)A0;
  rec[WFK_FCE_B] = (double)B0;
  for (int i = 1; i < 4; ++i) { rec[WFK_FCE_A + i] = (double)G.A[i]; rec[WFK_FCE_B + i] = (double)G.B[i]; }
  rec[WFK_FCE_WM] = G.wm;     // (slots 13 / 21 carried redundant copies of the packed word before)
  rec[WFK_FCE_SM] = G.sm;
  if (G.has_exp) {
    // exp(alpha (t - ref)): the seeds are exp(alpha (x - ref)) and the constant ratio exp(alpha D)
    rec[WFK_FCE_DEG] += (double)WFK_FCE_EXPENV;
    rec[WFK_FCE_SIGMA] = G.sigma; rec[WFK_FCE_SG] = G.sg;
    rec[WFK_FCE_H] = G.sigma * dstride; rec[WFK_FCE_Q] = 1.0;
    rec[WFK_FCE_F32OK] = G.env32 ? 1.0 : 0.0;
  } else if (G.has_env) {
    double Hh = dstride / G.sigma;
    rec[WFK_FCE_SIGMA] = G.sigma; rec[WFK_FCE_SG] = G.sg;
    rec[WFK_FCE_H] = Hh; rec[WFK_FCE_Q] = std::exp(-2.0 * Hh * Hh);
    rec[WFK_FCE_F32OK] = G.env32 ? 1.0 : 0.0;
  }
  rec[WFK_FCE_D] = dstride;
  if (G.bank > 0) {
    rec[WFK_FCE_DEG] += (double)WFK_FCE_BANK;
    rec[WFK_FCE_SIGMA] = (double)G.bank;
  }
  if (G.own_kind) {
    // (a plain carrier -- degree 0, B folded into the phase -- or a constant: the slots of the higher coefficients are free)
    const int32_t f = G.own_f;
    const double* fa = P->pool + P->fc_arg_off[f];
    rec[WFK_FCE_DEG] += (double)WFK_FCE_OWNMUL;
    rec[WFK_FCE_SLIN] = P->fc_shift[f];
    if (G.own_kind == 2) {
      const int64_t m = P->fc_arg_off[f + 1] - P->fc_arg_off[f] - 2;
      rec[WFK_FCE_B + 3] = 0.0;
      rec[WFK_FCE_B + 2] = fa[0];
      rec[WFK_FCE_A + 1] = (double)(m - 1);
      rec[WFK_FCE_A + 2] = (double)(m - 1) / (fa[1] - fa[0]);
      rec[WFK_FCE_A + 3] = (double)fmul_table(f);
      rec[WFK_FCE_B + 1] = dstride * rec[WFK_FCE_A + 2];
    } else {
      rec[WFK_FCE_B + 3] = 1.0;
      rec[WFK_FCE_A + 1] = 1.0 / fa[0];
    }
  }
  if (H.tlist) {
    // (pointwise evaluation: no lane stride; the H slot carries 1 / sigma -- the Gaussian's argument is formed
    //  by a multiplication, one rounding off the reference's division: 2 v^2 ulp <= 1.5e-13 relative at |v| = 26)
    if (G.has_env && !G.has_exp) rec[WFK_FCE_H] = 1.0 / G.sigma;
    double lim = 1.6e6;       // (tests: WFK_TLSMALL_LIMIT=0 sends every carrier through the two-term 1/pi reduction)
    if (env.has_tlsmall_limit) lim = env.tlsmall_limit;
    if (G.tl_thmax <= lim) rec[WFK_FCE_DEG] += (double)WFK_FCE_TLSMALL;
  }
  if (G.chirp) {
    // phase about tref:  K tau^2 + W' tau + phi0,  tau = t' - tref;  the per-stride rotation advances by
    // the constant phasor exp(i 2 K D^2)
    const long double PI2 = 6.283185307179586476925286766559005768L;
    const long double tr = G.tref - G.corg;           // the reference time, from the origin of the phase polynomial
    rec[WFK_FCE_W] = (double)(G.Wl + 2 * G.K * tr);
    rec[WFK_FCE_SREF] = G.tref;
    rec[WFK_FCE_WM] = (double)G.K;
    rec[WFK_FCE_SM] = (double)remainderl(G.K * tr * tr + G.Wl * tr - G.psi_ref, PI2);
    const long double d2 = 2 * G.K * (long double)dstride * (long double)dstride;
    rec[WFK_FCE_TAB] = (double)cosl(d2);
    rec[WFK_FCE_F32OK] = (double)sinl(d2);
    rec[WFK_FCE_DEG] += (double)WFK_FCE_CHIRP;
  }
  {
    // per-lane state of the lean kernel: a phasor (c, s) and / or a Gaussian (g, r), 1 KB each (a chirp:
    // the phasor, the phasor it advances by, then the envelope)
    const bool cs = G.W != 0.0 || G.chirp, gr = G.has_env || G.envmul;
    const int need = (cs ? 1 : 0) + (G.chirp ? 1 : 0) + (gr ? 1 : 0);
    if (B.state_units + need <= 63) {
      rec[WFK_FCE_DEG] += (double)((B.state_units << 19) | (cs ? WFK_FCE_HAS_CS : 0) | (gr ? WFK_FCE_HAS_GR : 0));
      B.state_units += need;
    } else {
      B.state_units = 1000;   // (a block this large is never lean)
    }
  }
  size_t at = B.body.size();
  B.body.insert(B.body.end(), rec, rec + WFK_FCE_REC);
  B.fce_ats.push_back(at);
  if (G.W != 0.0 && !G.chirp && !H.tlist) B.table_refs.emplace_back(at + WFK_FCE_TAB, table_for(B, G.W * dstride));
}

// Flat-top edges at AWG rates (short tier): m0 + m1 erf(v_k) sampled HERE, once per distinct edge, as a table of the
// pool in fmul_table's layout (value, step to the next) -- the envelope of an own-term op (short_cmul) that is read at
// whole knots.  A libm erf per sample on the device was two thirds of what a flat-top pulse train cost (150
// instructions behind a call, per sample of an edge), and the closing op a record of its own behind a dependent load.
// Two edges share a table when (sigma, m0, m1, length) agree and their v at the first sample differ by no more than
// the rounding noise of the reference's own t - shift (1.5 ulp of the edge's largest |t|, over sigma) and 2e-11:
// pulses that sit on the sample grid alike.  Every other edge gets a table of its own (16 B per sample).
int64_t PlanBuilder::erf_table(const FceGroup& E, double tshift, int64_t s0, int64_t s1) {
  const int64_t len = s1 - s0;
  auto xat = [&](int64_t k) { double x = ax.at(k); if (tshift != 0.0) x = x - tshift; return x; };
  const double xa = xat(s0), xb = xat(s1 - 1);
  const long double v0 = ((long double)xa - (long double)E.sg) / (long double)E.sigma;
  const double tmax = std::max(std::max(std::fabs(xa), std::fabs(xb)), std::fabs(E.sg));
  const double tol = std::min(1.5 * (std::nextafter(tmax, INFINITY) - tmax) / std::fabs(E.sigma), 2e-11);
  int scanned = 0;
  for (auto it = erf_tabs.rbegin(); it != erf_tabs.rend() && scanned < 64; ++it, ++scanned) {
    if (it->sigma != E.sigma || it->m0 != E.m0 || it->m1 != E.m1 || it->len != len || fabsl(it->v0 - v0) > (long double)tol) continue;
    const size_t a2 = 2 * (size_t)it->at;
    if (a2 + 2 * (size_t)len > H.pool.size()) continue;                   // (rolled back with its piece)
    if (std::memcmp(&H.pool[a2], &it->first, 8) != 0 || std::memcmp(&H.pool[a2 + 2 * (size_t)(len - 1)], &it->last, 8) != 0) continue;
    return it->at;
  }
  if (H.pool.size() & 1) H.pool.push_back(0.0);
  const int64_t at = (int64_t)(H.pool.size() / 2);
  double prev = 0.0;
  for (int64_t k = s0; k < s1; ++k) {
    const double val = (double)((long double)E.m0 + (long double)E.m1 * erfl(((long double)xat(k) - (long double)E.sg) / (long double)E.sigma));
    if (k > s0) H.pool.push_back(val - prev);
    H.pool.push_back(val);
    prev = val;
  }
  H.pool.push_back(0.0);
  erf_tabs.push_back(ErfTab{E.sigma, E.m0, E.m1, v0, len, at, H.pool[2 * (size_t)at], prev});
  return at;
}

}  // namespace
