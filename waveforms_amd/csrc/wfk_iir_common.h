// wfk_iir_common.h -- what every IIR form shares (wfk_iir.hip: three-launch scan, iir_onepass, iir_sampled;
// wfk_iir_rows.hip: one cascade per row): the cascade step, the double-double mat-vec that applies the
// transition tables, the quad-precision builder of those tables, and the table set of a chained scan.  (Errors,
// device memory: wfk_host.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "wfk_host.h"

namespace {

// ---- device ---------------------------------------------------------------------------------------------------

// One sample through a cascade of NSEC direct-form-II-transposed sections of order ORD each:
//     y = b0*x + z[0];   z[i] = b[i+1]*x - a[i+1]*y + z[i+1];   z[ord-1] = b[ord]*x - a[ord]*y
// b(s, i), a(s, i): coefficient i of section s, wherever the caller keeps them (a kernel argument, registers);
// section s has its state at z + s * ORD.  Every index is a constant, so the state stays in registers.
// (Accessors and the array reference, not pointers: this form compiles to the code of the kernels' own loops.)
template <int NSEC, int ORD, int N, class CB, class CA>
__device__ __forceinline__ double iir_cascade_step(CB b, CA a, double x, double (&z)[N]) {
#pragma unroll
  for (int s = 0; s < NSEC; ++s) {
    const double y = b(s, 0) * x + z[s * ORD];
#pragma unroll
    for (int i = 0; i + 1 < ORD; ++i) z[s * ORD + i] = b(s, i + 1) * x - a(s, i + 1) * y + z[s * ORD + i + 1];
    z[s * ORD + ORD - 1] = b(s, ORD) * x - a(s, ORD) * y;
    x = y;
  }
  return x;
}

// (sh + sl) += (th + tl) * x in double-double (TwoProd via fma, TwoSum)
__device__ __forceinline__ void dd_acc(double& sh, double& sl, double th, double tl, double x) {
  const double p = th * x;
  const double e = fma(th, x, -p) + tl * x;
  const double s = sh + p;
  const double bb = s - sh;
  sl += ((sh - (s - bb)) + (p - bb)) + e;
  sh = s;
}

// r = v + M c in double-double; M = D x D (hi, lo) pairs.  DD > 0: compile-time dimension, the first DD entries
// of the arrays (extent N >= DD) are used; DD == 0: D_rt at run time.  r may be v; c is neither.
template <int DD, int N>
__device__ __forceinline__ void dd_matvec_add(double (&r)[N], const double (&v)[N], const double* M,
                                              const double (&c)[N], int D_rt = DD) {
  const int D = DD > 0 ? DD : D_rt;
  double nv[N];
#pragma unroll
  for (int i = 0; i < (DD > 0 ? DD : N); ++i) {
    if (i < D) {
      double sh = v[i], sl = 0.0;
#pragma unroll
      for (int j = 0; j < (DD > 0 ? DD : N); ++j)
        if (j < D) dd_acc(sh, sl, M[(i * D + j) * 2], M[(i * D + j) * 2 + 1], c[j]);
      nv[i] = sh + sl;
    }
  }
#pragma unroll
  for (int i = 0; i < (DD > 0 ? DD : N); ++i)
    if (i < D) r[i] = nv[i];
}

// ---- host: transition tables in quad precision ------------------------------------------------------------------
// In direct-form coordinates the k-step transition matrix T is wildly non-normal for clustered poles (entries
// ~1e5 while every eigenvalue is < 1): a T computed by a double-precision recurrence is off by ~1e-9 relative,
// which a scan would amplify into 1e-6 output errors.  Computed in __float128 and stored as (hi, lo) pairs that
// the kernels apply in double-double, T*S is as accurate as the sequential filter itself.
// (Host functions only: no kernel touches a quad.)
typedef __float128 quad;

// one sample through the cascade; b, a: normalised coefficients, sections back to back (orders[s] + 1 each);
// z: the states, back to back
inline void iir_quad_step(int nsec, const int32_t* orders, const double* b, const double* a, quad x, quad* z) {
  for (int s = 0; s < nsec; ++s) {
    const int ord = orders[s];
    const quad y = (quad)b[0] * x + (ord > 0 ? z[0] : (quad)0);
    for (int i = 0; i + 1 < ord; ++i) z[i] = (quad)b[i + 1] * x - (quad)a[i + 1] * y + z[i + 1];
    if (ord > 0) z[ord - 1] = (quad)b[ord] * x - (quad)a[ord] * y;
    x = y;
    b += ord + 1; a += ord + 1; z += ord;
  }
}

// the D x D transition matrix over `steps` samples: column i = homogeneous response to the unit state e_i
inline std::vector<quad> iir_transition(int nsec, const int32_t* orders, const double* b, const double* a, int D,
                                        int steps) {
  std::vector<quad> T((size_t)D * D), z((size_t)D);
  for (int i = 0; i < D; ++i) {
    for (int r = 0; r < D; ++r) z[r] = r == i ? 1 : 0;
    for (int k = 0; k < steps; ++k) iir_quad_step(nsec, orders, b, a, (quad)0, z.data());
    for (int r = 0; r < D; ++r) T[(size_t)r * D + i] = z[r];
  }
  return T;
}

// C = A B (C is neither); every element is summed with k ascending from zero
inline void iir_qmatmul(const std::vector<quad>& A, const std::vector<quad>& B, std::vector<quad>& C, int D) {
  C.resize((size_t)D * D);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      quad acc = 0;
      for (int k = 0; k < D; ++k) acc += A[(size_t)i * D + k] * B[(size_t)k * D + j];
      C[(size_t)i * D + j] = acc;
    }
}

// Tables of a base matrix B as (hi, lo) pairs: pw[k] = B^(2^k), k < 7; lanep[l] = B^(first_power + l), l < 64
// (pw: 7 * D * D * 2 doubles, lanep: 64 * D * D * 2).  Returns B^64, the product B^63 B of the lanep chain.
inline std::vector<quad> iir_power_tables(const std::vector<quad>& B, int D, int first_power, double* pw,
                                          double* lanep) {
  const size_t MM = (size_t)D * D * 2;
  auto put = [&](double* at, const std::vector<quad>& M) {   // quad -> (hi, lo)
    for (size_t e = 0; e < M.size(); ++e) {
      const double hi = (double)M[e];
      at[2 * e] = hi;
      at[2 * e + 1] = (double)(M[e] - (quad)hi);
    }
  };
  std::vector<quad> cur = B, nxt;
  for (int k = 0; k < 7; ++k) {
    put(pw + k * MM, cur);
    iir_qmatmul(cur, cur, nxt, D);
    cur.swap(nxt);
  }
  cur = B;
  if (first_power == 0)
    for (int e = 0; e < D * D; ++e) cur[e] = (e / D == e % D) ? 1 : 0;
  for (int l = 0; l < 64; ++l) {
    put(lanep + l * MM, cur);
    if (first_power + l == 64) break;
    iir_qmatmul(cur, B, nxt, D);
    cur.swap(nxt);
  }
  return cur;
}

// The table set of a chained scan (iir_onepass, iir_sampled) whose lanes own runs of `run` samples: B = T1^(run / block)
// is the run's transition (T1: `block` samples, multiplied on from the right), U = B^64 a chunk's.
struct IirScanTables {
  std::vector<double> pw, lanep;   // B^(2^k), k < 7; B^(l+1), l < 64
  std::vector<double> lanepU;      // U^(l+1), l < 64: the look-back window
  std::vector<double> wdot;        // [run][4], on request: a run's end state from zero state per unit sample at
                                   // position k (the dot-product form of pass 1); zeros unless `plain`
  int run = 0;
  double tmax = 0.0;               // largest entry of B^1 .. B^64 (hi words)
  bool plain = false;              // entries of order 1, nothing cancels: scan and mat-vec in plain double
};

// b, a: as iir_quad_step.  may_plain = false: never plain.  WFK_IIR_DD=1 keeps every set in double-double.
inline IirScanTables iir_scan_tables(int nsec, const int32_t* orders, const double* b, const double* a, int D,
                                     const std::vector<quad>& T1, int block, int run, bool may_plain, bool dot) {
  IirScanTables t;
  t.run = run;
  const size_t MM = (size_t)D * D * 2;
  std::vector<double> pwU(7 * MM, 0.0);
  t.pw.assign(7 * MM, 0.0);
  t.lanep.assign(64 * MM, 0.0);
  t.lanepU.assign(64 * MM, 0.0);
  std::vector<quad> B = T1, nxt;
  for (int k = 1; k < run / block; ++k) { iir_qmatmul(B, T1, nxt, D); B.swap(nxt); }
  const std::vector<quad> U = iir_power_tables(B, D, 1, t.pw.data(), t.lanep.data());
  iir_power_tables(U, D, 1, pwU.data(), t.lanepU.data());
  for (size_t e = 0; e < t.lanep.size(); e += 2) t.tmax = std::max(t.tmax, std::fabs(t.lanep[e]));
  const char* dd = getenv("WFK_IIR_DD");
  t.plain = may_plain && t.tmax < 16.0 && !(dd && dd[0] == '1');
  if (dot) t.wdot.assign((size_t)run * 4, 0.0);
  for (int k = 0; k < run && dot && t.plain; ++k) {
    std::vector<quad> z((size_t)D, (quad)0);
    for (int s = k; s < run; ++s) iir_quad_step(nsec, orders, b, a, s == k ? (quad)1 : (quad)0, z.data());
    for (int r = 0; r < D && r < 4; ++r) t.wdot[(size_t)k * 4 + r] = (double)z[r];
  }
  return t;
}

}  // namespace
