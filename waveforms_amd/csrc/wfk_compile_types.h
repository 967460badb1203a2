// wfk_compile_types.h -- the plain types of the host plan compiler: the time axis, fused groups, parameter blocks,
// the ladder's Attempt, the environment table.  Included by wfk_compile.cpp only.
#pragma once

namespace {

struct TimeAxis {
  const wfk_grid* g;
  const double* t;
  int64_t n;
  double at(int64_t i) const {
    if (t) return t[i];
    if (g->has_last && i == g->n - 1) return g->last;
    volatile double m = (double)(i + g->i0) * g->step;
    return m + g->t0;
  }
  // first i with fl(x[i] - tshift) >= b
  int64_t search_left(double tshift, double b) const {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      int64_t mid = lo + (hi - lo) / 2;
      double x = at(mid);
      if (tshift != 0.0) x = x - tshift;
      if (x < b) lo = mid + 1; else hi = mid;
    }
    return lo;
  }
};

// one fused carrier-envelope group (see WFK_FCE_* in wfk_internal.h)
struct FceGroup {
  double W = 0, sref = 0;
  long double psi_ref = 0;
  bool has_env = false, env32 = false, has_lin = false;
  bool has_exp = false;         // the envelope is exp(sigma * (t - sg)) (sigma = rate, sg = reference time), not a Gaussian
  double sigma = 0, sg = 0, slin = 0;
  long double A[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0};
  int deg = 0, nterms = 0;
  bool imag = false;            // the group adds to the IMAGINARY part of the output
  bool envmul = false;          // pseudo-op: multiply the accumulators by the shared Gaussian envelope
  bool erfmul = false;          // pseudo-op: multiply them by m0 + m1 erf((t - sg) / sigma) (flat-top edge)
  double m0 = 0, m1 = 1;
  int bank = 0;                 // first of a run of `bank` bare carriers (WFK_FCE_BANK)
  int fmul = 0;                 // pseudo-op: multiply them by a stateless function of t - slin: 2 = a finite INTERP table read as a
                                // continuous piecewise-linear function, 3 = mollifier(r) (lean kernel family 3 only)
  int32_t fmul_f = -1;          // ... the program factor it stands for
  int own_kind = 0;             // lean kernel: this plain carrier group carries an envelope of its own (2 table, 3 mollifier) ...
  int32_t own_f = -1;           // ... the program factor of it (WFK_FCE_OWNMUL)
  bool fmul_own = false;        // short tier: the multiplier belongs to the ONE group in front of it (envelope x carrier as one op)
  long double K = 0;            // chirp: the phase is K u^2 + W u - psi_ref, u = t' - corg (W, psi_ref as for a plain carrier)
  long double corg = 0;         // chirp: the origin its phase polynomial is expanded about (the chirp's own shift: about t' = 0
                                // the three terms are 1e10 rad each 3 ms from t = 0 and cancel to 80-bit rounding, 5e-9 rad)
  long double Wl = 0;           // chirp: W before its rounding to double (|W| ~ 2 K |shift|: 2^-53 of it times t' shows in the phase)
  bool chirp = false;
  double tref = 0;              // chirp: reference time inside the piece (the device works in t' - tref)
  bool corr = false;            // carrier needs the per-sample rounding correction (WFK_FCE_PACK bit 7)
  double wm = 0, sm = 0;        // corr: the reference COS factor (w, shift) whose rounded phase fl(w*fl(x-shift)) is mimicked
  double tl_thmax = INFINITY;   // time-list plans: largest |W (t' - s_ref)| over the piece (cheap phase reduction below 1.6e6)
};

struct BlockBuilder {
  std::vector<double> body;     // after the 2-double header
  std::vector<double> tables;   // appended behind the records
  std::vector<std::pair<size_t, int>> table_refs;  // (index of aux slot in body, table id)
  std::vector<size_t> fce_ats;                      // body index of every fused-op record (packed word fix-up)
  std::map<double, int> table_of_w;               // dedupe COS tables by dphase
  int n_terms = 0;                                // ops in this block
  int state_units = 0;                            // lean kernel: per-lane state handed out so far (128 doubles each)
  size_t size() const { return WFK_BLK_HDR + body.size() + tables.size() + 1; }
};

// What one compile of the retry ladder (compile_ladder) runs with, next to the caller's CompileRequest
struct Attempt {
  bool allow_corr;         // far carriers may stay fused with the per-sample rounding correction (false: they go to libm)
  int want_short;          // -1 = decide the short tier from the mean live piece length (grid plans), 0 = never
  bool no_short_corr;      // second attempt at a short plan whose corrected carriers met ops family 6 does not hold
  bool no_chirp;           // second compile of a plan that mixes corrected carriers and chirps
  int lane_stride = 64;    // samples between a lane's consecutive samples ...
  int ns_override = 0;     // ... and samples per lane (0: the tier's own): wfk_compile_geom
};

// ---- environment switches: experiment, validation and tuning knobs, read once per plan ------------------------------
// Three parsing rules, one per switch as it always was: "set at all", "first character is 1", integer in a range.
bool env_set(const char* name) { return std::getenv(name) != nullptr; }
bool env_is1(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }
int env_1_to_64(const char* name) {          // 0: unset or out of range (the switch is ignored then)
  const char* e = std::getenv(name); const int v = e ? std::atoi(e) : 0; return v >= 1 && v <= 64 ? v : 0;
}
struct CompileEnv {
  bool no_sinc_tab = env_set("WFK_NO_SINC_TAB");
  bool no_moll_rec = env_set("WFK_NO_MOLL_REC");
  bool no_interp_grid = env_set("WFK_NO_INTERP_GRID");
  bool no_interp_lin = env_set("WFK_NO_INTERP_LIN");
  bool no_short_cmul = env_set("WFK_NO_SHORT_CMUL");
  bool no_short_chirp = env_set("WFK_NO_SHORT_CHIRP");
  bool no_short_multi = env_set("WFK_NO_SHORT_MULTI");
  bool no_lean_multi = env_set("WFK_NO_LEAN_MULTI");
  bool no_short_envmul = env_set("WFK_NO_SHORT_ENVMUL");
  bool no_bank = env_set("WFK_NO_BANK");
  bool no_short_xchirp = env_set("WFK_NO_SHORT_XCHIRP");
  bool no_short_erftab = env_set("WFK_NO_SHORT_ERFTAB");
  bool no_short_corr = env_set("WFK_NO_SHORT_CORR");
  bool keep_mixed_short = env_set("WFK_KEEP_MIXED_SHORT");   // a short plan that hands many samples on stays a short plan
  bool has_tlsmall_limit = env_set("WFK_TLSMALL_LIMIT");     // time lists: the phase bound of the cheap reduction ...
  double tlsmall_limit = has_tlsmall_limit ? std::atof(std::getenv("WFK_TLSMALL_LIMIT")) : 0.0;   // ... overridden
  bool disable_fast = env_is1("WFK_DISABLE_FAST");           // validation / A-B: every factor with device libm even on a grid
  bool disable_corr = env_is1("WFK_DISABLE_CORR");
  bool disable_chirp = env_is1("WFK_DISABLE_CHIRP");
  bool disable_lean = env_is1("WFK_DISABLE_LEAN");
  bool disable_fuse = env_is1("WFK_DISABLE_FUSE");
  bool disable_tlfuse = env_is1("WFK_DISABLE_TLFUSE");       // time lists: every factor on device libm, as before they fused
  bool disable_expfuse = env_is1("WFK_DISABLE_EXPFUSE");
  bool disable_erfmul = env_is1("WFK_DISABLE_ERFMUL");
  bool disable_fmul = env_is1("WFK_DISABLE_FMUL");
  bool disable_mixed = env_is1("WFK_DISABLE_MIXED");
  int short_mode = std::getenv("WFK_SHORT") ? std::atoi(std::getenv("WFK_SHORT")) : -1;   // 0: never, 1: whatever the piece length
  int64_t short_maxlen = std::getenv("WFK_SHORT_MAXLEN") ? std::atoll(std::getenv("WFK_SHORT_MAXLEN")) : 1536;   // tools/short_crossover.py
  int tpc = env_1_to_64("WFK_TPC");                          // tuning overrides: tiles per chunk, ...
  int tpc_f32 = env_1_to_64("WFK_TPC_F32");                  // ... the float launch's cap on them, ...
  int sh_upc = env_1_to_64("WFK_SH_UPC");                    // ... the short tier's units per chunk
};
struct ChunkRule {             // what a launch's chunking depends on beyond the plan's own tables
  int32_t total_channels;      // channels of the whole job (wfk_compile_blocks: of all blocks, so that their tables concatenate)
  int32_t lean_units_max;      // most state units of a lean piece (phasors + envelopes)
  bool has_bank;               // some piece holds a run of bare carriers (tone loop): longer chunks pay there
  int tpc;                     // WFK_TPC (0: none)
};
struct ShortCounts { int64_t short_pieces, foreign_pieces, short_samples, foreign_samples; };   // what the piece loop took / handed on

// a factor (or a carrier) may take the uniform-grid fast path while the grid jitter costs it no more than this
// (PlanBuilder::grid_jitter, wfk_compile_factor.h)
constexpr double WFK_JITTER_TOL = 2.5e-10;

// one sampled flat-top edge in the pool (PlanBuilder::erf_table)
struct ErfTab { double sigma, m0, m1; long double v0; int64_t len, at; double first, last; };

}  // namespace

// a vector of at most N elements on the stack (the fusion pass runs per term: heap traffic there was a third of a compile)
template <class T, int N>
struct SmallVec {
  alignas(T) unsigned char raw[N * sizeof(T)];     // (no element is constructed until it is pushed)
  int n = 0;
  SmallVec() {}
  SmallVec(const SmallVec& o) : n(o.n) { std::memcpy(raw, o.raw, (size_t)o.n * sizeof(T)); }
  SmallVec& operator=(const SmallVec& o) { n = o.n; std::memcpy(raw, o.raw, (size_t)o.n * sizeof(T)); return *this; }
  T* data() { return reinterpret_cast<T*>(raw); }
  const T* data() const { return reinterpret_cast<const T*>(raw); }
  bool push_back(const T& x) { if (n >= N) return false; data()[n++] = x; return true; }
  size_t size() const { return (size_t)n; }
  bool empty() const { return n == 0; }
  T* begin() { return data(); }
  T* end() { return data() + n; }
  const T* begin() const { return data(); }
  const T* end() const { return data() + n; }
  T& operator[](size_t i) { return data()[i]; }
  const T& operator[](size_t i) const { return data()[i]; }
  void swap(SmallVec& o) { SmallVec t(*this); *this = o; o = t; }
};
