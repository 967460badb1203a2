// wfk_compile_builder.h -- PlanBuilder: the state of one compile of the host plan compiler, by lifetime.
// Included by wfk_compile.cpp only (one translation unit: the optimiser still inlines the steps into the piece loop).
//
// The compiler's functions name their state directly (NS, jtol, piece_corr_ok, last_direct, ...), so the
// lifetimes are plain structs that PlanBuilder inherits:
//   PlanBuilder's own members   one compile: the inputs, the constants derived once, caches, tallies
//   GeomState                   the geometry in force; set_geom is its only writer
//   PieceState                  one device piece [s0, s1) of one channel, over all attempts at it
//   TryState                    ONE attempt at the piece; begin_attempt starts it from TryState()
//   BlockState                  the parameter block being filled; flush_block ends it
// What an attempt wrote OUTSIDE these -- into the plan -- is what PlanBuilder::restore takes back.
#pragma once

namespace {

struct GeomState {
  bool cur_short = false;       // the piece being built uses the short tier's contiguous-lane geometry
  int NS = 0;                   // samples per lane ...
  double dstride = 0.0;         // ... and the time between a lane's samples
};

// What restore() puts back when an attempt at a piece is given up (see there for what it leaves alone)
struct Snap {
  size_t params = 0, pool = 0;
  int32_t nf = 0, nd = 0, nu = 0, ng = 0, nc = 0;
  std::map<int64_t, int64_t> sampled;
  DevPiece D{};
};

struct PieceState {
  int32_t ch = 0;               // the channel ...
  double tshift = 0.0;          // ... and its shift
  int64_t s0 = 0, s1 = 0;       // the piece's samples
  // the jitter budget of ONE term of this piece: WFK_JITTER_TOL over the number of terms that meet in it (grid_jitter)
  double jtol = WFK_JITTER_TOL;
  bool piece_corr_ok = true;    // cleared for the second attempt at a piece that turned out not to be lean
  bool piece_chirp_ok = true;   // likewise: the fused chirp op exists in the lean kernel only
  bool piece_fmul_ok = true;    // likewise: the stateless closing multipliers
  bool piece_fuse_ok = true;    // time lists: cleared for the second attempt at a piece that kept a generic term
  bool chirp_ok = false;        // chirps may fuse in this attempt (begin_attempt)
  DevPiece D{};
  Snap snap;                    // the plan and D as they were before the first attempt
  // (scratch, kept across pieces: a 2 GS/s channel is thousands of pieces, and their heap traffic was a third of a compile)
  std::vector<int32_t> live, generic, order;
  std::vector<FceGroup> groups, mgroups;
};

// a further envelope of a piece that holds several (see PlanBuilder::fmul_factor_of)
struct XMod { int kind; int32_t f; std::vector<FceGroup> g; };

struct TryState {
  int attempt = 0;
  int32_t corr_before = 0;      // H.n_corr when the attempt began
  // the piece's closing multiplier, found by the fuse pass: the terms under it fuse into `mgroups`
  bool fmul_now = false;        // stateless multipliers are admissible in this attempt
  bool multi_ok = false;        // ... and several of them in one piece
  bool mod_on = false;
  double mod_sigma = 0, mod_shift = 0;
  int mod_kind = 0;             // 1: erf edge, 2: INTERP table, 3: mollifier (the closing multiplier of this piece)
  int32_t mod_f = -1;           // the first term's factor of that kind (later terms must carry an equal one)
  std::vector<XMod> xmods;      // the envelopes after the first one
  int fslot = 0;                // fmul_factor_of: 0 the piece's first envelope, i + 1: xmods[i], xmods.size() + 1: a new one
  bool multi_bad = false;       // several envelopes, and not each over ONE plain group
  bool piece_has_bank = false;
  // what survey_groups and emit_standard_piece find, for attempt_outcome and classify_lean
  bool piece_lean = false, piece_has_chirp = false, piece_has_fmul = false;
  int piece_fam = 0;            // lean kernel family the piece needs: 0 plain ops, 1 closing ops, 2 chirps, 3 stateless multipliers
  int32_t piece_units = 0;      // per-lane state units of the piece's (last) block
  int32_t blk_len = 0;          // length of the piece's last block
};

struct BlockState {
  BlockBuilder B;
  std::vector<double> last_direct;      // record of the last direct factor of the current block
};

// The four ways an attempt at a piece can end (PlanBuilder::attempt_outcome decides, build_piece acts)
enum class Outcome {
  Accept,
  AgainUnfused,         // a time-list piece that kept a generic term: every term factor by factor
  AgainStandard,        // a short piece that the tier cannot take: standard geometry, counted as foreign
  AgainWithoutLeanOps,  // not lean after all, but built with ops that only the lean kernel has
};
enum class Stage { Fused, Arranged, Emitted };      // how far the attempt has come when the question is asked

struct PlanBuilder : GeomState, PieceState, TryState, BlockState {
  // ---- the plan: inputs ----
  const wfk_program* const P;
  const TimeAxis& ax;
  const wfk_grid* const grid;   // (= ax.g)
  HostPlan& H;
  const CompileRequest& req;
  const Attempt& at;
  const CompileEnv& env;
  std::string& err;
  // ---- the plan: constants derived once ----
  const bool shortm;            // the plan is compiled for the short tier
  const int lean_par_cap;
  const bool env_no_short_corr;
  const bool nofast;
  // (short tier: family 6 evaluates corrected carriers of degree <= 1 on channels without a pending shift)
  const bool corr_enabled;
  const bool chirp_base;
  const bool nolean;
  // (time-list plans fuse too: their ops are evaluated pointwise -- one sincos + one exp per group and
  //  sample instead of a libm call per factor; WFK_DISABLE_TLFUSE=1: every factor on device libm, as before)
  const bool can_fuse;
  const bool expfuse;
  const bool erfmod_base;
  // stateless closing multipliers (INTERP tables, mollifiers): ops of the lean kernel's family 3 ONLY, so they
  // exist where every piece flagged lean is certain to run on that kernel (lean or mixed plans in the standard
  // geometry, no corrected carriers: that instantiation has families 0 / 1 only)
  const bool fmul_base;
  // ---- the plan: caches ----
  std::map<int64_t, int64_t> sampled_at;          // SAMPLED tables already copied: program pool offset -> H.pool offset
  std::multimap<uint64_t, int64_t> fmul_tables;   // fmul_table: content hash -> first entry in H.pool (16-byte entries)
  std::vector<ErfTab> erf_tabs;                   // erf_table
  std::vector<FceGroup> fuse_staged;              // fuse_term's scratch
  // ---- the plan: tallies ----
  bool lean_ok;
  bool plan_has_bank = false;   // some piece holds a run of bare carriers (tone loop): longer chunks pay there
  int64_t n_lean_pieces = 0, n_short_pieces = 0, n_foreign_pieces = 0, n_short_samples = 0, n_foreign_samples = 0;

  PlanBuilder(const wfk_program* P_, const TimeAxis& ax_, HostPlan& H_, std::string& err_, const CompileRequest& req_,
              const Attempt& at_, const CompileEnv& env_, bool shortm_)
      : P(P_), ax(ax_), grid(ax_.g), H(H_), req(req_), at(at_), env(env_), err(err_),
        shortm(shortm_),
        lean_par_cap(at.ns_override > 0 ? WFK_CHAIN_PAR : WFK_LEAN_PAR),
        env_no_short_corr(env.no_short_corr || at.no_short_corr),
        nofast(env.disable_fast),
        corr_enabled(at.allow_corr && (!shortm || !env_no_short_corr) && !H.tlist && !env.disable_corr),
        chirp_base(!H.tlist && at.ns_override == 0 && !at.no_chirp && !env.disable_chirp),
        nolean(env.disable_lean),
        can_fuse((!H.tlist || !env.disable_tlfuse) && !nofast && !env.disable_fuse),
        expfuse(!env.disable_expfuse),
        erfmod_base(can_fuse && !H.tlist && at.ns_override == 0 && !env.disable_erfmul),
        fmul_base(erfmod_base && !nolean && !at.no_chirp && !env.disable_fmul && !env.disable_mixed),
        lean_ok(can_fuse) {
    set_geom(shortm);
  }

  // geometry of the piece being built: lanes one sample apart (short tier) or `lane_stride` apart
  void set_geom(bool sh) {
    cur_short = sh;
    NS = sh ? WFK_SH_R : H.ns;
    dstride = grid ? (sh ? 1.0 : (double)at.lane_stride) * grid->step : 0.0;
  }

  // ---- wfk_compile_factor.h: jitter rules and factor records ----
  int table_for(BlockBuilder& B, double dphase);
  void gauss_range(double sigma, double shift, double tshift, int64_t s0, int64_t s1, bool& f64_ok, bool& f32_ok);
  double grid_jitter(int64_t s0, int64_t s1);
  bool rate_safe(double rate, int64_t s0, int64_t s1);
  bool rate_safe_n(double rate, int64_t s0, int64_t s1);
  bool corr_safe(double rate, int64_t s0, int64_t s1);
  void emit_factor(BlockBuilder& B, int32_t f, double tshift, int64_t s0, int64_t s1);
  int32_t flush_block(BlockBuilder& B);
  // ---- wfk_compile_fuse.h: terms -> carrier-envelope groups -> op records ----
  bool fuse_term(std::vector<FceGroup>& groups, int32_t k, double tshift, int64_t s0, int64_t s1, int32_t skip = -1);
  int64_t fmul_table(int32_t f);
  void emit_group(BlockBuilder& B, FceGroup& G);
  int64_t erf_table(const FceGroup& E, double tshift, int64_t s0, int64_t s1);
  // ---- wfk_compile_short.h ----
  int32_t emit_short_piece(const std::vector<FceGroup>& groups, double tshift, int64_t s0, int64_t s1, int32_t& n_rec);
  // ---- wfk_compile_piece.h: the piece, step by step ----
  int build_channel(int32_t c);
  void collect_live(int32_t m0, int32_t m1, std::vector<int32_t>& cur);
  int build_piece();
  void begin_attempt(int attempt_no);
  void restore(const Snap& snap);
  Outcome attempt_outcome(Stage stage);
  void order_terms();
  bool same_mod(int32_t a_, int32_t b_);
  int32_t fmul_factor_of(int32_t k, int& kind_out);
  int32_t erf_factor_of(int32_t k, double& sg_out, double& sh_out);
  void fuse_terms();
  void arrange_modulated();
  void arrange_envelopes();
  void arrange_multiplier();
  void arrange_erf_edge();
  void factor_shared_gaussian();
  void mark_tone_banks();
  void emit_short();
  void survey_groups();
  void fold_own_multipliers();
  int room_for(size_t need);
  int emit_standard_piece();
  void classify_lean();
};

}  // namespace
