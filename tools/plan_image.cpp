// plan_image -- the gate for reshaping the host plan compiler (wfk_compile.cpp).
//
//     plan_image CASE_DIR [--only PREFIX] [--no-interleave] [--time REPS]
//
// A HostPlan is a pure function of the program, the time axis and the switches, so "the compiler
// behaves as before" can mean: every table of every plan is byte-identical.  This program reads a
// directory of case files (tools/plan_image_cases.py writes them), compiles every case and prints
// one line per case: name, return code, a 64-bit hash of the complete HostPlan (for a refused
// compile: of the error text).  Build it against two source trees and diff the outputs
// (tools/plan_image.sh does all of it).  Host C++ only: no device, no Python at run time.
//
// Beyond the listing it checks, and exits non-zero on:
//  * witnesses: a case that names a baseline must hash DIFFERENTLY from it (a switch whose
//    witness equals its baseline is no longer tested by the case list);
//  * retry cases: a block batch marked as one wfk_compile_blocks hands back must return
//    WFK_RETRY_STD (a batch that started to concatenate no longer tests that way out);
//  * interleaving: the whole list runs a second time with a request-carrying compile between
//    every two cases and a second thread compiling the same, and every hash must equal the
//    first pass (a switch that outlives its compile shows here).
//
// -DPLAN_IMAGE_OLD_SWITCHES: the tree under test still takes its request through the
// thread-local setters (wfk_internal_keep_mixed_short and friends) -- for comparing against
// commits from before CompileRequest.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "wfk.h"
#include "wfk_internal.h"

namespace {

enum { KIND_COMPILE = 0, KIND_GEOM = 1, KIND_BLOCKS = 2 };
enum { FLAG_INTERLEAVE = 1, FLAG_TIMING = 2, FLAG_EXPECT_RETRY = 4 };

struct Switches { bool keep_mixed_short = false, no_short_fmul = false; int tlist_ns = 0; };

#ifdef PLAN_IMAGE_OLD_SWITCHES
struct OldSwitches {      // set for the length of one call, as the old callers did by hand
  explicit OldSwitches(const Switches& s) {
    wfk_internal_keep_mixed_short(s.keep_mixed_short); wfk_internal_no_short_fmul(s.no_short_fmul); wfk_internal_tlist_ns(s.tlist_ns);
  }
  ~OldSwitches() { wfk_internal_keep_mixed_short(false); wfk_internal_no_short_fmul(false); wfk_internal_tlist_ns(0); }
};
int compile_one(const wfk_program* P, const wfk_grid* g, const double* t, int64_t n, HostPlan& H, std::string& err, const Switches& s) {
  OldSwitches set(s);
  return wfk_compile(P, g, t, n, H, err);
}
int compile_blocks(const wfk_program* P, const wfk_grid* g, int nthreads, HostPlan& H, std::string& err, const Switches& s) {
  OldSwitches set(s);
  return wfk_compile_blocks(P, g, nthreads, H, err);
}
#else
CompileRequest request_of(const Switches& s) {
  CompileRequest r;
  r.keep_mixed_short = s.keep_mixed_short; r.no_short_fmul = s.no_short_fmul; r.tlist_ns = s.tlist_ns;
  return r;
}
int compile_one(const wfk_program* P, const wfk_grid* g, const double* t, int64_t n, HostPlan& H, std::string& err, const Switches& s) {
  return wfk_compile(P, g, t, n, H, err, request_of(s));
}
int compile_blocks(const wfk_program* P, const wfk_grid* g, int nthreads, HostPlan& H, std::string& err, const Switches& s) {
  return wfk_compile_blocks(P, g, nthreads, H, err, request_of(s));
}
#endif

// ---- case files -----------------------------------------------------------------------------------
struct Case {
  std::string name, baseline;
  int32_t kind = 0, nthreads = 0, lane_stride = 0, ns = 0, flags = 0;
  Switches sw;
  std::vector<std::pair<std::string, std::string>> env;
  bool has_grid = false;
  wfk_grid grid{};
  std::vector<double> tlist;
  wfk_program prog{};
  std::vector<std::vector<unsigned char>> arrays;      // the sixteen arrays of the program, each exactly as long as the writer made it
};

struct Reader {
  FILE* f;
  bool ok = true;
  void raw(void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) ok = false; }
  template <class T> T get() { T v{}; raw(&v, sizeof v); return v; }
  std::string str() { const int32_t n = get<int32_t>(); std::string s((size_t)std::max(n, 0), '\0'); raw(&s[0], s.size()); return s; }
};

bool load_case(const std::string& path, Case& c) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  Reader r{f};
  char magic[8];
  r.raw(magic, 8);
  if (!r.ok || std::memcmp(magic, "WFKIMG01", 8) != 0) { std::fclose(f); return false; }
  c.kind = r.get<int32_t>(); c.nthreads = r.get<int32_t>(); c.lane_stride = r.get<int32_t>(); c.ns = r.get<int32_t>();
  c.sw.keep_mixed_short = r.get<int32_t>() != 0; c.sw.no_short_fmul = r.get<int32_t>() != 0; c.sw.tlist_ns = r.get<int32_t>();
  c.flags = r.get<int32_t>();
  c.baseline = r.str();
  const int32_t n_env = r.get<int32_t>();
  for (int32_t i = 0; i < n_env && r.ok; ++i) { std::string k = r.str(), v = r.str(); c.env.emplace_back(k, v); }
  c.has_grid = r.get<int32_t>() != 0;
  c.grid.t0 = r.get<double>(); c.grid.step = r.get<double>(); c.grid.n = r.get<int64_t>();
  c.grid.has_last = r.get<int32_t>(); c.grid.last = r.get<double>(); c.grid.i0 = r.get<int64_t>();
  const int64_t nt = r.get<int64_t>();
  if (!r.ok || nt < 0) { std::fclose(f); return false; }
  c.tlist.resize((size_t)nt);
  r.raw(c.tlist.data(), (size_t)nt * sizeof(double));
  wfk_program& P = c.prog;
  P.n_channels = r.get<int32_t>(); P.n_members = r.get<int32_t>(); P.n_pieces = r.get<int32_t>();
  P.n_terms = r.get<int32_t>(); P.n_factors = r.get<int32_t>(); P.n_pool = r.get<int64_t>();
  c.arrays.resize(16);
  for (auto& a : c.arrays) {
    const int64_t nb = r.get<int64_t>();
    if (!r.ok || nb < 0) { std::fclose(f); return false; }
    a.assign((size_t)std::max<int64_t>(nb, 1), 0);     // (exactly as long as written, so that a sanitizer sees a walk past the end;
    r.raw(a.data(), (size_t)nb);                       //  never empty: the pointers stay valid)
  }
  std::fclose(f);
  if (!r.ok) return false;
  auto i32 = [&](int k) { return reinterpret_cast<const int32_t*>(c.arrays[k].data()); };
  auto f64 = [&](int k) { return reinterpret_cast<const double*>(c.arrays[k].data()); };
  P.ch_member_off = i32(0); P.ch_offset = f64(1); P.ch_tshift = f64(2); P.ch_clip_lo = f64(3); P.ch_clip_hi = f64(4);
  P.mb_piece_off = i32(5); P.pc_bound = f64(6); P.pc_term_off = i32(7); P.tm_amp_re = f64(8); P.tm_amp_im = f64(9);
  P.tm_factor_off = i32(10); P.fc_type = i32(11); P.fc_power = f64(12); P.fc_shift = f64(13);
  P.fc_arg_off = reinterpret_cast<const int64_t*>(c.arrays[14].data()); P.pool = f64(15);
  return true;
}

// ---- the image ------------------------------------------------------------------------------------
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  }
  template <class T> void scalar(T v) { bytes(&v, sizeof v); }
  template <class T> void vec(const std::vector<T>& v) { scalar<uint64_t>(v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};

void hash_plan(Fnv& F, const HostPlan& H) {
  F.scalar<int32_t>(H.tlist); F.scalar(H.n_channels); F.scalar(H.n); F.scalar(H.t0); F.scalar(H.step); F.scalar(H.last);
  F.scalar(H.has_last); F.scalar(H.i0); F.scalar(H.ns); F.scalar(H.tile); F.scalar(H.tiles_per_chunk); F.scalar(H.chunks_per_ch);
  F.vec(H.channels); F.vec(H.pieces); F.vec(H.params); F.vec(H.pool); F.vec(H.chunk_first);
  F.scalar<uint64_t>(H.member_idx.size());
  for (const auto& m : H.member_idx) F.vec(m);
  F.vec(H.channel_complex);
  F.scalar(H.n_fast); F.scalar(H.n_direct); F.scalar(H.n_fused); F.scalar(H.n_generic); F.scalar(H.n_corr);
  F.scalar<int32_t>(H.lean); F.scalar(H.lean_fam); F.scalar<int32_t>(H.mixed);
  F.scalar(H.lean_tile); F.scalar(H.lean_tiles_per_chunk); F.scalar(H.lean_chunks_per_ch); F.vec(H.lean_chunk_first);
  F.scalar(H.f32_tiles_per_chunk); F.scalar(H.f32_chunks_per_ch); F.vec(H.f32_chunk_first);
  F.scalar(H.lean_par); F.scalar(H.lean_ops);
  F.scalar<int32_t>(H.shortp); F.scalar(H.max_block_len); F.scalar(H.foreign_frac); F.scalar(H.mean_piece_len);
  F.scalar<int32_t>(H.short_gave_up); F.scalar<int32_t>(H.grid_as_tlist); F.scalar<int32_t>(H.short_has_fmul); F.scalar(H.short_fam);
  F.scalar<int32_t>(H.short_corr); F.scalar<int32_t>(H.short_needs_corr); F.scalar<int32_t>(H.pool_real);
  F.vec(H.s_units); F.vec(H.s_slots); F.scalar(H.s_lds_samples); F.scalar(H.s_units_per_chunk);
}

// where the plan ended up, for the summary: which tiers and ladder outcomes the case list reached
std::string plan_class(const HostPlan& H) {
  if (H.tlist) return H.mixed ? "tlist mixed" : "tlist";
  if (H.shortp) return std::string("short fam ") + std::to_string(H.short_fam) + (H.mixed ? " mixed" : "") + (H.short_gave_up ? " (gave up: pointwise)" : "");
  std::string s = H.lean ? "lean fam " + std::to_string(H.lean_fam) : H.mixed ? "mixed fam " + std::to_string(H.lean_fam) : "general";
  if (H.n_corr > 0) s += " corrected";
  if (H.short_gave_up) s += " (short gave up: pointwise)";
  return s;
}

struct Result { int rc = 0; uint64_t hash = 0; std::string cls; double ms = 0; };

// One case, as the library runs it.  A grid plan whose short attempt gave up is compiled again on the grid's own
// sample times with one sample per lane and the SAME request (wfk_api.cpp, plan_create_impl): both images count.
Result run_case(const Case& c) {
  Result R;
  Fnv F;
  HostPlan H;
  std::string err;
  const wfk_grid* g = c.has_grid ? &c.grid : nullptr;
  static const double dummy = 0.0;
  const double* t = c.has_grid ? nullptr : (c.tlist.empty() ? &dummy : c.tlist.data());
  const auto t0 = std::chrono::steady_clock::now();
  if (c.kind == KIND_GEOM) R.rc = wfk_compile_geom(&c.prog, g, c.lane_stride, c.ns, H, err);
  else if (c.kind == KIND_BLOCKS) R.rc = compile_blocks(&c.prog, g, c.nthreads, H, err, c.sw);
  else R.rc = compile_one(&c.prog, g, t, (int64_t)c.tlist.size(), H, err, c.sw);
  R.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (R.rc == WFK_OK) { hash_plan(F, H); R.cls = plan_class(H); }
  else if (R.rc == WFK_RETRY_STD) R.cls = "blocks: retry in one piece";
  else { F.bytes(err.data(), err.size()); R.cls = "refused"; }
  if (c.kind == KIND_COMPILE && g && R.rc == WFK_OK && H.short_gave_up && g->n > 0 && g->n <= ((int64_t)1 << 24)) {
    std::vector<double> times((size_t)g->n);
    wfk_internal_grid_times(g, times.data());
    Switches s2 = c.sw;
    s2.tlist_ns = WFK_NS_TLIST_SMALL;
    HostPlan H2;
    std::string err2;
    const int rc2 = compile_one(&c.prog, nullptr, times.data(), g->n, H2, err2, s2);
    F.scalar(rc2);
    if (rc2 == WFK_OK) hash_plan(F, H2); else F.bytes(err2.data(), err2.size());
    R.cls += " -> grid as tlist";
  }
  R.hash = F.h;
  return R;
}

struct EnvScope {          // the case's environment, for the length of the case; writers exclude the second thread's compiles
  const Case& c;
  std::shared_mutex& mu;
  EnvScope(const Case& c_, std::shared_mutex& mu_) : c(c_), mu(mu_) {
    if (c.env.empty()) return;
    std::unique_lock<std::shared_mutex> lk(mu);
    for (const auto& kv : c.env) setenv(kv.first.c_str(), kv.second.c_str(), 1);
  }
  ~EnvScope() {
    if (c.env.empty()) return;
    std::unique_lock<std::shared_mutex> lk(mu);
    for (const auto& kv : c.env) unsetenv(kv.first.c_str());
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: plan_image CASE_DIR [--only PREFIX] [--no-interleave] [--time REPS]\n"); return 2; }
  const std::string dir = argv[1];
  std::string only;
  bool interleave = true;
  int time_reps = 0;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--only" && i + 1 < argc) only = argv[++i];
    else if (a == "--no-interleave") interleave = false;
    else if (a == "--time" && i + 1 < argc) time_reps = std::atoi(argv[++i]);
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  std::vector<std::string> files;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 5 && n.compare(n.size() - 5, 5, ".case") == 0) files.push_back(n);
    }
    closedir(d);
  }
  std::sort(files.begin(), files.end());
  if (files.empty()) { std::fprintf(stderr, "no case files in %s\n", dir.c_str()); return 2; }
  // names carry a running number in front ("0042_name.case"): the order of the list; PREFIX filters on the name behind it
  auto name_of = [](const std::string& file) {
    const size_t us = file.find('_');
    return file.substr(us == std::string::npos ? 0 : us + 1, file.size() - 5 - (us == std::string::npos ? 0 : us + 1));
  };
  std::shared_mutex env_mu;
  int failures = 0;

  if (time_reps > 0) {
    // the timing loop: every case flagged as a timing workload, `time_reps` fresh compiles each
    for (const std::string& f : files) {
      Case c;
      if (!load_case(dir + "/" + f, c)) { std::fprintf(stderr, "cannot read %s\n", f.c_str()); return 2; }
      if (!(c.flags & FLAG_TIMING)) continue;
      EnvScope env(c, env_mu);
      std::vector<double> ms;
      for (int r = 0; r < time_reps; ++r) ms.push_back(run_case(c).ms);
      std::sort(ms.begin(), ms.end());
      std::printf("time %s min %.3f median %.3f max %.3f ms over %d\n", name_of(f).c_str(), ms.front(), ms[ms.size() / 2], ms.back(), time_reps);
    }
    return 0;
  }

  // ---- first pass: the listing ----
  std::map<std::string, uint64_t> hash_of;
  std::map<std::string, int> classes;
  std::vector<std::pair<std::string, std::string>> witnesses;      // (case, baseline)
  std::string interleave_file;
  int n_cases = 0, n_retry = 0;
  for (const std::string& f : files) {
    const std::string name = name_of(f);
    if (!only.empty() && name.compare(0, only.size(), only) != 0) continue;
    Case c;
    if (!load_case(dir + "/" + f, c)) { std::fprintf(stderr, "cannot read %s\n", f.c_str()); return 2; }
    c.name = name;
    if ((c.flags & FLAG_INTERLEAVE) && interleave_file.empty()) interleave_file = f;
    Result R;
    {
      EnvScope env(c, env_mu);
      R = run_case(c);
    }
    std::printf("%s %d %016llx\n", name.c_str(), R.rc, (unsigned long long)R.hash);
    hash_of[name] = R.hash;
    ++classes[R.cls];
    ++n_cases;
    if (!c.baseline.empty()) witnesses.emplace_back(name, c.baseline);
    if ((c.flags & FLAG_EXPECT_RETRY) && R.rc != WFK_RETRY_STD) {
      std::fprintf(stderr, "FAIL retry case %s: returned %d, not WFK_RETRY_STD -- that way out of wfk_compile_blocks is not tested\n", name.c_str(), R.rc);
      ++failures;
    }
    n_retry += (c.flags & FLAG_EXPECT_RETRY) ? 1 : 0;
  }
  for (const auto& w : witnesses) {
    const auto b = hash_of.find(w.second);
    if (b == hash_of.end()) { if (only.empty()) { std::fprintf(stderr, "FAIL witness %s: baseline %s is not in the list\n", w.first.c_str(), w.second.c_str()); ++failures; } }
    else if (b->second == hash_of[w.first]) { std::fprintf(stderr, "FAIL witness %s: image equals its baseline %s -- the switch is not tested\n", w.first.c_str(), w.second.c_str()); ++failures; }
  }
  std::fprintf(stderr, "%d cases, %zu witnesses, %d retry cases\n", n_cases, witnesses.size(), n_retry);
  for (const auto& kv : classes) std::fprintf(stderr, "  %5d  %s\n", kv.second, kv.first.c_str());

  // ---- second pass: the same list, a request-carrying compile between every two cases, a second thread doing the same ----
  if (interleave && !interleave_file.empty()) {
    Case between;
    if (!load_case(dir + "/" + interleave_file, between)) return 2;
    std::atomic<bool> stop(false);
    std::atomic<long> other_compiles(0);
    std::thread other([&] {
      while (!stop.load()) {
        std::shared_lock<std::shared_mutex> lk(env_mu);       // (the main thread changes the environment only between our compiles)
        (void)run_case(between);
        ++other_compiles;
      }
    });
    int differing = 0;
    for (const std::string& f : files) {
      const std::string name = name_of(f);
      if (!only.empty() && name.compare(0, only.size(), only) != 0) continue;
      Case c;
      if (!load_case(dir + "/" + f, c)) { stop = true; other.join(); return 2; }
      (void)run_case(between);
      EnvScope env(c, env_mu);
      const Result R = run_case(c);
      if (R.hash != hash_of[name]) { std::fprintf(stderr, "FAIL interleaved pass: %s differs from the first pass\n", name.c_str()); ++differing; }
    }
    stop = true;
    other.join();
    std::fprintf(stderr, "interleaved pass: %d of %d differ (%ld compiles on the second thread)\n", differing, n_cases, other_compiles.load());
    failures += differing;
  }
  return failures ? 1 : 0;
}
