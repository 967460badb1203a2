// wfk_pick.h -- which kernels a sampler plan launches, decided ONCE: wfk_plan_launch walks these picks, the two launch
// functions (wfk_kernels.hip, wfk_short.hip) dispatch on their fields, and wfk_plan_kernel_name prints them.
// Plain C++, no HIP: a stand-alone host program can include it and check the decision without a device.
#pragma once
#include <cstdlib>
#include <string>
#include <type_traits>

#include "wfk.h"
#include "wfk_internal.h"

enum class SamplerTier { Short, Lean, General, Wide };   // wfk_sample_short / _lean / wfk_sample / wfk_sample_wide
enum class ChunkTable { Standard, Lean, F32, ShortUnits };   // HostPlan::chunk_first / lean_chunk_first / f32_chunk_first / s_units

struct SamplerPick {          // one kernel instantiation and the chunk table of the plan its launch walks
  SamplerTier tier;
  ChunkTable table;
  bool slice;                 // general tiers of a grid plan with i0 != 0: wfk_sample_slice / wfk_sample_wide_slice
  bool f32, cplx;             // element type and complexness of the output kind
  bool tlist, generic, direct, corr;
  int ns;                     // samples per lane (short tier: per lane segment, WFK_SH_R)
  int fam;                    // lean: the family; short: the BUILD launched (0 / 1 / 2 / 3 / 4 / 6)
};

struct SamplerPicks { int n = 0; SamplerPick pick[2]; };   // a full launch, in stream order: one or two kernels

// Real float launches of short family 0 run the packed-fp32 build unless WFK_SH_NO_PK=1.  Read at every name call and
// every launch (tests flip it between calls), never at plan creation.
inline bool wfk_short_packed() { const char* e = std::getenv("WFK_SH_NO_PK"); return !(e && e[0] == '1'); }

// One compile-time dispatch over an output kind: f(T{}, std::bool_constant<CPLX>{}).
template <typename F>
auto wfk_with_kind(bool f32, bool cplx, F&& f) {
  if (f32) return cplx ? f(float{}, std::true_type{}) : f(float{}, std::false_type{});
  return cplx ? f(double{}, std::true_type{}) : f(double{}, std::false_type{});
}

// The ordered picks of a full launch of `h` for `out_kind`: short | short + general (the "foreign" pieces) | lean |
// lean + general (mixed grid plan) | pointwise time list + full time list (mixed time list) | general alone.
// WFK_OK, or WFK_EINVAL with the reason in err.
inline int wfk_sampler_picks(const HostPlan& h, int out_kind, bool packed, SamplerPicks& out, std::string& err) {
  out.n = 0;
  if (out_kind < WFK_OUT_F64 || out_kind > WFK_OUT_C64) { err = "bad out_kind"; return WFK_EINVAL; }
  SamplerPick k{};
  k.f32 = out_kind == WFK_OUT_F32 || out_kind == WFK_OUT_C64; k.cplx = out_kind == WFK_OUT_C128 || out_kind == WFK_OUT_C64;
  auto general = [&](bool generic, bool direct) {
    SamplerPick g = k;
    g.tlist = h.tlist; g.generic = generic; g.direct = direct; g.ns = h.ns;
    // float (complex64) outputs of plans with generic terms and of time lists: double arithmetic (wfk_sample_wide, see there)
    g.tier = k.f32 && (h.tlist || generic || direct) ? SamplerTier::Wide : SamplerTier::General;
    g.slice = !h.tlist && h.i0 != 0;   // a time slice of a longer grid: the builds that offset the sample index (a time list carries its times)
    g.table = ChunkTable::Standard;
    return g;
  };
  // the build with the direct tier evaluates generic terms too; time lists are either generic + direct or neither (every
  // term fused: the pointwise-ops-only build; any generic term brings the build with the direct tier)
  const bool direct = h.tlist ? (h.n_direct > 0 || h.n_generic > 0) : h.n_direct > 0;
  const bool generic = direct || h.n_generic > 0;
  if (h.shortp) {
    k.tier = SamplerTier::Short; k.table = ChunkTable::ShortUnits; k.ns = WFK_SH_R;
    const int f = h.short_fam;    // (what the compiler produces: HostPlan::short_fam)
    if (f != 0 && f != 1 && f != 2 && f != 4 && f != 6) { err = "short plan: no build for op family " + std::to_string(f); return WFK_EINVAL; }
    // (real float launches of family 0 run its packed-fp32 build, "family 3")
    k.fam = h.short_fam == 0 && out_kind == WFK_OUT_F32 && packed ? 3 : h.short_fam;
    out.pick[out.n++] = k;
    if (h.mixed) out.pick[out.n++] = general(generic, direct);   // pieces the short tier cannot take: a second launch of the general kernel
    return WFK_OK;
  }
  if (!h.tlist && (h.lean || h.mixed)) {
    // the lean kernel exists for grid plans only; in a mixed plan it takes the lean and the zero pieces first, on its
    // own chunking (one wave per workgroup), then the general kernel the pieces with generic terms
    if (h.lean_fam < 0 || h.lean_fam > 4) { err = "lean plan: no build for family " + std::to_string(h.lean_fam); return WFK_EINVAL; }
    k.tier = SamplerTier::Lean; k.ns = h.ns;
    // the corrected build exists for double only, and for families 0 and 1 (corrected carriers and chirps never share a
    // plan's lean pieces: wfk_compile.cpp)
    k.corr = h.n_corr > 0 && !k.f32;
    k.fam = k.corr ? (h.lean_fam >= 1 ? 1 : 0) : h.lean_fam;
    // float outputs: longer chunks, rarer exact reseeds (HostPlan::f32_*)
    k.table = k.f32 && h.f32_tiles_per_chunk > 0 ? ChunkTable::F32 : h.mixed ? ChunkTable::Lean : ChunkTable::Standard;
    out.pick[out.n++] = k;
    if (!h.mixed) return WFK_OK;
  } else if (h.tlist && h.mixed) {
    // time list: the fully fused and the zero pieces on the pointwise-ops build (same chunking), then the pieces with
    // generic terms on the build with the direct tier
    out.pick[out.n++] = general(false, false);
  }
  out.pick[out.n++] = general(generic, direct);
  return WFK_OK;
}

// The printed name of a pick: the kernel symbol with its template arguments, as rocprofv3 --kernel-trace shows it, but
// for two simplifications that tests and tools rely on: ACC (the short tier's accumulate build) always prints `false`,
// and a slice prints the base symbol (wfk_sample< / wfk_sample_wide<), by whose prefix the tiers are compared.
inline std::string wfk_pick_name(const SamplerPick& k) {
  auto b = [](bool v) { return std::string(v ? "true" : "false"); };
  const std::string T = k.f32 ? "float" : "double", ns = std::to_string(k.ns), fam = std::to_string(k.fam);
  if (k.tier == SamplerTier::Short) return "wfk_sample_short<" + T + "," + b(k.cplx) + ",false," + ns + "," + fam + ">";
  if (k.tier == SamplerTier::Lean) return "wfk_sample_lean<" + T + "," + b(k.cplx) + "," + ns + "," + b(k.corr) + "," + fam + ">";
  const std::string tail = b(k.cplx) + "," + b(k.tlist) + "," + b(k.generic) + "," + b(k.direct) + "," + ns + ">";
  return k.tier == SamplerTier::Wide ? "wfk_sample_wide<" + tail : "wfk_sample<" + T + "," + tail;
}
