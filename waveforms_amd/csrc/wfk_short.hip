// wfk_short.hip -- gfx950 sampler for SHORT pieces: the regime Waveform.sample() is used in.
//
// Reference path: calc_parts / _calc / _fill_parts (waveforms/_waveform.pyx:134-169,
// waveforms/waveform.py:524-527) on the grid of Waveform.sample (waveform.py:190:
// np.arange(start, stop, 1 / sample_rate)) at AWG rates: 1-5 GS/s, pulses of 20-40 ns, i.e.
// pieces of 20-200 samples.  The lean kernel (wfk_kernels.hip) strides a lane by 64 samples and
// carries op state from tile to tile; with pieces shorter than its 1024-sample wave tile every
// piece entry costs a libm seed per lane for 1-5 samples of use, and the Gaussian recurrence at
// stride 64 dt is not even admissible (64 dt / sigma > 2).
//
// Geometry here (see WFK_SH_* in wfk_internal.h; the host builds the tables, wfk_compile.cpp):
//   lane  -> one SEGMENT = <= R CONSECUTIVE samples of ONE piece.  The recurrences step by dt
//            (H = dt / sigma ~ 0.08: always admissible); one exact seed per (lane, op) -- short
//            straight-line sin/cos(pi r) and exp kernels, no libm call -- serves the whole run.
//            Lanes of a wave sit in DIFFERENT pieces: every op parameter is per lane, read from
//            the piece's compact record (16 doubles for a Gaussian + DRAG pulse).
//   wave  -> one UNIT = <= 64 segments plus the zero stretches between them, a contiguous range
//            of <= WFK_SH_LCAP samples of one channel.  Results go through LDS (lane l writes its
//            run at its offset; plain or stride-17 padded layout, chosen per unit by the host for
//            the fewest bank conflicts), then the wave stores the
//            range row by row: 64 consecutive samples per store instruction, rows aligned to
//            128-B lines.  Long zero stretches are pure-fill units (no slots, no LDS).
//   workgroup = one wave, walking `units_per_chunk` consecutive units; chunks are dealt to the
//            XCDs in contiguous eighths (same map as the lean kernel).
// All arithmetic is fp64 whatever the output type (the fp32 VALU rate of this part is the fp64
// rate unless packed); T only sets the width of the LDS staging and of the stores.
// Bound: HBM writes (8 / 4 / 16 B per sample) + the record, slot and unit tables (96 B per op of a
// piece, 128 B for cubics; 4 B per segment; 64 B per unit: +24 % at 60 samples per piece).
// No contraction => no MFMA.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <utility>

#include "wfk.h"
#include "wfk_internal.h"
#include "wfk_pick.h"
#include "wfk_short_dev.h"

namespace {

[[maybe_unused]] __device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
#define WFK_CONST __attribute__((address_space(4)))
template <typename V>
__device__ __forceinline__ V cload(const void* base, int64_t byte_off) {
  return *reinterpret_cast<const WFK_CONST V*>(reinterpret_cast<uintptr_t>(base) + byte_off);
}
template <typename P>
__device__ __forceinline__ P* uniptr(P* p) {
  using G = __attribute__((address_space(1))) P*;
  return (P*)reinterpret_cast<G>(uni64(reinterpret_cast<int64_t>(p)));
}

using namespace shdev;

template <typename T> struct ShOut;
template <> struct ShOut<double> { using Cplx = double2; };
template <> struct ShOut<float> { using Cplx = float2; };

__device__ __forceinline__ int swz(int i) { return i + (i >> 4); }   // lane stride 16 -> 17 elements

#ifndef WFK_SH_WAVES
#define WFK_SH_WAVES 3
#endif
struct UnitDesc {
  int64_t j0, rec0;
  int ch, ns, slot0, nslots, gaps, do_clip;
  double offset, clip_lo, clip_hi;
};
__device__ __forceinline__ UnitDesc load_unit(const ShortUnit* up) {
  UnitDesc u;
  u.j0 = cload<int64_t>(up, offsetof(ShortUnit, j0));
  u.ch = cload<int32_t>(up, offsetof(ShortUnit, ch));
  u.ns = cload<int32_t>(up, offsetof(ShortUnit, n_samples));
  u.slot0 = cload<int32_t>(up, offsetof(ShortUnit, slot0));
  u.nslots = cload<int32_t>(up, offsetof(ShortUnit, n_slots));
  u.gaps = cload<int32_t>(up, offsetof(ShortUnit, gaps));
  u.do_clip = cload<int32_t>(up, offsetof(ShortUnit, do_clip));
  u.offset = cload<double>(up, offsetof(ShortUnit, offset));
  u.clip_lo = cload<double>(up, offsetof(ShortUnit, clip_lo));
  u.clip_hi = cload<double>(up, offsetof(ShortUnit, clip_hi));
  u.rec0 = cload<int64_t>(up, offsetof(ShortUnit, rec0));
  return u;
}

// Raw buffer resources: the hardware range check does the masking.  A lane whose byte offset is
// >= num_records (or "negative": huge as unsigned) loads 0 / stores nothing, so masked row stores and
// the slot load of a partly filled unit are straight-line code without exec-mask branches.
// Cache policy of the row stores: non-temporal (nt).  The output is a write-once stream several times the
// size of L2 + Infinity Cache; written through L2 as ordinary lines it evicts the record and slot tables the
// neighbouring waves are about to read.  Same box, 2048 x 1e5 fp64: back-to-back pulses 0.414 -> 0.400 ms,
// 30 % duty (table lines re-used across the fill units) 0.444 -> 0.358 ms; sc0 / sc1 instead: no gain.
#ifndef WFK_SH_STORE_AUX
#define WFK_SH_STORE_AUX 2
#endif
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
template <typename E>
__device__ __forceinline__ void buf_store(const E& v, __amdgpu_buffer_rsrc_t r, int byte_off) {
  if constexpr (sizeof(E) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte_off, 0, WFK_SH_STORE_AUX);
  else if constexpr (sizeof(E) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, byte_off, 0, WFK_SH_STORE_AUX);
  else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, WFK_SH_STORE_AUX);
}
template <typename E>
__device__ __forceinline__ E buf_load(__amdgpu_buffer_rsrc_t r, int byte_off) {
  if constexpr (sizeof(E) == 4) return __builtin_bit_cast(E, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
  else if constexpr (sizeof(E) == 8) return __builtin_bit_cast(E, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0));
  else return __builtin_bit_cast(E, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

template <typename E, bool CPLX>
__device__ __forceinline__ void add_old(E& v, const E& old) {
  if constexpr (CPLX) { v.x += old.x; v.y += old.y; } else { v += old; }
}

// ---- the DAC build (wfk_sample_short_dac): what it has beside the sampler's own body --------------------------------
__device__ __forceinline__ void buf_store16(int16_t v, __amdgpu_buffer_rsrc_t r, int byte_off) {
  __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), r, byte_off, 0, WFK_SH_STORE_AUX);
}
// one sample to its code, statement by statement what dac_block (wfk_dac_rows.hip) does: a rounded product and a
// rounded sum, rint, the rails compared in double, NaN -> 0; `rails`: below | above << 16, `isnan`: 0 / 1 (a unit has
// <= 1008 samples: a wave's sums of these stay inside their 16 bits)
__device__ __forceinline__ int16_t dac_code(double v, double gain, double offset, double lo, double hi, int shift,
                                            unsigned& rails, unsigned& isnan) {
#pragma clang fp contract(off)
  const double w = v * gain + offset;
  const double q = rint(w);
  const bool nan = w != w, below = q < lo, above = q > hi;
  const double c = nan ? 0.0 : below ? lo : above ? hi : q;
  rails = (unsigned)below | ((unsigned)above << 16);
  isnan = (unsigned)nan;
  return (int16_t)((int)c * (1 << shift));
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {     // every lane gets the sum over the wave
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

// elements of the staging array: the longest unit (WFK_SH_LCAP samples + 15 of row alignment = 16 rows
// of 64) in the 17-per-16 swizzle, plus the overrun of a last partial row
constexpr int kStage = 68 * 16 + 16;

// Software pipeline over the units of a chunk.  Every stage of the chain unit -> slot -> op record
// is a dependent memory round trip of 1-2 us, as long as the evaluation of a whole unit, and on this
// ISA loads and stores share ONE in-order counter (vmcnt): waiting for a load also waits for every
// store issued before it.  So:
//   * at the top of unit u the wave holds desc(u), desc(u+1), the decoded slot of u and the first op
//     record of u (issued BEFORE the stores of u-1: the wait for it leaves those stores in flight);
//   * it issues desc(u+2) and slot(u+1), evaluates u, decodes slot(u+1), issues the first record of
//     u+1, then stages and stores u;
//   * a unit is stored by a FIXED sequence of 16 masked row stores (units span <= 16 rows, the host
//     sees to that): with a variable row loop the compiler cannot count the stores behind a load and
//     falls back to vmcnt(0) at the loop's back edge -- every wave then idles until its own stores
//     have been acknowledged (measured: 6 us per unit).
// FAM: the op family the plan needs (HostPlan::short_fam) -- 0: carrier-envelope ops and nothing else (the plain pulse train:
// the body of round 3); 1: + the closing ops of flat-top edges (erf) and multi-tone pieces (shared Gaussian), linear chirps,
// envelope seeds skipped where no lane has an envelope; 2: + table / mollifier envelopes (closing multipliers, own-term ops); 3: family 0
// in packed fp32 (real float launches); 4: + exponential / hyperbolic chirp multipliers; 6: family 0 + carriers with the
// grid-rounding correction (pulse trains milliseconds from t = 0).  Separate instantiations, so that a shape added to one family cannot move the code generation of the others (the
// chirp / cmul / shared-envelope ops of round 4, inlined into the one body, cost the plain pulse train 23 % more VALU
// instructions and 113-120 spilled SGPRs).
#ifndef WFK_SH_WAVES6
#define WFK_SH_WAVES6 2       // family 6 (corrected carriers): 219 registers and no spill at two waves per SIMD against 168 + 46 spilled
#endif                        // at three -- rows 1 ms from t = 0, same box: 1.06 -> 0.835 ms
// DAC / COUNT: off in the sampler (wfk_sample_short); the DAC build without / with the clip report
// (wfk_sample_short_dac: T = double, real, no accumulate).  Same unit walk, same op evaluation, same pipeline; what differs is what a sample
// becomes once it is final.  The sample v = acc[k] + offset goes through dac_code with the row's gain and offset (a
// second scalar load, issued for the NEXT unit as the descriptors are) and is staged as an int16 code at head + i,
// head = the unit's first code's position in its 16-byte group of 8 -- the groups are laid out from the 16-byte
// boundary at or before the output row's first code, whatever 2-byte offset the row starts at.  The unit (<= 7 + 1008
// codes: <= 127 groups) leaves in THREE masked store instructions: two of 16 bytes per lane for the groups that lie
// whole inside the unit, one of 2 bytes per lane (lanes 0-7: group 0, lanes 8-15: the last group) for the codes of a
// first and a last partial group -- those 16 bytes are shared with the neighbouring unit, which another wave owns (or
// with whatever lies in front of and behind the row), and are never read or written as a whole.  A pure-fill unit
// stores the code of the channel's constant the same way.  Counting (COUNT): every lane counts its own run's samples
// below / above the rails and NaN, the wave sums them (two packed words through the cross-lane network), the samples
// of the unit no run covers count as the constant does, and lanes 0-2 add the three sums to the row's int64 counters,
// one atomic each where the sum is not zero.  Integer sums: the report does not depend on the order of arrival.
// The body is ONE text, wfk_short_body.inc, included into both kernels -- not a function the two call: handed the
// kernel's arguments by reference, the compiler first copied them out of the kernel-argument segment, and 42 of the
// sampler's 44 instantiations came out with other instruction words and registers (tools/kernel_cmp.py).  The body
// reads T, CPLX, ACC, R, FAM, DAC, COUNT, `a` and `dk` from where it is included; DAC and COUNT depend on a template
// parameter in both kernels, so that the other build's statements are discarded, never instantiated.
template <typename T, bool CPLX, bool ACC, int R, int FAM>
__global__ void __launch_bounds__(64, CPLX ? 2 : (FAM == 6 ? WFK_SH_WAVES6 : WFK_SH_WAVES)) wfk_sample_short(const SArgs a) {
  constexpr bool DAC = sizeof(T) == 0, COUNT = DAC;
  [[maybe_unused]] const DacKArgs dk{};
#include "wfk_short_body.inc"
}

// the DAC build: int16 codes to a.out, rows a.ch_stride codes apart; real double arithmetic, no accumulate
// (family 4, and the counting builds of families 1 and 2, spill 2 to 13 VGPRs to scratch at three waves per SIMD: two)
template <int R, int FAM, bool COUNTED>
__global__ void __launch_bounds__(64, FAM == 6 || FAM == 4 || (COUNTED && FAM != 0) ? WFK_SH_WAVES6 : WFK_SH_WAVES) wfk_sample_short_dac(const SArgs a, const DacKArgs dk) {
  using T = double;
  constexpr bool DAC = FAM >= 0, COUNT = COUNTED, CPLX = !DAC, ACC = !DAC;
  static_assert(FAM != 3, "family 3 is packed fp32: no DAC build");
#include "wfk_short_body.inc"
}

// one build of the kernel, the pick's: 0 / 1 / 2 / 4 / 6, and 3 = family 0 in packed fp32 (real float outputs only)
template <typename T, bool CPLX, bool ACC>
bool launch_short(const SArgs& a, int build, unsigned blocks, hipStream_t s) {
#define SH_LAUNCH(FAMV) hipLaunchKernelGGL((wfk_sample_short<T, CPLX, ACC, WFK_SH_R, FAMV>), dim3(blocks), dim3(64), 0, s, a)
  switch (build) {
    case 0: SH_LAUNCH(0); return true;
    case 1: SH_LAUNCH(1); return true;
    case 2: SH_LAUNCH(2); return true;
    case 3: if constexpr (std::is_same<T, float>::value && !CPLX) { SH_LAUNCH(3); return true; } return false;
    case 4: SH_LAUNCH(4); return true;
    case 6: SH_LAUNCH(6); return true;
  }
#undef SH_LAUNCH
  return false;
}

template <bool COUNT>
bool launch_short_dac(const SArgs& a, const DacKArgs& d, int fam, unsigned blocks, hipStream_t s) {
#define SH_LAUNCH(FAMV) hipLaunchKernelGGL((wfk_sample_short_dac<WFK_SH_R, FAMV, COUNT>), dim3(blocks), dim3(64), 0, s, a, d)
  switch (fam) {
    case 0: SH_LAUNCH(0); return true;
    case 1: SH_LAUNCH(1); return true;
    case 2: SH_LAUNCH(2); return true;
    case 4: SH_LAUNCH(4); return true;
    case 6: SH_LAUNCH(6); return true;
  }
#undef SH_LAUNCH
  return false;
}

}  // namespace

int wfk_launch_short_dac(const SArgs& a, const DacKArgs& d, int fam, void* stream, std::string& err) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t blocks = ((a.n_chunks + 7) >> 3) << 3;
  if (blocks == 0) return WFK_OK;
  if (blocks > 0x7fffffffLL) { err = "grid too large"; return WFK_EINVAL; }
  if (a.lds_samples > WFK_SH_LCAP) { err = "short plan: unit longer than the staging array"; return WFK_EINVAL; }
  const bool built = d.counts ? launch_short_dac<true>(a, d, fam, (unsigned)blocks, s)
                              : launch_short_dac<false>(a, d, fam, (unsigned)blocks, s);
  if (!built) { err = "short plan: no DAC build for op family " + std::to_string(fam); return WFK_EINVAL; }
  if (hipGetLastError() != hipSuccess) { err = std::string("short DAC kernel launch failed: ") + hipGetErrorString(hipGetLastError()); return WFK_EHIP; }
  return WFK_OK;
}

int wfk_launch_short(const SArgs& a, const SamplerPick& k, void* stream, std::string& err) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t blocks = ((a.n_chunks + 7) >> 3) << 3;
  if (blocks == 0) return WFK_OK;
  if (blocks > 0x7fffffffLL) { err = "grid too large"; return WFK_EINVAL; }
  if (a.lds_samples > WFK_SH_LCAP) { err = "short plan: unit longer than the staging array"; return WFK_EINVAL; }
  const bool built = wfk_with_kind(k.f32, k.cplx, [&](auto t, auto c) {
    return a.accumulate ? launch_short<decltype(t), decltype(c)::value, true>(a, k.fam, (unsigned)blocks, s)
                        : launch_short<decltype(t), decltype(c)::value, false>(a, k.fam, (unsigned)blocks, s);
  });
  if (!built) { err = "short plan: no build for op family " + std::to_string(k.fam); return WFK_EINVAL; }
  if (hipGetLastError() != hipSuccess) { err = std::string("short kernel launch failed: ") + hipGetErrorString(hipGetLastError()); return WFK_EHIP; }
  return WFK_OK;
}
