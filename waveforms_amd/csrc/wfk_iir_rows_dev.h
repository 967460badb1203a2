// wfk_iir_rows_dev.h -- what the per-row IIR kernels share: iir_rows_tile (wfk_iir_rows.hip) LOADS a tile of a row into
// LDS, iir_rows_sampled / iir_rows_short (wfk_iir_rows_sampled.hip) EVALUATE it there.  Here: the geometry of the tile and
// the layout of a row's table (built by irw_build_row, wfk_iir_rows.hip).  Everything after the fill -- the same
// arithmetic in the same order for all three -- is the text of wfk_iir_rows_body.inc, which each kernel includes inside
// its tile loop with these names in scope (all but L, t, base and left come from wfk_iir_rows_head.inc, the row head every
// kernel includes at its top):
//   T, NSEC, ORD, D = NSEC * ORD                    the instantiation
//   __shared__ T tile[IRW_THREADS * IRW_PITCH]; __shared__ double s_tot[IRW_WAVES][D], s_carry[2][D]
//                                                   (s_carry[0] = the row's zi before the first tile)
//   tid, lane = tid & 63, wv = tid >> 6 (uniform), my = tile + tid * IRW_PITCH
//   B(s, i), A(s, i)                                the row's coefficients (iir_cascade_step)
//   pw, W = pw + 6 * MM, L[MM]                      the row's T^(2^k) tables, T^64, T^lane as (hi, lo) pairs
//   pre, zf, row, y                                 the row's level, the final states (or null), its index, its output
//   t, base = t * IRW_TILE, left = n - base         the tile
// and IRW_STORE_INC names the text of the body's store section (wfk_iir_rows_store.inc | wfk_iir_rows_store_dac.inc).
#pragma once
#include <hip/hip_runtime.h>

#include "wfk_iir_common.h"

#define IRW_RUN 16                        // samples per lane and tile
#define IRW_THREADS 256
#define IRW_WAVES (IRW_THREADS / 64)
#define IRW_TILE (IRW_RUN * IRW_THREADS)  // 4096 samples: 34 KB of LDS in fp64
#define IRW_PITCH (IRW_RUN + 1)           // elements between the runs of neighbouring lanes
#define IRW_MAXD 4                        // state dimension limit
#define IRW_NPW 7                         // T^(2^k), k = 0 .. 6 (k = 6: one wave)

// the converter side of the kernels that store int16 DAC codes (iir_rows_dac, iir_rows_sampled_dac, iir_rows_short_dac;
// DESIGN.md §3.23): gd [batch][2] = (gain, offset) per row; counts [batch][3] = [below, above, nan] or null; the rails
#define IRW_DAC_PARAMS \
  const double* __restrict__ gd, unsigned long long* __restrict__ counts, double lo, double hi, int shift

// the curve side of the kernels that look every sample up in the row's calibration curve before it enters the tile
// (iir_rows_curve_dac and the _curve_dac builds of the sampled pair; the types: wfk_curve_dev.h):
// crows [batch], the knot and bucket tables they point into, beyond [batch][3] = [below, above, nan] or null, and the
// knots of the plan's largest row (the pitch of xp / fp / slope in the dynamic LDS)
#define IRW_CURVE_PARAMS                                                                                      \
  const CurveRow* __restrict__ crows, const double* __restrict__ cknots, const uint32_t* __restrict__ cbuckets, \
      unsigned long long* __restrict__ beyond, int lds_knots

namespace {

// Bytes of dynamic LDS a curve may take next to the tile of `es`-byte elements: 64 KiB less the static arrays of the
// widest shape (tile, s_tot, s_carry, the two [waves][3] counters), the `extra` static bytes of a kernel with a fill,
// and a line of slack for the region's alignment.
__host__ __device__ constexpr size_t irw_curve_lds_budget(size_t es, size_t extra = 0) {
  return 65536 - (es * IRW_THREADS * IRW_PITCH + (IRW_WAVES + 2) * IRW_MAXD * 8 + 2 * IRW_WAVES * 3 * 8) - extra - 64;
}

// per-row table (doubles): b[NC] a[NC] | pw[IRW_NPW][D][D][2] | lanep[64][D][D][2] (T^l, l = 0 .. 63)
__host__ __device__ constexpr int irw_row_doubles(int nsec, int ord) {
  return 2 * nsec * (ord + 1) + (IRW_NPW + 64) * (nsec * ord) * (nsec * ord) * 2;
}

// element of the tile array that holds sample j of the tile: lane l finds its run of 16 at l * 17 elements
__device__ __forceinline__ int irw_at(int j) { return (j / IRW_RUN) * IRW_PITCH + (j % IRW_RUN); }

}  // namespace
