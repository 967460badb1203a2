/* Plain-C consumer of the sampler -> per-row IIR declarations of include/wfk.h, on the device: two channels
 *   A_c * gaussian(0.6) * cos(7 (t - 0.25))  on [-1, 1)   (the program of abi_smoke.c, twice)
 * on 9000 points from -2 in steps of 2^-11 (two whole tiles of the kernel and a partial one; the piece edges fall on
 * samples 2048 and 6144 exactly), each through a first-order section of
 * its own from a level of its own, compared sample by sample with libm + the sequential recurrence in C; the final
 * states too.  Prints "chain_iir_rows_smoke: <kernel name>, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 9000
#define ROWS 2
#define STRIDE 9011

int main(void) {
  const int32_t ch_member_off[] = {0, 1, 2}, mb_piece_off[] = {0, 3, 6};
  const double ch_offset[] = {0, 0}, ch_tshift[] = {0, 0}, lo[] = {-INFINITY, -INFINITY}, hi[] = {INFINITY, INFINITY};
  const double pc_bound[] = {-1.0, 1.0, INFINITY, -1.0, 1.0, INFINITY};
  const int32_t pc_term_off[] = {0, 0, 1, 1, 1, 2, 2};
  const double amp_re[] = {0.5, -0.8}, amp_im[] = {0.0, 0.0};
  const int32_t tm_factor_off[] = {0, 2, 4};
  const int32_t fc_type[] = {WFK_GAUSSIAN, WFK_COS, WFK_GAUSSIAN, WFK_COS};
  const double fc_power[] = {1, 1, 1, 1}, fc_shift[] = {0.0, 0.25, 0.0, 0.25};
  const int64_t fc_arg_off[] = {0, 1, 2, 3, 4};
  const double pool[] = {0.6, 7.0, 0.6, 7.0};
  wfk_program P = {ROWS, 2, 6, 2, 4, 4, ch_member_off, ch_offset, ch_tshift, lo, hi, mb_piece_off,
                   pc_bound, pc_term_off, amp_re, amp_im, tm_factor_off, fc_type, fc_power,
                   fc_shift, fc_arg_off, pool};
  wfk_grid g = {-2.0, 1.0 / 2048, N, 0, 0.0, 0};             /* np.arange(9000) / 2048 - 2 */
  /* one first-order section per row, rows back to back: y = b0 x + z, z = b1 x - a1 y */
  const int32_t orders[] = {1};
  const double b[ROWS * 2] = {1.01, -1.009, 0.98, -0.971}, a[ROWS * 2] = {1.0, -0.999, 1.0, -0.99};
  const double level[ROWS] = {0.125, -0.25};
  const int32_t bad_orders[] = {5};
  static double y[ROWS * STRIDE];
  double zf[ROWS];
  wfk_chain_iir_rows_plan* plan = NULL;
  void *yd = NULL, *zfd = NULL, *ld = NULL;
  int ndev = 0, r;

  if (wfk_chain_iir_rows_plan_create(NULL, &g, 1, orders, b, a, WFK_OUT_F64, &plan) != WFK_EINVAL || plan) return 1;
  if (wfk_chain_iir_rows_plan_create(&P, &g, 1, orders, b, a, WFK_OUT_C128, &plan) != WFK_EINVAL) return 2;
  if (wfk_chain_iir_rows_plan_create(&P, &g, 1, bad_orders, b, a, WFK_OUT_F64, &plan) != WFK_EUNSUP) return 3;
  if (wfk_chain_iir_rows_launch(NULL, NULL, N, NULL, NULL, NULL, NULL) != WFK_EINVAL) return 4;
  if (wfk_chain_iir_rows_plan_destroy(NULL) != WFK_OK) return 5;
  wfk_device_count(&ndev);
  if (ndev <= 0) {
    printf("chain_iir_rows_smoke: no device, argument checks ok\n");
    return 0;
  }
  if (wfk_chain_iir_rows_plan_create(&P, &g, 1, orders, b, a, WFK_OUT_F64, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 11;
  }
  if (wfk_chain_iir_rows_state_dim(plan) != 1 || wfk_chain_iir_rows_table_bytes(plan) <= 0) return 12;
  /* this program is one the fused kernels take: the sampler must run inside the per-row IIR kernel */
  if (!wfk_chain_iir_rows_is_fused(plan) || strlen(wfk_chain_iir_rows_unfused_reason(plan))) {
    fprintf(stderr, "not fused: %s (%s)\n", wfk_chain_iir_rows_unfused_reason(plan), wfk_chain_iir_rows_kernel_name(plan));
    return 13;
  }
  if (strncmp(wfk_chain_iir_rows_kernel_name(plan), "iir_rows_sampled<f64,1,1>", 25) != 0 &&
      strncmp(wfk_chain_iir_rows_kernel_name(plan), "iir_rows_short<f64,1,1>", 23) != 0)
    return 14;
  for (r = 0; r < ROWS * STRIDE; ++r) y[r] = -5.0;
  if (wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&zfd, sizeof zf) != WFK_OK || wfk_malloc(&ld, sizeof level) != WFK_OK)
    return 15;
  if (wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK || wfk_memcpy_h2d(ld, level, sizeof level) != WFK_OK) return 16;
  if (wfk_chain_iir_rows_launch(plan, yd, N - 1, NULL, zfd, ld, NULL) != WFK_EINVAL) return 17;   /* stride < n */
  if (wfk_chain_iir_rows_launch(plan, yd, STRIDE, NULL, zfd, ld, NULL) != WFK_OK) {
    fprintf(stderr, "launch: %s\n", wfk_last_error());
    return 18;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(zf, zfd, sizeof zf) != WFK_OK)
    return 19;
  for (r = 0; r < ROWS; ++r) {
    double z = 0.0;
    int i;
    for (i = 0; i < STRIDE; ++i) {
      const double got = y[r * STRIDE + i];
      double want = -5.0;                                      /* past the row: untouched */
      if (i < N) {
        const double t = (double)i * g.step + g.t0;
        const double x = (i >= 2048 && i < 6144 ? amp_re[r] * exp(-(t / 0.6) * (t / 0.6)) * cos(7.0 * (t - 0.25)) : 0.0) - level[r];
        const double v = b[2 * r] / a[2 * r] * x + z;
        z = b[2 * r + 1] / a[2 * r] * x - a[2 * r + 1] / a[2 * r] * v;
        want = v + level[r];
      }
      if (!(fabs(got - want) <= 1e-10)) {
        fprintf(stderr, "row %d sample %d: got %.17g, want %.17g\n", r, i, got, want);
        return 20;
      }
    }
    if (!(fabs(zf[r] - z) <= 1e-10)) {
      fprintf(stderr, "row %d final state: got %.17g, want %.17g\n", r, zf[r], z);
      return 21;
    }
  }
  printf("chain_iir_rows_smoke: %s, parity ok\n", wfk_chain_iir_rows_kernel_name(plan));
  wfk_chain_iir_rows_plan_destroy(plan);
  wfk_free(yd);
  wfk_free(zfd);
  wfk_free(ld);
  return 0;
}
