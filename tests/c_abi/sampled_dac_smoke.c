/* Plain-C consumer of the sampler -> DAC codes declarations of include/wfk.h, on the device: two channels
 *   A_c * gaussian(0.6) * cos(7 (t - 0.25))  on [-1, 1)   (the program of abi_smoke.c, twice)
 * on 200 points from -3 in steps of 2^-5 (the pulse is 64 samples long: the short tier's regime), scaled by a gain and
 * an offset of their own to 14-bit codes, left-justified by 2, into rows that start 3 codes into a wider buffer.
 * Compared code by code with libm in C (a sample within 1e-6 LSB of a rounding tie may differ by one code), the counts
 * with what the codes show, the codes around the rows untouched.
 * Prints "sampled_dac_smoke: <kernel name>, parity ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define N 200
#define ROWS 2
#define STRIDE 215
#define LEAD 3

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
  wfk_grid g = {-3.0, 1.0 / 32, N, 0, 0.0, 0};                /* np.arange(200) / 32 - 3 */
  const double gain[ROWS] = {20000.25, 9000.5}, offset[ROWS] = {100.5, -3.25}, bad_gain[ROWS] = {1.0, NAN};
  const int bits = 14, shift = 2;
  const double rail_lo = -8192.0, rail_hi = 8191.0;
  static int16_t y[ROWS * STRIDE];
  int64_t counts[ROWS * 3], want_counts[ROWS * 3];
  wfk_chain_dac_plan* plan = NULL;
  void *yd = NULL, *cd = NULL, *sd = NULL;
  int ndev = 0, r, i;

  if (wfk_chain_dac_plan_create(NULL, &g, gain, offset, bits, shift, 1, &plan) != WFK_EINVAL || plan) return 1;
  if (wfk_chain_dac_plan_create(&P, &g, bad_gain, offset, bits, shift, 1, &plan) != WFK_EINVAL || plan) return 2;
  if (!strstr(wfk_last_error(), "row 1: gain is not finite")) return 3;
  if (wfk_chain_dac_plan_create(&P, &g, gain, offset, 17, 0, 1, &plan) != WFK_EINVAL) return 4;
  if (wfk_chain_dac_plan_create(&P, &g, gain, offset, bits, 3, 1, &plan) != WFK_EINVAL) return 5;
  if (wfk_chain_dac_plan_create(&P, &g, gain, offset, bits, shift, 3, &plan) != WFK_EINVAL) return 6;
  if (wfk_chain_dac_launch(NULL, NULL, N, NULL, NULL, 0, NULL) != WFK_EINVAL) return 7;
  if (wfk_chain_dac_plan_destroy(NULL) != WFK_OK) return 8;
  wfk_device_count(&ndev);
  if (ndev <= 0) {
    printf("sampled_dac_smoke: no device, argument checks ok\n");
    return 0;
  }
  if (wfk_chain_dac_plan_create(&P, &g, gain, offset, bits, shift, 1, &plan) != WFK_OK) {
    fprintf(stderr, "plan_create: %s\n", wfk_last_error());
    return 11;
  }
  if (wfk_chain_dac_table_bytes(plan) <= 0) return 12;
  /* a reason exactly where the sampler does not write the codes itself */
  if (!wfk_chain_dac_is_fused(plan) != (strlen(wfk_chain_dac_unfused_reason(plan)) != 0)) return 13;
  for (i = 0; i < ROWS * STRIDE; ++i) y[i] = -21846;
  if (wfk_malloc(&yd, sizeof y) != WFK_OK || wfk_malloc(&cd, sizeof counts) != WFK_OK ||
      wfk_malloc(&sd, sizeof(double) * ROWS * N) != WFK_OK)
    return 15;
  if (wfk_memcpy_h2d(yd, y, sizeof y) != WFK_OK) return 16;
  if (wfk_chain_dac_launch(plan, (int16_t*)yd + LEAD, N - 1, cd, sd, N, NULL) != WFK_EINVAL) return 17;   /* stride < n */
  if (wfk_chain_dac_launch(plan, (int16_t*)yd + LEAD, STRIDE, (int64_t*)((char*)cd + 4), sd, N, NULL) != WFK_EINVAL) return 18;
  if (wfk_chain_dac_launch(plan, (int16_t*)yd + LEAD, STRIDE, cd, sd, N, NULL) != WFK_OK) {
    fprintf(stderr, "launch: %s\n", wfk_last_error());
    return 19;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(y, yd, sizeof y) != WFK_OK ||
      wfk_memcpy_d2h(counts, cd, sizeof counts) != WFK_OK)
    return 20;
  memset(want_counts, 0, sizeof want_counts);
  for (r = 0; r < ROWS; ++r) {
    for (i = 0; i < STRIDE; ++i) {
      const int got = y[r * STRIDE + i];
      int want = -21846, slack = 0;                               /* around the row: untouched */
      if (i >= LEAD && i < LEAD + N) {
        const double t = (double)(i - LEAD) * g.step + g.t0;
        const double x = t >= -1.0 && t < 1.0 ? amp_re[r] * exp(-(t / 0.6) * (t / 0.6)) * cos(7.0 * (t - 0.25)) : 0.0;
        const double v = x * gain[r] + offset[r], q = rint(v);
        const double c = q < rail_lo ? rail_lo : q > rail_hi ? rail_hi : q;
        want = (int)c * (1 << shift);
        slack = fabs(fabs(v - floor(v)) - 0.5) < 1e-6 ? (1 << shift) : 0;
        want_counts[3 * r] += q < rail_lo;
        want_counts[3 * r + 1] += q > rail_hi;
      }
      if (abs(got - want) > slack) {
        fprintf(stderr, "row %d code %d: got %d, want %d\n", r, i, got, want);
        return 21;
      }
    }
    for (i = 0; i < 3; ++i)
      if (counts[3 * r + i] != want_counts[3 * r + i]) {
        fprintf(stderr, "row %d counter %d: got %lld, want %lld\n", r, i, (long long)counts[3 * r + i], (long long)want_counts[3 * r + i]);
        return 22;
      }
  }
  if (want_counts[1] == 0) return 23;                             /* row 0 does clip at the top rail */
  printf("sampled_dac_smoke: %s, parity ok\n", wfk_chain_dac_kernel_name(plan, 1));
  wfk_chain_dac_plan_destroy(plan);
  wfk_free(yd);
  wfk_free(cd);
  wfk_free(sd);
  return 0;
}
