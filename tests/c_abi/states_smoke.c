/* Plain-C consumer of the state discriminator in include/wfk.h: IQ points of 3 tones (3 states, the last tone has 2
 * and pads with NaN) that cycle through 7 steps arrive in two blocks cut in the middle of a cycle; the first apply
 * overwrites the counts and the joint histogram, the second accumulates onto them with `first` = the shots already
 * taken.  Labels, words, counts and the joint histogram are compared with loops in C: exact.  The points have a row
 * stride above n_tones and carry a NaN, so one shot is invalid.
 * Exit code 0 = ok.  (tests/test_gpu_states.py compiles and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

#define NF 3
#define K 3
#define G 7
#define BITS 2
#define BINS ((1 << (NF * BITS)) + 1)

int main(void) {
  const int64_t S = 1003, cut = 488, stride = NF + 2;   /* 488 = 69 * 7 + 5: the cut falls inside a cycle */
  const double centres[NF * K * 2] = {1, 0, -1, 0, 0, 1.5, 0.5, 0.5, -0.5, -0.5, 2, -2, 0, 1, 0, -1, NAN, NAN};
  double* x = (double*)malloc(sizeof(double) * 2 * S * stride);
  uint8_t* want_lab = (uint8_t*)malloc(S * NF);
  uint8_t* got_lab = (uint8_t*)malloc(S * NF);
  int64_t* want_w = (int64_t*)malloc(sizeof(int64_t) * S);
  int64_t* got_w = (int64_t*)malloc(sizeof(int64_t) * S);
  int64_t want_c[G * NF * (K + 1)], got_c[G * NF * (K + 1)], want_j[G * BINS], got_j[G * BINS];
  memset(want_c, 0, sizeof want_c);
  memset(want_j, 0, sizeof want_j);
  unsigned r = 2463534242u;
  for (int64_t i = 0; i < 2 * S * stride; ++i) {
    r = r * 1103515245u + 12345u;
    x[i] = ((double)(r >> 8) / 8388608.0 - 1.0) * 2.5;   /* a 24-bit grid in [-2.5, 2.5): squares and sums are exact */
  }
  x[2 * (17 * stride + 1)] = NAN;                         /* shot 17, tone 1 */
  for (int64_t s = 0; s < S; ++s) {
    int64_t word = 0;
    int bad = 0;
    for (int j = 0; j < NF; ++j) {
      double best = INFINITY;
      int winner = 255;
      for (int k = 0; k < K; ++k) {
        const double dr = x[2 * (s * stride + j)] - centres[2 * (j * K + k)];
        const double di = x[2 * (s * stride + j) + 1] - centres[2 * (j * K + k) + 1];
        const double d2 = dr * dr + di * di;
        if (d2 < best) {
          best = d2;
          winner = k;
        }
      }
      want_lab[s * NF + j] = (uint8_t)winner;
      want_c[((s % G) * NF + j) * (K + 1) + (winner == 255 ? K : winner)] += 1;
      bad = bad || winner == 255;
      word |= (int64_t)winner << (j * BITS);
    }
    want_w[s] = bad ? -1 : word;
    want_j[(s % G) * BINS + (bad ? BINS - 1 : word)] += 1;
  }
  wfk_states_plan* p = NULL;
  if (wfk_states_plan_create(centres, NF, K, G, &p) != WFK_OK) {
    fprintf(stderr, "create: %s\n", wfk_last_error());
    return 11;
  }
  void *xd = NULL, *ld = NULL, *wd = NULL, *cd = NULL, *jd = NULL;
  if (wfk_malloc(&xd, sizeof(double) * 2 * S * stride) != WFK_OK || wfk_malloc(&ld, S * NF) != WFK_OK ||
      wfk_malloc(&wd, sizeof(int64_t) * S) != WFK_OK || wfk_malloc(&cd, sizeof want_c) != WFK_OK ||
      wfk_malloc(&jd, sizeof want_j) != WFK_OK)
    return 12;
  if (wfk_memcpy_h2d(xd, x, sizeof(double) * 2 * S * stride) != WFK_OK) return 13;
  if (wfk_memset(cd, 0x5a, sizeof want_c) != WFK_OK || wfk_memset(jd, 0x5a, sizeof want_j) != WFK_OK) return 13;
  if (wfk_states_apply(p, xd, cut, stride, 0, (uint8_t*)ld, NF, (int64_t*)wd, (int64_t*)cd, (int64_t*)jd, 0, NULL) != WFK_OK ||
      wfk_states_apply(p, (const double*)xd + 2 * cut * stride, S - cut, stride, cut, (uint8_t*)ld + cut * NF, NF,
                       (int64_t*)wd + cut, (int64_t*)cd, (int64_t*)jd, 1, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 14;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(got_lab, ld, S * NF) != WFK_OK ||
      wfk_memcpy_d2h(got_w, wd, sizeof(int64_t) * S) != WFK_OK || wfk_memcpy_d2h(got_c, cd, sizeof got_c) != WFK_OK ||
      wfk_memcpy_d2h(got_j, jd, sizeof got_j) != WFK_OK)
    return 15;
  for (int64_t i = 0; i < S * NF; ++i)
    if (got_lab[i] != want_lab[i]) {
      fprintf(stderr, "label of shot %lld, tone %lld: %d vs %d\n", (long long)(i / NF), (long long)(i % NF), got_lab[i],
              want_lab[i]);
      return 16;
    }
  if (want_lab[17 * NF + 1] != 255 || want_w[17] != -1) return 17;
  for (int64_t s = 0; s < S; ++s)
    if (got_w[s] != want_w[s]) {
      fprintf(stderr, "word of shot %lld: %lld vs %lld\n", (long long)s, (long long)got_w[s], (long long)want_w[s]);
      return 18;
    }
  if (memcmp(got_c, want_c, sizeof want_c) != 0) return 19;
  if (memcmp(got_j, want_j, sizeof want_j) != 0) return 20;
  if (wfk_states_kernel_name(p, cut)[0] != 's') return 21;
  /* refusals: a stride below n_tones, a negative first, no output, labels that overlap the points */
  if (wfk_states_apply(p, xd, cut, NF - 1, 0, (uint8_t*)ld, NF, NULL, NULL, NULL, 0, NULL) != WFK_EINVAL) return 22;
  if (wfk_states_apply(p, xd, cut, stride, -1, (uint8_t*)ld, NF, NULL, NULL, NULL, 0, NULL) != WFK_EINVAL) return 23;
  if (wfk_states_apply(p, xd, cut, stride, 0, NULL, NF, NULL, NULL, NULL, 0, NULL) != WFK_EINVAL) return 24;
  if (wfk_states_apply(p, xd, cut, stride, 0, (uint8_t*)xd, NF, NULL, NULL, NULL, 0, NULL) != WFK_EINVAL) return 25;
  wfk_free(xd);
  wfk_free(ld);
  wfk_free(wd);
  wfk_free(cd);
  wfk_free(jd);
  wfk_states_plan_destroy(p);
  wfk_states_plan_destroy(NULL);
  free(x);
  free(want_lab);
  free(got_lab);
  free(want_w);
  free(got_w);
  printf("states_smoke: two blocks discriminated on the device, labels, words and counts exact\n");
  return 0;
}
