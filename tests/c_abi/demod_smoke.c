/* Plain-C consumer of the demodulator in include/wfk.h: create a plan for a 3-tone matrix, upload int16
 * traces with wfk_malloc / wfk_memcpy_h2d, apply, download, and compare with a double loop.  Exit code 0 = ok.
 * (tests/test_gpu_demod.py compiles and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "wfk.h"

int main(void) {
  const int64_t S = 130, N = 2053;
  const int32_t nf = 3;
  const double f[3] = {11e6, -47e6, 203e6}, sr = 1e9, pi = 3.14159265358979323846;
  double* e = (double*)malloc(sizeof(double) * 2 * N * nf);
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * S * N);
  double* got = (double*)malloc(sizeof(double) * 2 * S * nf);
  for (int64_t k = 0; k < N; ++k)
    for (int j = 0; j < nf; ++j) {
      const double ph = 2 * pi * f[j] * ((double)k / sr);
      e[2 * (k * nf + j)] = 2.0 / N * cos(ph);
      e[2 * (k * nf + j) + 1] = -2.0 / N * sin(ph);
    }
  unsigned r = 12345u;
  for (int64_t i = 0; i < S * N; ++i) {
    r = r * 1103515245u + 12345u;
    x[i] = (int16_t)(r >> 16);
  }
  wfk_demod_plan* p = NULL;
  if (wfk_demod_plan_create(e, N, nf, WFK_IN_I16, &p) != WFK_OK) {
    fprintf(stderr, "create: %s\n", wfk_last_error());
    return 11;
  }
  void *xd = NULL, *od = NULL;
  if (wfk_malloc(&xd, sizeof(int16_t) * S * N) != WFK_OK || wfk_malloc(&od, sizeof(double) * 2 * S * nf) != WFK_OK)
    return 12;
  if (wfk_memcpy_h2d(xd, x, sizeof(int16_t) * S * N) != WFK_OK) return 13;
  if (wfk_demod_apply(p, xd, S, N, od, nf, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 14;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(got, od, sizeof(double) * 2 * S * nf) != WFK_OK) return 15;
  for (int64_t s = 0; s < S; ++s)
    for (int j = 0; j < nf; ++j) {
      double re = 0, im = 0, bound = 0;
      for (int64_t k = 0; k < N; ++k) {
        const double xv = x[s * N + k], er = e[2 * (k * nf + j)], ei = e[2 * (k * nf + j) + 1];
        re += xv * er;
        im += xv * ei;
        bound += fabs(xv) * hypot(er, ei);
      }
      const double dr = got[2 * (s * nf + j)] - re, di = got[2 * (s * nf + j) + 1] - im;
      if (hypot(dr, di) > 1e-12 * bound) {
        fprintf(stderr, "shot %lld tone %d: (%g, %g) vs (%g, %g)\n", (long long)s, j, got[2 * (s * nf + j)],
                got[2 * (s * nf + j) + 1], re, im);
        return 16;
      }
    }
  wfk_free(xd);
  wfk_free(od);
  wfk_demod_plan_destroy(p);
  free(e);
  free(x);
  free(got);
  printf("demod_smoke: demodulated on the device, parity ok\n");
  return 0;
}
