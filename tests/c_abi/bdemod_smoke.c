/* Plain-C consumer of the binned demodulator in include/wfk.h: create a plan for a 3-tone matrix with bins of 100
 * samples from sample 3, upload int16 traces with wfk_malloc / wfk_memcpy_h2d, apply, download, and compare every bin
 * with a double loop.  Exit code 0 = ok.  (tests/test_gpu_bdemod.py compiles and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "wfk.h"

int main(void) {
  const int64_t S = 130, N = 2053, start = 3, bin = 100, W = 19; /* one bin fewer than fits: samples are left over */
  const int32_t nf = 3;
  const double f[3] = {11e6, -47e6, 203e6}, sr = 1e9, pi = 3.14159265358979323846;
  double* e = (double*)malloc(sizeof(double) * 2 * N * nf);
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * S * N);
  double* got = (double*)malloc(sizeof(double) * 2 * S * W * nf);
  for (int64_t k = 0; k < N; ++k)
    for (int j = 0; j < nf; ++j) {
      const double ph = 2 * pi * f[j] * ((double)k / sr);
      e[2 * (k * nf + j)] = 2.0 / bin * cos(ph);
      e[2 * (k * nf + j) + 1] = -2.0 / bin * sin(ph);
    }
  unsigned r = 12345u;
  for (int64_t i = 0; i < S * N; ++i) {
    r = r * 1103515245u + 12345u;
    x[i] = (int16_t)(r >> 16);
  }
  if (wfk_bdemod_bin_groups(S, nf, W) != 4) {
    fprintf(stderr, "bin groups: %lld\n", (long long)wfk_bdemod_bin_groups(S, nf, W));
    return 10;
  }
  wfk_bdemod_plan* p = NULL;
  if (wfk_bdemod_plan_create(e, N, nf, WFK_IN_I16, start, bin, W, &p) != WFK_OK) {
    fprintf(stderr, "create: %s\n", wfk_last_error());
    return 11;
  }
  void *xd = NULL, *od = NULL;
  if (wfk_malloc(&xd, sizeof(int16_t) * S * N) != WFK_OK || wfk_malloc(&od, sizeof(double) * 2 * S * W * nf) != WFK_OK)
    return 12;
  if (wfk_memcpy_h2d(xd, x, sizeof(int16_t) * S * N) != WFK_OK) return 13;
  if (wfk_bdemod_apply(p, xd, S, N, od, W * nf, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 14;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(got, od, sizeof(double) * 2 * S * W * nf) != WFK_OK) return 15;
  for (int64_t s = 0; s < S; ++s)
    for (int64_t w = 0; w < W; ++w)
      for (int j = 0; j < nf; ++j) {
        double re = 0, im = 0, bound = 0;
        for (int64_t k = start + w * bin; k < start + (w + 1) * bin; ++k) {
          const double xv = x[s * N + k], er = e[2 * (k * nf + j)], ei = e[2 * (k * nf + j) + 1];
          re += xv * er;
          im += xv * ei;
          bound += fabs(xv) * hypot(er, ei);
        }
        const double* g = got + 2 * ((s * W + w) * nf + j);
        if (!(hypot(g[0] - re, g[1] - im) <= 1e-12 * bound)) {
          fprintf(stderr, "shot %lld bin %lld tone %d: (%g, %g) vs (%g, %g)\n", (long long)s, (long long)w, j, g[0], g[1],
                  re, im);
          return 16;
        }
      }
  printf("bdemod_smoke: %s, %lld bins per shot on the device, parity ok\n", wfk_bdemod_kernel_name(p, S), (long long)W);
  wfk_free(xd);
  wfk_free(od);
  wfk_bdemod_plan_destroy(p);
  free(e);
  free(x);
  free(got);
  return 0;
}
