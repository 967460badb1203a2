/* Plain-C consumer of the probe plan in include/wfk.h: a boxcar integral of three rows read off at probe times
 * (inside the grid, on grid points, outside it), compared with a double loop; then one refused call.
 * Exit code 0 = ok.  (tests/test_gpu_phase_curve.py compiles and runs it.) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wfk.h"

static double box(const double* y, int64_t n, int64_t end, int64_t pp, double gain) {
  double s = 0;
  for (int64_t m = 0; m < pp; ++m) {
    const int64_t i = end - m;
    if (i >= 0 && i < n) s += y[i];
  }
  return gain * s;
}

int main(void) {
  const int64_t n = 3001, rows = 3, stride = 3010, pp = 45, c = 60;
  const int32_t nq = 9;
  const double sr = 2e9, lim = 0.75e-6, gain = 2.5;
  const double t[9] = {-1e-6, -0.75e-6, -0.3e-6 + 0.1e-9, 0.0, 12.25e-9, 0.7e-6, 0.7495e-6, 0.75e-6, 1e-6};
  double* tl = (double*)malloc(sizeof(double) * n);
  double* y = (double*)malloc(sizeof(double) * rows * stride);
  double* got = (double*)malloc(sizeof(double) * rows * nq);
  for (int64_t i = 0; i < n; ++i) tl[i] = (double)i / sr - lim;
  unsigned r = 2024u;
  for (int64_t i = 0; i < rows * stride; ++i) {
    r = r * 1103515245u + 12345u;
    y[i] = (double)(int)(r >> 16) / 65536.0 - 0.5;
  }
  wfk_boxprobe_plan* p = NULL;
  if (wfk_boxprobe_plan_create(tl, n, t, nq, pp, c, gain, &p) != WFK_OK) {
    fprintf(stderr, "create: %s\n", wfk_last_error());
    return 11;
  }
  void *yd = NULL, *od = NULL;
  if (wfk_malloc(&yd, sizeof(double) * rows * stride) != WFK_OK || wfk_malloc(&od, sizeof(double) * rows * nq) != WFK_OK)
    return 12;
  if (wfk_memcpy_h2d(yd, y, sizeof(double) * rows * stride) != WFK_OK) return 13;
  if (wfk_boxprobe_apply(p, (const double*)yd, rows, stride, (double*)od, nq, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 14;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(got, od, sizeof(double) * rows * nq) != WFK_OK) return 15;
  for (int64_t s = 0; s < rows; ++s)
    for (int q = 0; q < nq; ++q) {
      double want;
      const double* row = y + s * stride;
      if (t[q] <= tl[0]) {
        want = box(row, n, c, pp, gain);
      } else if (t[q] >= tl[n - 1]) {
        want = box(row, n, n - 1 + c, pp, gain);
      } else {
        int64_t j = 0;
        while (tl[j + 1] <= t[q]) ++j;
        const double f0 = box(row, n, j + c, pp, gain), f1 = box(row, n, j + 1 + c, pp, gain);
        want = f0 + (f1 - f0) / (tl[j + 1] - tl[j]) * (t[q] - tl[j]);
      }
      if (fabs(got[s * nq + q] - want) > 1e-12 * gain * pp) {
        fprintf(stderr, "row %lld query %d: %.17g vs %.17g\n", (long long)s, q, got[s * nq + q], want);
        return 16;
      }
    }
  if (wfk_boxprobe_apply(p, (const double*)yd, rows, n - 1, (double*)od, nq, NULL) != WFK_EINVAL ||
      strlen(wfk_last_error()) == 0)
    return 17;
  if (strcmp(wfk_boxprobe_kernel_name(p), "boxprobe_wave") != 0) return 18;
  wfk_free(yd);
  wfk_free(od);
  wfk_boxprobe_plan_destroy(p);
  free(tl);
  free(y);
  free(got);
  printf("probe_smoke: probed on the device, parity ok\n");
  return 0;
}
