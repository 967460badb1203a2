/* Plain-C consumer of the trace averager in include/wfk.h: int16 traces that cycle through 7 steps arrive in two
 * blocks cut in the middle of a cycle; the first apply overwrites the sums, the second accumulates onto them with
 * `first` = the shots already taken.  The int64 sums and sums of squares are compared with a double loop in C: exact.
 * Exit code 0 = ok.  (tests/test_gpu_avg.py compiles and runs it.) */
#include <stdio.h>
#include <stdlib.h>

#include "wfk.h"

int main(void) {
  const int64_t S = 1003, N = 2053, G = 7, cut = 488;   /* 488 = 69 * 7 + 5: the cut falls inside a cycle */
  const int64_t stride = N + 3;
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * S * stride);
  int64_t* want = (int64_t*)calloc(2 * G * N, sizeof(int64_t));
  int64_t* got = (int64_t*)malloc(sizeof(int64_t) * 2 * G * N);
  unsigned r = 2463534242u;
  for (int64_t i = 0; i < S * stride; ++i) {
    r = r * 1103515245u + 12345u;
    x[i] = (int16_t)(r >> 16);
  }
  for (int64_t s = 0; s < S; ++s)
    for (int64_t c = 0; c < N; ++c) {
      const int64_t v = x[s * stride + c];
      want[(s % G) * N + c] += v;
      want[(G + s % G) * N + c] += v * v;
    }
  wfk_avg_plan* p = NULL;
  if (wfk_avg_plan_create(N, G, WFK_IN_I16, &p) != WFK_OK) {
    fprintf(stderr, "create: %s\n", wfk_last_error());
    return 11;
  }
  void *xd = NULL, *od = NULL;
  if (wfk_malloc(&xd, sizeof(int16_t) * S * stride) != WFK_OK || wfk_malloc(&od, sizeof(int64_t) * 2 * G * N) != WFK_OK)
    return 12;
  if (wfk_memcpy_h2d(xd, x, sizeof(int16_t) * S * stride) != WFK_OK) return 13;
  if (wfk_memset(od, 0x5a, sizeof(int64_t) * 2 * G * N) != WFK_OK) return 13;
  int64_t* sum = (int64_t*)od;
  int64_t* sumsq = sum + G * N;
  if (wfk_avg_apply(p, xd, cut, stride, 0, sum, N, sumsq, N, 0, NULL) != WFK_OK ||
      wfk_avg_apply(p, (const int16_t*)xd + cut * stride, S - cut, stride, cut, sum, N, sumsq, N, 1, NULL) != WFK_OK) {
    fprintf(stderr, "apply: %s\n", wfk_last_error());
    return 14;
  }
  if (wfk_stream_sync(NULL) != WFK_OK || wfk_memcpy_d2h(got, od, sizeof(int64_t) * 2 * G * N) != WFK_OK) return 15;
  for (int64_t i = 0; i < 2 * G * N; ++i)
    if (got[i] != want[i]) {
      fprintf(stderr, "%s of step %lld, column %lld: %lld vs %lld\n", i < G * N ? "sum" : "sumsq",
              (long long)(i / N % G), (long long)(i % N), (long long)got[i], (long long)want[i]);
      return 16;
    }
  if (wfk_avg_splits(p, cut, 0) < 1 || wfk_avg_kernel_name(p, cut, 1)[0] != 'a') return 17;
  /* refusals: a stride below N, a negative first, sums that overlap the traces */
  if (wfk_avg_apply(p, xd, cut, N - 1, 0, sum, N, sumsq, N, 0, NULL) != WFK_EINVAL) return 18;
  if (wfk_avg_apply(p, xd, cut, stride, -1, sum, N, sumsq, N, 0, NULL) != WFK_EINVAL) return 19;
  if (wfk_avg_apply(p, xd, cut, stride, 0, xd, N, sumsq, N, 0, NULL) != WFK_EINVAL) return 20;
  wfk_free(xd);
  wfk_free(od);
  wfk_avg_plan_destroy(p);
  wfk_avg_plan_destroy(NULL);
  free(x);
  free(want);
  free(got);
  printf("avg_smoke: two blocks averaged on the device, sums exact\n");
  return 0;
}
