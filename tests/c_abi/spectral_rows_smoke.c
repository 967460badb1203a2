/* Plain-C consumer of the per-row spectral declarations of include/wfk.h: the host-only parts (argument checks, the
 * quad-precision phase step) run without a device.  Prints "spectral_rows_smoke ok". */
#include <stdio.h>
#include <string.h>

#include "wfk.h"

int main(void) {
  wfk_spectral_rows_plan* plan = NULL;
  wfk_spec_term terms[WFK_SPEC_ROWS_MAX_TERMS + 1];
  int32_t counts[1];
  double hi = 0.0, lo = 0.0;
  int i;
  memset(terms, 0, sizeof terms);
  for (i = 0; i <= WFK_SPEC_ROWS_MAX_TERMS; ++i) {
    terms[i].kind = WFK_SPEC_DELAY;
    terms[i].tau = 1e-9;
  }
  counts[0] = WFK_SPEC_ROWS_MAX_TERMS + 1;
  if (wfk_spectral_rows_plan_create(64, 1, WFK_OUT_F64, 1e9, terms, counts, &plan) != WFK_EINVAL || plan) return 1;
  counts[0] = 1;
  terms[0].kind = WFK_SPEC_REFLECT;
  terms[0].A = 1.0;
  if (wfk_spectral_rows_plan_create(64, 1, WFK_OUT_F64, 1e9, terms, counts, &plan) != WFK_EINVAL) return 2;
  terms[0].A = -1.25;
  if (wfk_spectral_rows_plan_create(64, 1, WFK_OUT_F64, 1e9, terms, counts, &plan) != WFK_EINVAL) return 3;
  terms[0].kind = 7;
  terms[0].A = 0.1;
  if (wfk_spectral_rows_plan_create(64, 1, WFK_OUT_F64, 1e9, terms, counts, &plan) != WFK_EINVAL) return 4;
  if (wfk_spectral_rows_apply(NULL, NULL, 64, NULL, 64, NULL) != WFK_EINVAL) return 5;
  if (wfk_spectral_rows_plan_destroy(NULL) != WFK_OK) return 6;
  /* 0.25 ns at 1 GS/s over 64 samples: 2^-8 cycles per bin, exact */
  if (wfk_spectral_rows_phase_step(0.25, 1.0, 64, &hi, &lo) != WFK_OK || hi != 0.00390625 || lo != 0.0) return 7;
  printf("spectral_rows_smoke ok\n");
  return 0;
}
