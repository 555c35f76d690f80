/* kacc_group_quantiles from plain C99: the function is declared with the
 * documented signature and rejects NULL handles before it touches a device
 * (tests/test_quant_abi.py).                                                  */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*quant_fn)(kacc_ctx *, kacc_table, uint32_t, const kacc_top_rows *, const uint32_t *, uint32_t,
                        const double *, uint32_t, const uint32_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t *,
                        double *, double *, void *);

int main(void) {
  quant_fn f = &kacc_group_quantiles;
  kacc_top_rows rows = {0u, 0u, NULL, NULL, NULL};
  double phi[2] = {0.5, 0.99};
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_null = f(NULL, KACC_T_PROC_POWER, 0u, NULL, NULL, 1u, NULL, 0u, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_rows = f(NULL, KACC_T_POD_ENERGY, 0u, &rows, NULL, 1u, phi, 2u, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  printf("%u %d %d %u %u\n", (unsigned)KACC_ABI_VERSION, rc_null, rc_rows, (unsigned)KACC_QUANT_MAX_PHI,
         (unsigned)KACC_QUANT_MAX_QUERIES);
  return 0;
}
