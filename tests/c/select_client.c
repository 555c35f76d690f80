/* kacc_select_above from plain C99: the function is declared with the documented
 * signature and rejects NULL handles before it touches a device
 * (tests/test_select_abi.py).                                                 */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*select_fn)(kacc_ctx *, kacc_table, uint32_t, uint64_t, const kacc_top_rows *, const uint32_t *, uint32_t,
                         uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint64_t *, double *, void *);

int main(void) {
  select_fn f = &kacc_select_above;
  kacc_top_rows rows = {0u, 0u, NULL, NULL, NULL};
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_null = f(NULL, KACC_T_PROC_POWER, 0u, 0u, NULL, NULL, 0u, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_rows = f(NULL, KACC_T_POD_ENERGY, 0u, 1u, &rows, NULL, 0u, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  printf("%u %d %d\n", (unsigned)KACC_ABI_VERSION, rc_null, rc_rows);
  return 0;
}
