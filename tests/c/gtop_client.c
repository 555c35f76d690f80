/* kacc_group_top from plain C99: the function is declared with the documented
 * signature and rejects NULL handles before it touches a device
 * (tests/test_gtop_abi.py).                                                   */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*gtop_fn)(kacc_ctx *, kacc_table, uint32_t, uint32_t, const kacc_top_rows *, const uint32_t *, uint32_t,
                       const uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint32_t *, uint64_t *, void *);

int main(void) {
  gtop_fn f = &kacc_group_top;
  kacc_top_rows rows = {0u, 0u, NULL, NULL, NULL};
  uint32_t count[1] = {0u};
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_null = f(NULL, KACC_T_PROC_POWER, 0u, 10u, NULL, NULL, 1u, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_rows = f(NULL, KACC_T_POD_ENERGY, 0u, 10u, &rows, NULL, 1u, NULL, count, NULL, NULL, NULL, NULL, NULL);
  printf("%u %d %d %u %u\n", (unsigned)KACC_ABI_VERSION, rc_null, rc_rows, (unsigned)KACC_TOP_MAX,
         (unsigned)KACC_GROUP_TOP_MAX_ITEMS);
  return 0;
}
