/* kacc_group_sums from plain C99: the function is declared with the documented
 * signature and rejects NULL handles before it touches a device
 * (tests/test_group_abi.py).                                                  */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*group_fn)(kacc_ctx *, kacc_kind, const kacc_top_rows *, const uint32_t *, uint32_t, const uint32_t *,
                        uint32_t *, uint64_t *, uint64_t *, double *, uint32_t *, void *);

int main(void) {
  group_fn f = &kacc_group_sums;
  kacc_top_rows rows = {0u, 0u, NULL, NULL, NULL};
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_null = f(NULL, KACC_KIND_PROC, NULL, NULL, 1u, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_rows = f(NULL, KACC_KIND_POD, &rows, NULL, KACC_GROUP_MAX, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  printf("%u %d %d %u %u %u\n", (unsigned)KACC_ABI_VERSION, rc_null, rc_rows, (unsigned)KACC_GROUP_NONE,
         (unsigned)KACC_GROUP_MAX, (unsigned)KACC_GROUP_POWER_FRAC_BITS);
  return 0;
}
