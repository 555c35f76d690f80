/* The terminated-export entry points from plain C99: both functions are
 * declared with the documented signatures and KACC_TRACKER_READ_CLEAR is a
 * preprocessor constant (tests/test_tracker_export_abi.py).                 */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*read_fn)(kacc_tracker *, const uint32_t *, uint32_t, uint32_t, uint32_t *, uint64_t *, uint32_t *,
                       uint64_t *, double *, void *);
typedef int (*lines_dev_fn)(kacc_ctx *, int, const void *, uint64_t, const char *, const char *const *,
                            const uint32_t *, uint32_t, const char *, const uint64_t *, const uint32_t *, uint64_t *,
                            char *, uint64_t, uint64_t *, void *);

int main(void) {
  read_fn r = &kacc_tracker_read;
  lines_dev_fn f = &kacc_format_lines_dev;
  uint64_t total = 7;
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_r = r(NULL, NULL, 0u, 0u, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_f = f(NULL, 1, NULL, 0u, NULL, NULL, NULL, 0u, NULL, NULL, NULL, NULL, NULL, 0u, &total, NULL);
  printf("%u %u %d %d\n", (unsigned)KACC_TRACKER_READ_CLEAR, (unsigned)KACC_ABI_VERSION, rc_r, rc_f);
  return 0;
}
