/* kacc_window_* from plain C99: the functions are declared with the documented
 * signatures and reject NULL handles before they touch a device
 * (tests/test_window_abi.py).                                                 */
#include <stdio.h>

#include "kepler_accel.h"

typedef int (*create_fn)(kacc_ctx *, kacc_kind, uint32_t, kacc_window **);
typedef void (*destroy_fn)(kacc_window *);
typedef int (*step_fn)(kacc_window *, const kacc_top_rows *, const uint32_t *, uint32_t, const kacc_slotmap *,
                       const uint32_t *, const uint32_t *, void *);
typedef int (*mark_fn)(kacc_window *, void *);
typedef int (*read_fn)(kacc_window *, const kacc_top_rows *, const uint32_t *, uint32_t *, uint64_t *, uint64_t *,
                       uint32_t *, uint64_t *, uint64_t *, void *);
typedef int (*download_fn)(kacc_window *, uint64_t, uint64_t, uint64_t *, uint32_t *);

int main(void) {
  create_fn create = &kacc_window_create;
  destroy_fn destroy = &kacc_window_destroy;
  step_fn step = &kacc_window_step;
  mark_fn mark = &kacc_window_mark;
  read_fn read = &kacc_window_read;
  download_fn download = &kacc_window_download;
  kacc_top_rows rows = {0u, 0u, NULL, NULL, NULL};
  kacc_window *w = NULL;
  uint32_t count[1] = {0u};
  uint64_t base[1] = {0u};
  /* NULL handles: KACC_EINVAL, nothing touches a device */
  int rc_create = create(NULL, KACC_KIND_PROC, 1u, &w);
  int rc_step = step(NULL, &rows, NULL, KACC_WINDOW_ASSIGN_ALL, NULL, NULL, NULL, NULL);
  int rc_mark = mark(NULL, NULL);
  int rc_read = read(NULL, &rows, NULL, count, NULL, NULL, NULL, NULL, NULL, NULL);
  int rc_down = download(NULL, 0u, 1u, base, count);
  destroy(NULL);
  printf("%u %d %d %d %d %d %u %u\n", (unsigned)KACC_ABI_VERSION, rc_create, rc_step, rc_mark, rc_read, rc_down,
         (unsigned)KACC_WINDOW_ASSIGN_ALL, (unsigned)(w == NULL));
  return 0;
}
