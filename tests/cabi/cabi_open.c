/* Plain-C consumer of the opening calls of include/starkperp.h (sp_commit_open_size, sp_commit_open).  Built and run by
 * tests/test_gpu_commit_open.py.  A 4 x 2 table is committed with sp_commit_rows_dev; two of its rows are opened, out of
 * order, by one sp_commit_open call, whose output goes to sp_merkle_verify_paths as it comes (off, keys = rows, the
 * tree's root); a changed sibling fails its own item only; a refused call writes nothing.
 * Device memory comes from the HIP runtime the library has already loaded, found with dlsym: no HIP header needed. */
#define _GNU_SOURCE /* RTLD_DEFAULT */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

#define ROWS 4
#define COLS 2

typedef int (*malloc_fn)(void**, size_t);
typedef int (*memcpy_fn)(void*, const void*, size_t, int);
typedef int (*free_fn)(void*);

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
  memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
  free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
  if (!dev_malloc || !dev_memcpy || !dev_free) { fprintf(stderr, "no HIP runtime in the process\n"); return 3; }
  const int to_device = 1, to_host = 2; /* hipMemcpyHostToDevice, hipMemcpyDeviceToHost */

  uint64_t table[COLS][ROWS][4];
  for (int c = 0; c < COLS; ++c)
    for (int r = 0; r < ROWS; ++r) {
      table[c][r][0] = 1000 + 10 * c + r, table[c][r][1] = 7 * r, table[c][r][2] = c, table[c][r][3] = 1;
    }
  void *d_cols = NULL, *d_levels = NULL;
  if (dev_malloc(&d_cols, sizeof(table)) != 0 || dev_malloc(&d_levels, (2 * ROWS - 1) * 32) != 0) return 4;
  if (dev_memcpy(d_cols, table, sizeof(table), to_device) != 0) return 5;
  uint8_t st = 0xEE;
  if (sp_commit_rows_dev((const uint64_t*)d_cols, ROWS, COLS, (uint64_t*)d_levels, &st, NULL) != SP_OK || st != SP_HASH_OK) {
    fprintf(stderr, "commit: %s\n", sp_last_error());
    return 6;
  }
  uint64_t root[4];
  if (dev_memcpy(root, (char*)d_levels + (2 * ROWS - 2) * 32, 32, to_host) != 0) return 7;

  const void* cols[1] = {d_cols};
  const void* levels[1] = {d_levels};
  const size_t stride[1] = {ROWS}, n_rows[1] = {ROWS}, n_cols[1] = {COLS};
  const uint32_t table_of[2] = {0, 0};
  const uint64_t rows[2] = {3, 0};
  size_t nv = 0, ns = 0;
  if (sp_commit_open_size(1, n_rows, n_cols, 2, table_of, &nv, &ns) != SP_OK || nv != 2 * COLS || ns != 2 * 2) return 8;
  uint64_t values[2 * COLS][4], leaves[2][4], sib[4][4];
  uint32_t val_off[3], off[3];
  if (sp_commit_open(1, cols, stride, n_rows, n_cols, levels, 2, table_of, rows, &values[0][0], val_off, &leaves[0][0],
                     &sib[0][0], off) != SP_OK) {
    fprintf(stderr, "open: %s\n", sp_last_error());
    return 9;
  }
  if (val_off[0] != 0 || val_off[1] != COLS || val_off[2] != 2 * COLS || off[0] != 0 || off[1] != 2 || off[2] != 4) return 10;
  for (int i = 0; i < 2; ++i)
    for (int c = 0; c < COLS; ++c)
      if (memcmp(values[val_off[i] + c], table[c][rows[i]], 32) != 0) return 11;

  uint8_t verdict[2], status[2];
  if (sp_merkle_verify_paths(&leaves[0][0], &sib[0][0], off, 0, rows, 2, root, 1, verdict, status) != SP_OK) {
    fprintf(stderr, "verify: %s\n", sp_last_error());
    return 12;
  }
  if (verdict[0] != SP_PATH_TRUE || verdict[1] != SP_PATH_TRUE || status[0] != SP_HASH_OK || status[1] != SP_HASH_OK) return 13;
  sib[off[1] + 1][2] ^= 1; /* the upper sibling of the second opening */
  if (sp_merkle_verify_paths(&leaves[0][0], &sib[0][0], off, 0, rows, 2, root, 1, verdict, status) != SP_OK) return 14;
  if (verdict[0] != SP_PATH_TRUE || verdict[1] != SP_PATH_FALSE) return 15;

  /* a refused call writes nothing; no openings is no error */
  const uint64_t rows_bad[2] = {3, ROWS};
  memset(val_off, 0xEE, sizeof(val_off));
  memset(leaves, 0xEE, sizeof(leaves));
  if (sp_commit_open(1, cols, stride, n_rows, n_cols, levels, 2, table_of, rows_bad, &values[0][0], val_off, &leaves[0][0],
                     &sib[0][0], off) != SP_ERR_BAD_ARGUMENT) return 16;
  if (strstr(sp_last_error(), "rows") == NULL) return 17;
  for (size_t i = 0; i < sizeof(val_off); ++i)
    if (((unsigned char*)val_off)[i] != 0xEE) return 18;
  for (size_t i = 0; i < sizeof(leaves); ++i)
    if (((unsigned char*)leaves)[i] != 0xEE) return 19;
  if (sp_commit_open(1, cols, stride, n_rows, n_cols, levels, 0, NULL, NULL, NULL, val_off, NULL, NULL, off) != SP_OK) return 20;
  if (val_off[0] != 0 || off[0] != 0) return 21;

  if (dev_free(d_cols) != 0 || dev_free(d_levels) != 0) return 22;
  sp_shutdown();
  printf("cabi_open ok\n");
  return 0;
}
