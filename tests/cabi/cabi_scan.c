/* Plain-C consumer of sp_tree_scan (include/starkperp.h).  Built and run by tests/test_gpu_tree_scan.py, which compares
 * the printed lines.  A height-64 tree after one update of 5 keys, both ends of the key range among them: pages of 2
 * until `more` is 0, resuming behind the last key of each page; then bad arguments, which write nothing. */
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  int tree = 0;
  uint64_t zero[4] = {0, 0, 0, 0}, root_old[4], root[4];
  uint8_t st = 0;
  if (sp_tree_create(64, zero, &tree) != SP_OK) return 3;
  uint64_t keys[2], leaves[2][4];
  size_t n = 77;
  int more = 77;
  /* a tree never updated: empty, no launch */
  if (sp_tree_scan(tree, 0, UINT64_MAX, 2, keys, &leaves[0][0], &n, &more) != SP_OK || n != 0 || more != 0) return 4;
  const uint64_t written[5] = {0, 7, 0x8000000000000000ull, 0x8000000000000001ull, UINT64_MAX};
  uint64_t values[5][4] = {{11, 0, 0, 0}, {22, 0, 0, 0}, {33, 5, 0, 0}, {44, 0, 0, 1}, {55, 0, 0, 0}};
  if (sp_tree_update(tree, written, &values[0][0], 5, root_old, root, &st) != SP_OK || st) return 5;
  uint64_t lo = 0;
  int pages = 0;
  do {
    if (sp_tree_scan(tree, lo, UINT64_MAX, 2, keys, &leaves[0][0], &n, &more) != SP_OK) {
      fprintf(stderr, "scan: %s\n", sp_last_error());
      return 6;
    }
    if (n == 0 || n > 2) return 7;
    for (size_t i = 0; i < n; ++i) printf("key %" PRIu64 " leaf %" PRIu64 " %" PRIu64 "\n", keys[i], leaves[i][0], leaves[i][3]);
    printf("page %d n %zu more %d\n", pages, n, more);
    lo = keys[n - 1] + 1;
    if (++pages > 5) return 8;
  } while (more);
  /* bad arguments write nothing */
  memset(keys, 0xEE, sizeof(keys));
  n = 77;
  more = 77;
  if (sp_tree_scan(tree, 5, 4, 2, keys, &leaves[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 9;
  if (sp_tree_scan(tree, 0, 4, 0, keys, &leaves[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 10;
  if (sp_tree_scan(tree, 0, 4, 2, NULL, &leaves[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 11;
  if (sp_tree_scan(tree + 1000, 0, 4, 2, keys, &leaves[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 12;
  if (sp_last_error()[0] == 0) return 13;
  if (n != 77 || more != 77 || keys[0] != 0xEEEEEEEEEEEEEEEEull || keys[1] != 0xEEEEEEEEEEEEEEEEull) return 14;
  if (sp_tree_destroy(tree) != SP_OK) return 15;
  sp_shutdown();
  printf("cabi_scan ok\n");
  return 0;
}
