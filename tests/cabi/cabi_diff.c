/* Plain-C consumer of sp_tree_clone and sp_tree_diff (include/starkperp.h).  Built and run by tests/test_gpu_tree_diff.py,
 * which compares the printed lines.  A height-64 tree of 5 keys is cloned, the clone is updated (two leaves rewritten, one
 * set back to the empty leaf, one new key, one key left alone), and the diff is paged with capacity 2 until `more` is 0,
 * resuming behind the last key of each page; then bad arguments, which write nothing; then the source is destroyed and
 * the clone lives on. */
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  int tree = 0, clone = 0;
  uint64_t zero[4] = {0, 0, 0, 0}, root_old[4], root[4], root_clone[4];
  uint8_t st = 0;
  if (sp_tree_create(64, zero, &tree) != SP_OK) return 3;
  const uint64_t written[5] = {0, 7, 0x8000000000000000ull, 0x8000000000000001ull, UINT64_MAX};
  uint64_t values[5][4] = {{11, 0, 0, 0}, {22, 0, 0, 0}, {33, 5, 0, 0}, {44, 0, 0, 1}, {55, 0, 0, 0}};
  if (sp_tree_update(tree, written, &values[0][0], 5, root_old, root, &st) != SP_OK || st) return 4;
  if (sp_tree_clone(tree, &clone) != SP_OK || clone == tree) { fprintf(stderr, "clone: %s\n", sp_last_error()); return 5; }
  if (sp_tree_root(clone, root_clone) != SP_OK || memcmp(root, root_clone, 32) != 0) return 6;
  uint64_t keys[2], a[2][4], b[2][4];
  size_t n = 77;
  int more = 77;
  /* equal roots: empty, no launch */
  if (sp_tree_diff(tree, clone, 0, UINT64_MAX, 2, keys, &a[0][0], &b[0][0], &n, &more) != SP_OK || n != 0 || more != 0) return 7;
  const uint64_t touched[5] = {0, 8, 0x8000000000000000ull, 0x8000000000000001ull, UINT64_MAX};
  uint64_t fresh[5][4] = {{12, 0, 0, 0}, {66, 0, 0, 2}, {0, 0, 0, 0}, {45, 0, 0, 1}, {56, 0, 0, 0}};
  if (sp_tree_update(clone, touched, &fresh[0][0], 5, root_old, root_clone, &st) != SP_OK || st) return 8;
  if (sp_tree_root(tree, root_old) != SP_OK || memcmp(root, root_old, 32) != 0) return 9; /* the source stands */
  uint64_t lo = 0;
  int pages = 0;
  do {
    if (sp_tree_diff(tree, clone, lo, UINT64_MAX, 2, keys, &a[0][0], &b[0][0], &n, &more) != SP_OK) {
      fprintf(stderr, "diff: %s\n", sp_last_error());
      return 10;
    }
    if (n == 0 || n > 2) return 11;
    for (size_t i = 0; i < n; ++i)
      printf("key %" PRIu64 " a %" PRIu64 " %" PRIu64 " b %" PRIu64 " %" PRIu64 "\n", keys[i], a[i][0], a[i][3], b[i][0], b[i][3]);
    printf("page %d n %zu more %d\n", pages, n, more);
    lo = keys[n - 1] + 1;
    if (++pages > 5) return 12;
  } while (more);
  /* bad arguments write nothing */
  memset(keys, 0xEE, sizeof(keys));
  n = 77;
  more = 77;
  if (sp_tree_diff(tree, clone, 5, 4, 2, keys, &a[0][0], &b[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 13;
  if (sp_tree_diff(tree, clone, 0, 4, 0, keys, &a[0][0], &b[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 14;
  if (sp_tree_diff(tree, clone, 0, 4, 2, NULL, &a[0][0], &b[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 15;
  if (sp_tree_diff(tree, tree, 0, 4, 2, keys, &a[0][0], &b[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 16;
  if (sp_tree_diff(tree, clone + 1000, 0, 4, 2, keys, &a[0][0], &b[0][0], &n, &more) != SP_ERR_BAD_ARGUMENT) return 17;
  if (sp_tree_clone(tree, NULL) != SP_ERR_BAD_ARGUMENT || sp_tree_clone(tree + 1000, &clone) != SP_ERR_BAD_ARGUMENT) return 18;
  if (sp_last_error()[0] == 0) return 19;
  if (n != 77 || more != 77 || keys[0] != 0xEEEEEEEEEEEEEEEEull || keys[1] != 0xEEEEEEEEEEEEEEEEull) return 20;
  /* the clone outlives its source */
  if (sp_tree_destroy(tree) != SP_OK) return 21;
  if (sp_tree_root(clone, root) != SP_OK || memcmp(root, root_clone, 32) != 0) return 22;
  if (sp_tree_destroy(clone) != SP_OK) return 23;
  sp_shutdown();
  printf("cabi_diff ok\n");
  return 0;
}
