/* Plain-C consumer of the witness export of include/starkperp.h (sp_tree_witness_size, sp_tree_witness,
 * sp_tree_prove).  Built and run by tests/test_gpu_tree_witness.py.  A height-8 tree after two updates:
 * size -> witness -> prove; the last record is the root; every record hashes (sp_pedersen_batch over all records);
 * every proof folds to the root, level by level through sp_pedersen_batch. */
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

#define HEIGHT 8
#define NKEYS 5
#define MAXREC (NKEYS * HEIGHT)

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  int tree = 0;
  uint64_t zero[4] = {0, 0, 0, 0}, root_old[4], root_new[4], root[4];
  uint8_t st = 0;
  if (sp_tree_create(HEIGHT, zero, &tree) != SP_OK) return 3;
  /* two updates: keys 3, 200, 255, then 2 (the sibling of 3) and 200 again */
  const uint64_t keys_a[3] = {3, 200, 255}, keys_b[2] = {2, 200};
  uint64_t leaves_a[3][4] = {{11, 0, 0, 0}, {22, 5, 0, 0}, {33, 0, 0, 1}}, leaves_b[2][4] = {{44, 0, 0, 0}, {55, 0, 7, 0}};
  if (sp_tree_update(tree, keys_a, &leaves_a[0][0], 3, root_old, root_new, &st) != SP_OK || st) return 4;
  if (sp_tree_update(tree, keys_b, &leaves_b[0][0], 2, root_old, root_new, &st) != SP_OK || st) return 5;
  if (sp_tree_root(tree, root) != SP_OK || memcmp(root, root_new, 32) != 0) return 6;

  /* witness of two written keys, their neighbourhood and a key never written */
  const uint64_t keys[NKEYS] = {2, 3, 100, 200, 254};
  size_t want = 0, got = 0;
  if (sp_tree_witness_size(HEIGHT, keys, NKEYS, &want) != SP_OK || want == 0 || want > MAXREC) return 7;
  uint8_t level[MAXREC];
  uint64_t index[MAXREC], node[MAXREC][4], left[MAXREC][4], right[MAXREC][4], hashed[MAXREC][4];
  uint8_t status[MAXREC];
  if (sp_tree_witness(tree, keys, NKEYS, want - 1, level, index, &node[0][0], &left[0][0], &right[0][0], &got)
      != SP_ERR_BAD_ARGUMENT || got != want) return 8;
  got = 0;
  if (sp_tree_witness(tree, keys, NKEYS, want, level, index, &node[0][0], &left[0][0], &right[0][0], &got) != SP_OK
      || got != want) return 9;
  if (level[want - 1] != HEIGHT || index[want - 1] != 0 || memcmp(node[want - 1], root, 32) != 0) return 10;
  if (level[0] != 1 || index[0] != 1) return 11; /* keys 2 and 3 share their parent */
  for (size_t u = 1; u < want; ++u)
    if (level[u] < level[u - 1] || (level[u] == level[u - 1] && index[u] <= index[u - 1])) return 12;
  if (sp_pedersen_batch(&left[0][0], &right[0][0], &hashed[0][0], status, want) != SP_OK) return 13;
  for (size_t u = 0; u < want; ++u)
    if (status[u] || memcmp(hashed[u], node[u], 32) != 0) return 14;
  if (memcmp(left[0], leaves_b[0], 32) != 0 || memcmp(right[0], leaves_a[0], 32) != 0) return 15;

  /* proofs, any order and a repeat: fold all of them one level per sp_pedersen_batch call */
  const uint64_t pkeys[NKEYS] = {200, 3, 100, 3, 2};
  uint64_t pleaves[NKEYS][4], sib[NKEYS][HEIGHT][4], x[NKEYS][4], y[NKEYS][4], acc[NKEYS][4];
  if (sp_tree_prove(tree, pkeys, NKEYS, &pleaves[0][0], &sib[0][0][0]) != SP_OK) return 16;
  if (memcmp(pleaves[0], leaves_b[1], 32) != 0 || memcmp(pleaves[1], leaves_a[0], 32) != 0
      || memcmp(pleaves[2], zero, 32) != 0 || memcmp(pleaves[3], leaves_a[0], 32) != 0
      || memcmp(pleaves[4], leaves_b[0], 32) != 0) return 17;
  memcpy(acc, pleaves, sizeof(acc));
  for (int l = 0; l < HEIGHT; ++l) {
    for (int i = 0; i < NKEYS; ++i) {
      const int bit = (int)((pkeys[i] >> l) & 1);
      memcpy(x[i], bit ? sib[i][l] : acc[i], 32);
      memcpy(y[i], bit ? acc[i] : sib[i][l], 32);
    }
    if (sp_pedersen_batch(&x[0][0], &y[0][0], &acc[0][0], status, NKEYS) != SP_OK) return 18;
    for (int i = 0; i < NKEYS; ++i)
      if (status[i]) return 19;
  }
  for (int i = 0; i < NKEYS; ++i)
    if (memcmp(acc[i], root, 32) != 0) return 20;

  /* bad arguments leave the tree alone */
  const uint64_t unsorted[2] = {9, 4}, outside[1] = {256};
  if (sp_tree_witness(tree, unsorted, 2, MAXREC, level, index, &node[0][0], &left[0][0], &right[0][0], &got)
      != SP_ERR_BAD_ARGUMENT) return 21;
  if (sp_tree_prove(tree, outside, 1, &pleaves[0][0], &sib[0][0][0]) != SP_ERR_BAD_ARGUMENT) return 22;
  if (sp_tree_root(tree, root_old) != SP_OK || memcmp(root_old, root, 32) != 0) return 23;
  if (sp_tree_destroy(tree) != SP_OK) return 24;
  if (sp_tree_prove(tree, pkeys, NKEYS, &pleaves[0][0], &sib[0][0][0]) != SP_ERR_BAD_ARGUMENT) return 25;
  sp_shutdown();
  printf("cabi_witness ok\n");
  return 0;
}
