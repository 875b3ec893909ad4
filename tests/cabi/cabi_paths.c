/* Plain-C consumer of the Merkle path calls of include/starkperp.h (sp_merkle_fold_paths, sp_merkle_verify_paths).
 * Built and run by tests/test_gpu_merkle_paths.py.  A height-8 tree after one update: sp_tree_prove's output goes to
 * sp_merkle_verify_paths as it comes (off = NULL, one shared root), every folded root is sp_tree_root; a changed
 * sibling, a changed key and a sibling equal to p are told apart per item; the ragged form with per-item roots; bad
 * arguments write nothing. */
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

#define HEIGHT 8
#define NKEYS 6

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  int tree = 0;
  uint64_t zero[4] = {0, 0, 0, 0}, root_old[4], root[4];
  uint8_t st = 0;
  if (sp_tree_create(HEIGHT, zero, &tree) != SP_OK) return 3;
  const uint64_t keys_a[4] = {2, 3, 200, 255};
  uint64_t leaves_a[4][4] = {{44, 0, 0, 0}, {11, 0, 0, 0}, {22, 5, 0, 0}, {33, 0, 0, 1}};
  if (sp_tree_update(tree, keys_a, &leaves_a[0][0], 4, root_old, root, &st) != SP_OK || st) return 4;

  /* proofs in any order, a repeat and a key never written */
  const uint64_t keys[NKEYS] = {200, 3, 100, 3, 2, 255};
  uint64_t leaves[NKEYS][4], sib[NKEYS][HEIGHT][4], roots[NKEYS][4];
  uint8_t verdict[NKEYS], status[NKEYS];
  if (sp_tree_prove(tree, keys, NKEYS, &leaves[0][0], &sib[0][0][0]) != SP_OK) return 5;
  if (sp_merkle_verify_paths(&leaves[0][0], &sib[0][0][0], NULL, HEIGHT, keys, NKEYS, root, 1, verdict, status) != SP_OK) {
    fprintf(stderr, "verify: %s\n", sp_last_error());
    return 6;
  }
  for (int i = 0; i < NKEYS; ++i)
    if (verdict[i] != SP_PATH_TRUE || status[i] != SP_HASH_OK) return 7;
  if (sp_merkle_fold_paths(&leaves[0][0], &sib[0][0][0], NULL, HEIGHT, keys, NKEYS, &roots[0][0], NULL) != SP_OK) return 8;
  for (int i = 0; i < NKEYS; ++i)
    if (memcmp(roots[i], root, 32) != 0) return 9;

  /* item 0: the neighbouring key (its leaf is the other child); item 1: a changed sibling; item 4: a sibling equal to p */
  const uint64_t p[4] = {1, 0, 0, 0x0800000000000011ull};
  uint64_t bad_keys[NKEYS];
  memcpy(bad_keys, keys, sizeof(keys));
  sib[1][4][0] ^= 1;
  bad_keys[0] ^= 1;
  memcpy(sib[4][7], p, 32);
  if (sp_merkle_verify_paths(&leaves[0][0], &sib[0][0][0], NULL, HEIGHT, bad_keys, NKEYS, root, 1, verdict, status) != SP_OK) return 10;
  for (int i = 0; i < NKEYS; ++i) {
    const int tampered = i == 0 || i == 1 || i == 4;
    if (verdict[i] != (tampered ? SP_PATH_FALSE : SP_PATH_TRUE)) return 11;
    if (status[i] != (i == 4 ? SP_HASH_OUT_OF_RANGE : SP_HASH_OK)) return 12;
  }
  sib[1][4][0] ^= 1;

  /* the ragged form: the first 8, 0 and 3 levels of three of the paths, each against its own root */
  uint64_t rsib[11][4], rleaves[3][4], want[3][4], part[3][4];
  const uint32_t off[4] = {0, 8, 8, 11};
  const uint64_t rkeys[3] = {200, 0, 3 & 7};
  memcpy(rsib[0], sib[0][0], 8 * 32);
  memcpy(rsib[8], sib[1][0], 3 * 32);
  memcpy(rleaves[0], leaves[0], 32);
  memcpy(rleaves[1], leaves[5], 32);
  memcpy(rleaves[2], leaves[1], 32);
  if (sp_merkle_fold_paths(&rleaves[0][0], &rsib[0][0], off, 0, rkeys, 3, &part[0][0], status) != SP_OK) return 13;
  if (status[0] || status[1] || status[2]) return 14;
  if (memcmp(part[0], root, 32) != 0 || memcmp(part[1], leaves[5], 32) != 0) return 15;
  /* the node three levels above leaf 3 is sibling 3 of key 8's path (8 >> 3 = 1 is the sibling of 3 >> 3 = 0) */
  const uint64_t k8[1] = {8};
  uint64_t l8[4], s8[HEIGHT][4];
  if (sp_tree_prove(tree, k8, 1, l8, &s8[0][0]) != SP_OK) return 16;
  if (memcmp(part[2], s8[3], 32) != 0) return 17;
  memcpy(want, part, sizeof(want));
  want[1][0] ^= 1;
  if (sp_merkle_verify_paths(&rleaves[0][0], &rsib[0][0], off, 0, rkeys, 3, &want[0][0], 3, verdict, NULL) != SP_OK) return 18;
  if (verdict[0] != SP_PATH_TRUE || verdict[1] != SP_PATH_FALSE || verdict[2] != SP_PATH_TRUE) return 19;

  /* bad arguments write nothing */
  const uint32_t off_bad[4] = {0, 8, 7, 11};
  const uint64_t keys_bad[3] = {200, 1, 3};
  memset(verdict, 0xEE, sizeof(verdict));
  if (sp_merkle_verify_paths(&rleaves[0][0], &rsib[0][0], off_bad, 0, rkeys, 3, &want[0][0], 3, verdict, NULL) != SP_ERR_BAD_ARGUMENT) return 20;
  if (sp_merkle_verify_paths(&rleaves[0][0], &rsib[0][0], off, 0, keys_bad, 3, &want[0][0], 3, verdict, NULL) != SP_ERR_BAD_ARGUMENT) return 21;
  if (sp_merkle_verify_paths(&rleaves[0][0], &rsib[0][0], off, 0, rkeys, 3, &want[0][0], 2, verdict, NULL) != SP_ERR_BAD_ARGUMENT) return 22;
  if (sp_last_error()[0] == 0) return 23;
  for (int i = 0; i < NKEYS; ++i)
    if (verdict[i] != 0xEE) return 24;
  if (sp_merkle_fold_paths(NULL, NULL, NULL, 65, NULL, 0, NULL, NULL) != SP_OK) return 25;
  if (sp_tree_destroy(tree) != SP_OK) return 26;
  sp_shutdown();
  printf("cabi_paths ok\n");
  return 0;
}
