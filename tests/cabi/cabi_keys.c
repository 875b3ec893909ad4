/* Plain-C consumer of sp_stark_key_y_batch and sp_felt_sqrt_batch (include/starkperp.h).  Built and run by
 * tests/test_gpu_stark_keys.py.  The y of EC_GEN's x (signature.py:56; its y is below p / 2, so it is the smaller root
 * itself), an x with no point on the curve, a felt that is not below p; validity bits alone; argument errors. */
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

#define SENTINEL 0xEEEEEEEEEEEEEEEEull

int main(void) {
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }
  const uint64_t gen_y[4] = {0x2873000c36e8dc1full, 0xde53ecd11abe43a3ull, 0xb7be4801df46ec62ull, 0x005668060aa49730ull};
  const uint64_t qx[3][4] = {
      {0x3d723d8bc943cfcaull, 0xdeacfd9b0d1819e0ull, 0x7beced415a40f0c7ull, 0x01ef15c18599971bull}, /* EC_GEN.x */
      {5, 0, 0, 0},                                                                              /* no such point */
      {1, 0, 0, 0x0800000000000011ull}};                                                         /* p itself */
  uint64_t qy[3][4];
  uint8_t st[3] = {77, 77, 77}, only[3] = {77, 77, 77};
  memset(qy, 0xEE, sizeof(qy));
  if (sp_stark_key_y_batch(&qx[0][0], &qy[0][0], st, 3) != SP_OK) {
    fprintf(stderr, "sp_stark_key_y_batch: %s\n", sp_last_error());
    return 3;
  }
  if (st[0] != SP_SQRT_OK || st[1] != SP_SQRT_NON_RESIDUE || st[2] != SP_SQRT_OUT_OF_RANGE) return 4;
  if (memcmp(qy[0], gen_y, 32) != 0) return 5;
  for (int i = 1; i < 3; ++i)
    for (int k = 0; k < 4; ++k)
      if (qy[i][k] != SENTINEL) return 6; /* outputs of items without a root are left as they were */
  if (sp_stark_key_y_batch(&qx[0][0], NULL, only, 3) != SP_OK || memcmp(only, st, 3) != 0) return 7;
  /* 4 = 2^2; 3 generates the whole group, so it is no square */
  const uint64_t a[2][4] = {{4, 0, 0, 0}, {3, 0, 0, 0}};
  uint64_t root[2][4];
  memset(root, 0xEE, sizeof(root));
  if (sp_felt_sqrt_batch(&a[0][0], &root[0][0], st, 2) != SP_OK) return 8;
  if (st[0] != SP_SQRT_OK || root[0][0] != 2 || root[0][1] || root[0][2] || root[0][3]) return 9;
  if (st[1] != SP_SQRT_NON_RESIDUE || root[1][0] != SENTINEL) return 10;
  /* argument errors write nothing; an empty batch is legal */
  st[0] = 77;
  if (sp_felt_sqrt_batch(&root[0][0], &root[0][0], st, 2) != SP_ERR_BAD_ARGUMENT) return 11;
  if (sp_felt_sqrt_batch(&a[0][0], &root[0][0], NULL, 2) != SP_ERR_BAD_ARGUMENT) return 12;
  if (sp_last_error()[0] == 0 || st[0] != 77) return 13;
  if (sp_stark_key_y_batch(NULL, NULL, NULL, 0) != SP_OK) return 14;
  sp_shutdown();
  printf("cabi_keys ok\n");
  return 0;
}
