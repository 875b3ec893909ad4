/* Plain-C consumer of sp_ec_mult_batch, sp_ec_lincomb_batch and sp_ec_add_batch (include/starkperp.h).  Built and run
 * by tests/test_gpu_ec_points.py.  What needs a fresh process: the calls before sp_init.  Then 2 EC_GEN four ways
 * (2 G, G + G, G - (-G) through k = N - 1, 1 G + 1 G), the four statuses in one batch, x alone, argument errors. */
#include <stdio.h>
#include <string.h>
#include "../../include/starkperp.h"

#define SENTINEL 0xEEEEEEEEEEEEEEEEull
#define GX {0x3d723d8bc943cfcaull, 0xdeacfd9b0d1819e0ull, 0x7beced415a40f0c7ull, 0x01ef15c18599971bull}
#define GY {0x2873000c36e8dc1full, 0xde53ecd11abe43a3ull, 0xb7be4801df46ec62ull, 0x005668060aa49730ull}

static int untouched(const uint64_t* v) { return v[0] == SENTINEL && v[1] == SENTINEL && v[2] == SENTINEL && v[3] == SENTINEL; }

int main(void) {
  const uint64_t two_x[4] = {0x4c5416f439403cf5ull, 0xbf40959283187c65ull, 0xd535a81e83039658ull, 0x0759ca09377679ecull};
  const uint64_t two_y[4] = {0x93b562d7a9646c41ull, 0xe7455aa88778b19full, 0xd5c01a28598ad272ull, 0x06f524a3400e7708ull};
  /* items: 2 G (OK), 0 G (INFINITY), N G (OUT_OF_RANGE), 2 (Gx, Gy + 1) (NOT_ON_CURVE) */
  const uint64_t k[4][4] = {{2, 0, 0, 0}, {0, 0, 0, 0},
                            {0x1e66a241adc64d2full, 0xb781126dcae7b232ull, 0xffffffffffffffffull, 0x0800000000000010ull},
                            {2, 0, 0, 0}};
  const uint64_t px[4][4] = {GX, GX, GX, GX};
  const uint64_t py[4][4] = {GY, GY, GY,
                             {0x2873000c36e8dc20ull, 0xde53ecd11abe43a3ull, 0xb7be4801df46ec62ull, 0x005668060aa49730ull}};
  const uint64_t one[4][4] = {{1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 0, 0}};
  const uint64_t n_minus_1[4] = {0x1e66a241adc64d2eull, 0xb781126dcae7b232ull, 0xffffffffffffffffull, 0x0800000000000010ull};
  uint64_t rx[4][4], ry[4][4], nx[4], ny[4];
  uint8_t st[4] = {77, 77, 77, 77};
  memset(rx, 0xEE, sizeof(rx));
  memset(ry, 0xEE, sizeof(ry));
  /* before sp_init: no CPU fallback, nothing written */
  if (sp_ec_mult_batch(&k[0][0], &px[0][0], &py[0][0], &rx[0][0], &ry[0][0], st, 4) != SP_ERR_NOT_INITIALISED) return 20;
  if (sp_ec_lincomb_batch(&k[0][0], &k[0][0], &px[0][0], &py[0][0], &rx[0][0], &ry[0][0], st, 4) != SP_ERR_NOT_INITIALISED) return 21;
  if (sp_ec_add_batch(&px[0][0], &py[0][0], &px[0][0], &py[0][0], 0, &rx[0][0], &ry[0][0], st, 4) != SP_ERR_NOT_INITIALISED) return 22;
  if (st[0] != 77 || !untouched(rx[0])) return 23;
  if (sp_init(0, 0) != SP_OK) { fprintf(stderr, "sp_init: %s\n", sp_last_error()); return 2; }

  if (sp_ec_mult_batch(&k[0][0], &px[0][0], &py[0][0], &rx[0][0], &ry[0][0], st, 4) != SP_OK) {
    fprintf(stderr, "sp_ec_mult_batch: %s\n", sp_last_error());
    return 3;
  }
  if (st[0] != SP_EC_OK || st[1] != SP_EC_INFINITY || st[2] != SP_EC_OUT_OF_RANGE || st[3] != SP_EC_NOT_ON_CURVE) return 4;
  if (memcmp(rx[0], two_x, 32) != 0 || memcmp(ry[0], two_y, 32) != 0) return 5;
  for (int i = 1; i < 4; ++i)
    if (!untouched(rx[i]) || !untouched(ry[i])) return 6; /* outputs of items that are not OK are left as they were */

  /* G + G, G - G */
  memset(rx, 0xEE, sizeof(rx));
  memset(ry, 0xEE, sizeof(ry));
  if (sp_ec_add_batch(&px[0][0], &py[0][0], &px[0][0], &py[0][0], 0, &rx[0][0], &ry[0][0], st, 1) != SP_OK) return 7;
  if (st[0] != SP_EC_OK || memcmp(rx[0], two_x, 32) != 0 || memcmp(ry[0], two_y, 32) != 0) return 8;
  if (sp_ec_add_batch(&px[0][0], &py[0][0], &px[0][0], &py[0][0], 1, &rx[1][0], &ry[1][0], st, 1) != SP_OK) return 9;
  if (st[0] != SP_EC_INFINITY || !untouched(rx[1])) return 10;
  /* -G = (N - 1) G, then G - (-G) with x alone */
  if (sp_ec_mult_batch(n_minus_1, &px[0][0], &py[0][0], nx, ny, st, 1) != SP_OK || st[0] != SP_EC_OK) return 11;
  if (memcmp(nx, px[0], 32) != 0 || memcmp(ny, py[0], 32) == 0) return 12;
  memset(rx, 0xEE, sizeof(rx));
  if (sp_ec_add_batch(&px[0][0], &py[0][0], nx, ny, 1, &rx[0][0], NULL, st, 1) != SP_OK) return 13;
  if (st[0] != SP_EC_OK || memcmp(rx[0], two_x, 32) != 0) return 14;
  /* 1 G + 1 G: the sum is a doubling; 1 G + (N - 1) G: infinity */
  memset(rx, 0xEE, sizeof(rx));
  memset(ry, 0xEE, sizeof(ry));
  if (sp_ec_lincomb_batch(&one[0][0], &one[0][0], &px[0][0], &py[0][0], &rx[0][0], &ry[0][0], st, 1) != SP_OK) return 15;
  if (st[0] != SP_EC_OK || memcmp(rx[0], two_x, 32) != 0 || memcmp(ry[0], two_y, 32) != 0) return 16;
  if (sp_ec_lincomb_batch(&one[0][0], n_minus_1, &px[0][0], &py[0][0], &rx[1][0], &ry[1][0], st, 1) != SP_OK) return 17;
  if (st[0] != SP_EC_INFINITY || !untouched(rx[1]) || !untouched(ry[1])) return 18;

  /* argument errors write nothing; an empty batch is legal */
  st[0] = 77;
  memcpy(rx[0], k[0], 32);
  if (sp_ec_mult_batch(&rx[0][0], &px[0][0], &py[0][0], &rx[0][0], &ry[0][0], st, 1) != SP_ERR_BAD_ARGUMENT) return 30;
  if (sp_ec_mult_batch(&k[0][0], &px[0][0], &py[0][0], NULL, &ry[0][0], st, 1) != SP_ERR_BAD_ARGUMENT) return 31;
  if (sp_ec_add_batch(&px[0][0], &py[0][0], &px[0][0], &py[0][0], 0, &rx[0][0], &ry[0][0], NULL, 1) != SP_ERR_BAD_ARGUMENT) return 32;
  if (sp_last_error()[0] == 0 || st[0] != 77 || memcmp(rx[0], k[0], 32) != 0) return 33;
  if (sp_ec_lincomb_batch(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != SP_OK) return 34;
  sp_shutdown();
  printf("cabi_points ok\n");
  return 0;
}
