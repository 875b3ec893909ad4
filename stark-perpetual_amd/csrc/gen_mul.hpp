// The gathered fixed-base walk over the EC_GEN window table, shared by the ECDSA kernels (ecdsa.hip gen_mul, which
// chooses between it and the masked walk of masked_walk.hpp) and the public point arithmetic (ec_points.hip, which
// bypasses the masked table).  Device only: the table is the context's, in HBM.
#pragma once
#include "context.hpp"

namespace sp {

// k * EC_GEN from the window table of nwin windows of wbits > 0 bits; k < 2^252.  Infinity (only for k == 0 mod N)
// shows as ZZ == 0.
__device__ __forceinline__ xyzz gen_mul_gathered(u256 k, const aff_packed* __restrict__ gen, int wbits, int nwin) {
  const size_t per = (size_t)1 << wbits;
  const uint32_t mask = (1u << wbits) - 1u;
  auto pop = [&](void) {
    const uint32_t v = k.w[0] & mask;
#pragma unroll
    for (int i = 0; i < 7; ++i) k.w[i] = (k.w[i] >> wbits) | (k.w[i + 1] << (32 - wbits));
    k.w[7] >>= wbits;
    return v;
  };
  // the entry of window i + 1 is requested before window i is added: a lone wave per SIMD has nothing else to
  // hide a random 64-byte gather (tables of tens of GiB: a TLB miss on most of them) behind
  const aff e0 = ld_aff(gen + pop());
  aff nxt = nwin > 1 ? ld_aff(gen + per + pop()) : aff{};
  xyzz acc;
  int first = 1;
  if (nwin > 1) {  // windows 0 and 1 are both affine: mmadd (4M + 2S) instead of a mixed addition (8M + 2S)
    const aff q1 = nxt;
    if (2 < nwin) nxt = ld_aff(gen + (size_t)2 * per + pop());
    acc = xyzz_mmadd(e0, q1);
    first = 2;
  } else {
    acc = xyzz_from_aff(e0);
  }
  for (int i = first; i < nwin; ++i) {
    const aff q = nxt;
    if (i + 1 < nwin) nxt = ld_aff(gen + (size_t)(i + 1) * per + pop());
    acc = xyzz_madd(acc, q);
  }
  return acc;
}

}  // namespace sp
