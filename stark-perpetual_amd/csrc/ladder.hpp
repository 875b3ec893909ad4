// The variable-base ladder of the ECDSA verification (ecdsa.hip) and of the public point arithmetic (ec_points.hpp):
// regular signed recoding and the fixed signed 4-bit window ladder on a per-lane table of eight affine odd multiples.
// Host and device: the kernels run it with the table in HBM (one slot per lane, limb-major), the host tests with a
// plain array (n = 1, e = 0).
#pragma once
#include "curve.hpp"
#include "u256.hpp"

namespace sp {

// Regular signed recoding shared by the window ladder and the comb: for odd k,
//   k = sum_{j<256} (2 E_j - 1) 2^j   with   E = (k - 1)/2 + 2^255,
// so every 4-bit window of E is an odd digit 2e - 15 and every comb column has no zero row.
// Even scalars use N - k (odd) and the caller negates the result (`flip`).
SP_HD u256 recode_odd(const u256& u2, bool& flip) {
  flip = (u2.w[0] & 1u) == 0;
  u256 k = u2;
  if (flip) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t d = (uint64_t)U256_N.w[i] - u2.w[i] - borrow;
      k.w[i] = (uint32_t)d;
      borrow = (d >> 32) & 1u;
    }
  }
  u256 E;  // (k - 1) / 2 + 2^255   (k odd: k - 1 clears bit 0)
#pragma unroll
  for (int i = 0; i < 7; ++i) E.w[i] = (k.w[i] >> 1) | (k.w[i + 1] << 31);
  E.w[7] = (k.w[7] >> 1) | 0x80000000u;
  return E;
}

// B' = u2 * base on y^2 = x^3 + a_coef x + ...  Fixed signed window, w = 4, regular recoding:
// the digits d_i = 2 e_i - 15 (all odd, |d_i| <= 15) are read straight off the 4-bit windows e_i
// of E, and the top digit is always +1 - every lane does the same 252 doublings + 63 additions
// (no divergent branch; the binary ladder paid a mixed addition on every bit because some lane
// always needed one).  The eight odd multiples (2j+1)*base live in a per-signature table in HBM,
// limb-major (entry * 36 + limb) * n + e, and are made AFFINE before the ladder starts - one shared inversion
// of Z_1 ... Z_7 (Montgomery's trick, ~100 multiplication-equivalents) buys 63 mixed additions (7M + 4S)
// instead of 63 general ones (11M + 5S): -6 % of the ladder.  A zero among the Z's (a base point of order
// <= 15: impossible on the curve, prime order, and on its twist, no factor below 2 * 10^5) would poison the
// shared inversion; the product is tested and such a ladder returns the absorbing state Z = 0 (-> False).
//
// On a base point of order N the ladder's incomplete additions meet an exceptional case for exactly one odd
// scalar: the partial sum m before a window satisfies 0 < 16 m +- 15 < N + 31, and 16 m = +-d mod N with d odd
// leaves 16 m - d = N at the last window, d = -15 - the scalar N - 30 (and 30, which is recoded as N - 30), where the
// last addition would be a doubling and gives Z = 0.  The verifier answers False there; ec_points.hpp steps around it.
SP_HD jac ladder_mul(const u256& u2, const aff& base, const fe& a_coef,
                     int32_t* __restrict__ tab, size_t n, size_t e) {
  bool flip;
  u256 E = recode_odd(u2, flip);
  // planes of an entry: 0..8 X (then affine x), 9..17 Y (then affine y), 18..26 Z, 27..35 prefix product
  auto tab_at = [&](int entry, int limb) -> int32_t* { return tab + ((size_t)(entry * 36 + limb) * n + e); };
  auto tab_store = [&](int entry, int plane, const fe& v) {
#pragma unroll
    for (int l = 0; l < NL; ++l) *tab_at(entry, 9 * plane + l) = v.l[l];
  };
  auto tab_load = [&](int entry, int plane) {
    fe v;
#pragma unroll
    for (int l = 0; l < NL; ++l) v.l[l] = *tab_at(entry, 9 * plane + l);
    return v;
  };
  jac B;
  B.X = base.x; B.Y = base.y; B.Z = FE_ONE_M;
  {
    tab_store(0, 0, base.x);
    tab_store(0, 1, base.y);
    const jac twoQ = jac_dbl(B, a_coef);
    jac odd = jac_madd(twoQ, base);  // 3Q
    fe run = FE_ONE_M;
#pragma unroll 1
    for (int j = 1; j < 8; ++j) {
      if (j > 1) odd = jac_add(odd, twoQ);
      tab_store(j, 0, odd.X);
      tab_store(j, 1, odd.Y);
      tab_store(j, 2, odd.Z);
      tab_store(j, 3, run);
      run = fe_mul(run, odd.Z);
    }
    if (fe_is_zero(run)) {  // see above: unreachable for valid inputs, absorbing state otherwise
      B.Z = FE_ZERO;
      return B;
    }
    fe inv = fe_inv(run);
#pragma unroll 1
    for (int j = 7; j >= 1; --j) {
      const fe zinv = fe_mul(inv, tab_load(j, 3));
      inv = fe_mul(inv, tab_load(j, 2));
      const fe zi2 = fe_sqr(zinv);
      tab_store(j, 0, fe_mul(tab_load(j, 0), zi2));
      tab_store(j, 1, fe_mul(tab_load(j, 1), fe_mul(zi2, zinv)));
    }
  }
  // top window is e = 8  ->  digit +1: start from Q itself, then 63 windows
  {
#pragma unroll
    for (int i = 7; i > 0; --i) E.w[i] = (E.w[i] << 4) | (E.w[i - 1] >> 28);
    E.w[0] <<= 4;
  }
  // The loop body is kept to ONE doubling + ONE addition of code (~35 KB): with the four doublings unrolled the
  // body outgrows the 64 KB instruction cache and a lone wave per SIMD waits on instruction fetch.
#pragma unroll 1
  for (int wi = 0; wi < 63; ++wi) {
    const uint32_t ew = E.w[7] >> 28;
#pragma unroll
    for (int i = 7; i > 0; --i) E.w[i] = (E.w[i] << 4) | (E.w[i - 1] >> 28);
    E.w[0] <<= 4;
    const int d = 2 * (int)ew - 15;
    const int mag = (d < 0 ? -d : d) >> 1;  // table index of |d| = 2 mag + 1
    aff T;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      T.x.l[l] = *tab_at(mag, l);
      const int32_t y = *tab_at(mag, 9 + l);
      T.y.l[l] = d < 0 ? -y : y;
    }
    // four doublings in modified Jacobian form (W = a Z^4 carried along: 16M + 18S instead of 8M + 32S)
    mjac Bm = mjac_from(B, a_coef);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) mjac_dbl(Bm, k < 3);
    B.X = Bm.X; B.Y = Bm.Y; B.Z = Bm.Z;
    B = jac_madd(B, T);
  }
  if (flip) B.Y = fe_neg(B.Y);
  return B;
}

}  // namespace sp
