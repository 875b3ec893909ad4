// One item of the public point arithmetic on the Stark curve (ec_points.hip): R = k P, R = a EC_GEN + b P, R = P +- Q
// (ec_mult / ec_add / ec_double of math_utils.py:59-100, on the one curve the device knows).  Host and device: the
// kernels run it one item per lane, tests/host/ec_points_shim.cpp runs the same code under g++ with the bound checks on.
//
// The variable-base multiple is ladder.hpp's ladder_mul, the code the verifier runs.  Its additions are incomplete by
// design - verification may answer False where they break down - so everything after the ladder goes through
// ec_add_complete, which owns infinity on either side, equal operands (the doubling) and opposite operands (infinity),
// and the one scalar pair at which the ladder itself meets its own operand (30 and N - 30, ladder.hpp) is stepped
// around: the ladder runs on 29 resp. N - 29 and +-P is added afterwards.  A ladder that still ends in its absorbing
// state Z = 0 is reported as SP_EC_INFINITY, never as a point.
#pragma once
#include "../../include/starkperp.h"
#include "curve_consts.hpp"
#include "ladder.hpp"

namespace sp {

constexpr xyzz XYZZ_INFINITY = {FE_ZERO, FE_ZERO, FE_ZERO, FE_ZERO};

SP_HD bool u256_eq(const u256& a, const u256& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.w[i] ^ b.w[i];
  return o == 0;
}

// ---- the checks: range of everything first, then the curve ----
SP_HD aff ec_point_of(const u256& x, const u256& y) {  // both in [0, p)
  aff P;
  P.x = fe_to_mont(fe_unpack(x));
  P.y = fe_to_mont(fe_unpack(y));
  return P;
}
SP_HD bool ec_on_curve(const aff& P) {  // y^2 == x^3 + x + beta
  const fe rhs = fe_carry(fe_add(fe_add(fe_mul(fe_sqr(P.x), P.x), P.x), fe_to_mont(fe_unpack(CURVE_BETA))));
  return fe_eq(fe_sqr(P.y), rhs);
}
SP_HD aff ec_neg(const aff& P) {
  aff R;
  R.x = P.x;
  R.y = fe_carry(fe_neg(P.y));
  return R;
}

// ---- the complete finish ----
SP_HD xyzz xyzz_from_jac(const jac& p) {  // Z == 0 (the ladder's absorbing state) becomes ZZ == 0
  xyzz r;
  r.X = p.X;
  r.Y = p.Y;
  r.ZZ = fe_sqr(p.Z);
  r.ZZZ = fe_mul(r.ZZ, p.Z);
  return r;
}

// 2 a on y^2 = x^3 + x + beta ("dbl-2008-s-1" with a = 1, 6M + 4S).  y = 0 gives ZZ = 0; no such point exists here
// (odd group order).  Rare path: every sum is carried before it is multiplied.
SP_HD xyzz xyzz_dbl(const xyzz& a) {
  const fe U = fe_carry(fe_dbl(a.Y));
  const fe V = fe_sqr(U);
  const fe W = fe_mul(U, V);
  const fe S = fe_mul(a.X, V);
  const fe XX = fe_sqr(a.X);
  const fe M = fe_carry(fe_add(fe_carry(fe_add(fe_dbl(XX), XX)), fe_sqr(a.ZZ)));
  xyzz r;
  r.X = fe_carry(fe_sub(fe_sqr(M), fe_dbl(S)));
  r.Y = fe_carry(fe_sub(fe_mul(M, fe_carry(fe_sub(S, r.X))), fe_mul(W, fe_carry(a.Y))));
  r.ZZ = fe_mul(V, a.ZZ);
  r.ZZZ = fe_mul(W, a.ZZZ);
  return r;
}

// a + b for every pair of group elements, infinity (ZZ == 0) included on either side and as the result.
SP_HD xyzz ec_add_complete(const xyzz& a, const xyzz& b) {
  if (fe_is_zero(a.ZZ)) return fe_is_zero(b.ZZ) ? XYZZ_INFINITY : b;
  if (fe_is_zero(b.ZZ)) return a;
  // x equal <=> X_a ZZ_b == X_b ZZ_a;  y equal <=> Y_a ZZZ_b == Y_b ZZZ_a
  if (fe_eq(fe_mul(a.X, b.ZZ), fe_mul(b.X, a.ZZ))) {
    if (fe_eq(fe_mul(a.Y, b.ZZZ), fe_mul(b.Y, a.ZZZ))) return xyzz_dbl(a);
    return XYZZ_INFINITY;  // b == -a
  }
  return xyzz_add(a, b);
}

// Affine (x, y) of r as plain integers in [0, p): one field inversion (variable-time: the data is public).
SP_HD uint8_t ec_affine_out(const xyzz& r, u256& rx, u256& ry) {
  if (fe_is_zero(r.ZZ)) return SP_EC_INFINITY;
  const fe izzz = fe_inv(r.ZZZ);
  rx = fe_pack(fe_from_mont(fe_mul(r.X, fe_sqr(fe_mul(r.ZZ, izzz)))));
  ry = fe_pack(fe_from_mont(fe_mul(r.Y, izzz)));
  return SP_EC_OK;
}

// ---- the variable-base multiple: k in (0, N) ----
// ladder_mul breaks down at exactly k = 30 and k = N - 30 (ladder.hpp): those two run the ladder on 29 resp. N - 29
// and leave `corr` = +1 resp. -1, the multiple of the base the caller still has to add.
constexpr u256 U256_30 = {{30u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
constexpr u256 U256_29 = {{29u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
constexpr u256 U256_N_MINUS_30 = {{0xadc64d11u, 0x1e66a241u, 0xcae7b232u, 0xb781126du, 0xffffffffu, 0xffffffffu,
                                   0x10u, 0x08000000u}};
constexpr u256 U256_N_MINUS_29 = {{0xadc64d12u, 0x1e66a241u, 0xcae7b232u, 0xb781126du, 0xffffffffu, 0xffffffffu,
                                   0x10u, 0x08000000u}};
SP_HD xyzz ec_var_mul(const u256& k, const aff& P, int32_t* __restrict__ tab, size_t n, size_t e) {
  u256 k2 = k;
  int corr = 0;
  if (u256_eq(k, U256_30)) { k2 = U256_29; corr = 1; }
  if (u256_eq(k, U256_N_MINUS_30)) { k2 = U256_N_MINUS_29; corr = -1; }
  const xyzz B = xyzz_from_jac(ladder_mul(k2, P, FE_ONE_M, tab, n, e));
  if (corr == 0) return B;
  return ec_add_complete(B, xyzz_from_aff(corr > 0 ? P : ec_neg(P)));
}

// ---- the three items.  rx / ry are written only for SP_EC_OK; `tab`, n, e: the ladder's table slot (ladder.hpp) ----
SP_HD uint8_t ec_mult_item(const u256& k, const u256& px, const u256& py, int32_t* __restrict__ tab, size_t n,
                           size_t e, u256& rx, u256& ry) {
  if (!u256_lt(k, U256_N) || !u256_lt(px, U256_P) || !u256_lt(py, U256_P)) return SP_EC_OUT_OF_RANGE;
  const aff P = ec_point_of(px, py);
  if (!ec_on_curve(P)) return SP_EC_NOT_ON_CURVE;
  if (u256_is_zero(k)) return SP_EC_INFINITY;
  return ec_affine_out(ec_var_mul(k, P, tab, n, e), rx, ry);
}

// gen_mul_of(a) = a EC_GEN as xyzz for a in (0, N): the kernel walks the context's window table (gen_mul.hpp), the
// host shim uses the affine group law of hostcurve.hpp.
template <class GenMul>
SP_HD uint8_t ec_lincomb_item(const u256& a, const u256& b, const u256& px, const u256& py, GenMul&& gen_mul_of,
                              int32_t* __restrict__ tab, size_t n, size_t e, u256& rx, u256& ry) {
  if (!u256_lt(a, U256_N) || !u256_lt(b, U256_N) || !u256_lt(px, U256_P) || !u256_lt(py, U256_P))
    return SP_EC_OUT_OF_RANGE;
  const aff P = ec_point_of(px, py);
  if (!ec_on_curve(P)) return SP_EC_NOT_ON_CURVE;
  xyzz R = XYZZ_INFINITY;  // a zero term drops out
  if (!u256_is_zero(a)) R = gen_mul_of(a);
  if (!u256_is_zero(b)) R = ec_add_complete(R, ec_var_mul(b, P, tab, n, e));
  return ec_affine_out(R, rx, ry);
}

SP_HD uint8_t ec_add_item(const u256& px, const u256& py, const u256& qx, const u256& qy, bool subtract, u256& rx,
                          u256& ry) {
  if (!u256_lt(px, U256_P) || !u256_lt(py, U256_P) || !u256_lt(qx, U256_P) || !u256_lt(qy, U256_P))
    return SP_EC_OUT_OF_RANGE;
  const aff P = ec_point_of(px, py);
  aff Q = ec_point_of(qx, qy);
  if (!ec_on_curve(P) || !ec_on_curve(Q)) return SP_EC_NOT_ON_CURVE;
  if (subtract) Q = ec_neg(Q);
  return ec_affine_out(ec_add_complete(xyzz_from_aff(P), xyzz_from_aff(Q)), rx, ry);
}

}  // namespace sp
