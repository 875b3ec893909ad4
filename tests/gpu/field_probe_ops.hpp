// Op table of tests/gpu/field_probe.hip: one function per lane-private operation of csrc/fp29.hpp and
// csrc/curve.hpp, on raw limbs (9 x int32 per element) so that a test chooses the exact N-form representative.
// Every op reads KIN elements and writes KOUT elements and NFLAG int32 flags per item.  The same table compiles
// with hipcc into the device probe and with g++ -DSP_CHECK_BOUNDS into its host twin (tests/host/field_probe_twin.cpp):
// the twin carries the host bound checks over to the inputs the device build is run on.
// Test infrastructure only - never loaded by the product.
#pragma once
#include "curve.hpp"
#include "curve_consts.hpp"

namespace probe {
using namespace sp;

#define PROBE_OP(name, kin, kout, nflag)                  \
  struct op_##name {                                      \
    static constexpr int KIN = kin, KOUT = kout, NFLAG = nflag; \
    static SP_HD void run(const fe* v, fe* o, int32_t* f); \
  };                                                      \
  SP_HD void op_##name::run(const fe* v, fe* o, int32_t* f)
#define PROBE_UNUSED (void)v, (void)o, (void)f

// ---- a. pack / unpack: the eight 32-bit words travel in limbs 0..7 of one element ----
SP_HD u256 words_of(const fe& a) {
  u256 u;
  for (int k = 0; k < 8; ++k) u.w[k] = (uint32_t)a.l[k];
  return u;
}
PROBE_OP(unpack, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_unpack(words_of(v[0])); }
PROBE_OP(pack_unpack, 1, 1, 0) {
  PROBE_UNUSED;
  const u256 r = fe_pack(fe_unpack(words_of(v[0])));
  for (int k = 0; k < 8; ++k) o[0].l[k] = (int32_t)r.w[k];
  o[0].l[8] = 0;
}

// ---- b. multiplications: column form, scan form of each, all from one 6-tuple ----
PROBE_OP(mul_forms, 6, 10, 0) {
  PROBE_UNUSED;
  o[0] = fe_mul(v[0], v[1]);
  o[1] = fe_mul_scan(v[0], v[1]);
  o[2] = fe_sqr(v[0]);
  o[3] = fe_sqr_scan(v[0]);
  o[4] = fe_mul_sub_mul(v[0], v[1], v[2], v[3]);
  o[5] = fe_mul_sub_mul_scan(v[0], v[1], v[2], v[3]);
  o[6] = fe_mul_add_mul(v[0], v[1], v[2], v[3]);
  o[7] = fe_mul_add_mul_scan(v[0], v[1], v[2], v[3]);
  o[8] = fe_mul3_add(v[0], v[1], v[2], v[3], v[4], v[5]);
  o[9] = fe_mul3_add_scan(v[0], v[1], v[2], v[3], v[4], v[5]);
}

// ---- c. small ops ----
PROBE_OP(carry, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_carry(v[0]); }
PROBE_OP(canon, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_canon(v[0]); }
PROBE_OP(half, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_half(v[0]); }
PROBE_OP(to_mont, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_to_mont(v[0]); }
PROBE_OP(from_mont, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_from_mont(v[0]); }
PROBE_OP(is_zero, 1, 0, 1) { PROBE_UNUSED; f[0] = fe_is_zero(v[0]); }
PROBE_OP(eq, 2, 0, 1) { PROBE_UNUSED; f[0] = fe_eq(v[0], v[1]); }
PROBE_OP(is_qr, 1, 0, 1) { PROBE_UNUSED; f[0] = fe_is_qr(v[0]); }

// ---- d. group law: column form then scan form; the flags are fe_is_zero(ZZ3) of each, taken here ----
SP_HD void put(fe* o, const xyzz& r) { o[0] = r.X; o[1] = r.Y; o[2] = r.ZZ; o[3] = r.ZZZ; }
PROBE_OP(xyzz_madd, 6, 8, 2) {  // X Y ZZ ZZZ | qx qy
  const xyzz a{v[0], v[1], v[2], v[3]};
  const aff q{v[4], v[5]};
  put(o, xyzz_madd<false>(a, q));
  put(o + 4, xyzz_madd<true>(a, q));
  f[0] = fe_is_zero(o[2]);
  f[1] = fe_is_zero(o[6]);
}
PROBE_OP(xyzz_madd_x_only, 6, 4, 2) {  // -> X3 ZZ3 | X3 ZZ3
  const xyzz a{v[0], v[1], v[2], v[3]};
  const aff q{v[4], v[5]};
  xyzz_madd_x_only<false>(a, q, o[0], o[1]);
  xyzz_madd_x_only<true>(a, q, o[2], o[3]);
  f[0] = fe_is_zero(o[1]);
  f[1] = fe_is_zero(o[3]);
}
PROBE_OP(xyzz_mmadd, 4, 8, 2) {  // ax ay | bx by
  const aff a{v[0], v[1]}, b{v[2], v[3]};
  put(o, xyzz_mmadd<false>(a, b));
  put(o + 4, xyzz_mmadd<true>(a, b));
  f[0] = fe_is_zero(o[2]);
  f[1] = fe_is_zero(o[6]);
}
PROBE_OP(xyzz_add, 8, 8, 2) {
  const xyzz a{v[0], v[1], v[2], v[3]}, b{v[4], v[5], v[6], v[7]};
  put(o, xyzz_add<false>(a, b));
  put(o + 4, xyzz_add<true>(a, b));
  f[0] = fe_is_zero(o[2]);
  f[1] = fe_is_zero(o[6]);
}
PROBE_OP(xyzz_add_x_only, 8, 4, 2) {
  const xyzz a{v[0], v[1], v[2], v[3]}, b{v[4], v[5], v[6], v[7]};
  xyzz_add_x_only<false>(a, b, o[0], o[1]);
  xyzz_add_x_only<true>(a, b, o[2], o[3]);
  f[0] = fe_is_zero(o[1]);
  f[1] = fe_is_zero(o[3]);
}
PROBE_OP(jac_dbl, 4, 3, 0) {  // X Y Z | curve coefficient a
  PROBE_UNUSED;
  const jac r = jac_dbl(jac{v[0], v[1], v[2]}, v[3]);
  o[0] = r.X; o[1] = r.Y; o[2] = r.Z;
}
PROBE_OP(jac_madd, 5, 3, 0) {
  PROBE_UNUSED;
  const jac r = jac_madd(jac{v[0], v[1], v[2]}, aff{v[3], v[4]});
  o[0] = r.X; o[1] = r.Y; o[2] = r.Z;
}
PROBE_OP(jac_add, 6, 3, 0) {
  PROBE_UNUSED;
  const jac r = jac_add(jac{v[0], v[1], v[2]}, jac{v[3], v[4], v[5]});
  o[0] = r.X; o[1] = r.Y; o[2] = r.Z;
}

// ---- e. inversions ----
PROBE_OP(fe_inv, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv(v[0]); }
PROBE_OP(fe_inv_lehmer, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_lehmer(v[0]); }
PROBE_OP(fe_inv_gcd, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_gcd(v[0]); }
PROBE_OP(fe_inv_gcd_var, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_gcd_var(v[0]); }
PROBE_OP(fe_inv_plain_lehmer, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_plain_lehmer(v[0]); }
PROBE_OP(fe_inv_plain_gcd, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_plain_gcd(v[0]); }
PROBE_OP(fe_inv_plain_gcd_var, 1, 1, 0) { PROBE_UNUSED; o[0] = fe_inv_plain_gcd_var(v[0]); }
PROBE_OP(fn_inv, 1, 1, 0) { PROBE_UNUSED; o[0] = fn_inv(v[0]); }
PROBE_OP(fn_inv_var, 1, 1, 0) { PROBE_UNUSED; o[0] = fn_inv_var(v[0]); }
// the return value of lehmer_bezout as flag 0 (on the device: of the whole wave), the sign as flag 1, D as output
PROBE_OP(lehmer_bezout, 1, 1, 2) { f[0] = lehmer_bezout(FE_P, v[0], o[0], f[1]); }
// the call of fn_inv_var: modulus N, the representative in [0, N) of its input
PROBE_OP(lehmer_bezout_n, 1, 1, 2) {
  f[0] = lehmer_bezout(FN_N, fn_canon(fn_mul(v[0], FN_ONE_M)), o[0], f[1]);
}

#define FIELD_PROBE_LANE_OPS(X)                                                                          \
  X(unpack) X(pack_unpack) X(mul_forms) X(carry) X(canon) X(half) X(to_mont) X(from_mont) X(is_zero)    \
  X(eq) X(is_qr) X(xyzz_madd) X(xyzz_madd_x_only) X(xyzz_mmadd) X(xyzz_add) X(xyzz_add_x_only)          \
  X(jac_dbl) X(jac_madd) X(jac_add) X(fe_inv) X(fe_inv_lehmer) X(fe_inv_gcd) X(fe_inv_gcd_var)          \
  X(fe_inv_plain_lehmer) X(fe_inv_plain_gcd) X(fe_inv_plain_gcd_var) X(fn_inv) X(fn_inv_var)            \
  X(lehmer_bezout) X(lehmer_bezout_n)

}  // namespace probe
