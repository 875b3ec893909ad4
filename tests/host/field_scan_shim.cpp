// Host-side shim of tests/test_field_scan_host.py: the product-scanning forms of csrc/fp29.hpp beside their column
// forms, compiled with g++ and bound checks on (a column or limb that leaves its budget aborts the process).
// Works on raw limbs (9 x int32 per element) so that the test chooses N-form patterns directly.
// Test infrastructure only - never loaded by the product.
#define SP_CHECK_BOUNDS 1
#include "../../stark-perpetual_amd/csrc/curve.hpp"
#include <string.h>
using namespace sp;

static fe ld(const int32_t* p) { fe r; memcpy(r.l, p, sizeof r.l); return r; }
static void st(int32_t* p, const fe& a) { memcpy(p, a.l, sizeof a.l); }
static bool same(const fe& a, const fe& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
static bool same(const xyzz& a, const xyzz& b) { return same(a.X, b.X) && same(a.Y, b.Y) && same(a.ZZ, b.ZZ) && same(a.ZZZ, b.ZZZ); }

enum { OP_MUL, OP_SQR, OP_MUL_SUB_MUL, OP_MUL_ADD_MUL, OP_MUL3_ADD, N_OPS };

static void both(int op, const fe* v, fe& col, fe& scan) {
  switch (op) {
    case OP_MUL: col = fe_mul(v[0], v[1]); scan = fe_mul_scan(v[0], v[1]); break;
    case OP_SQR: col = fe_sqr(v[0]); scan = fe_sqr_scan(v[0]); break;
    case OP_MUL_SUB_MUL: col = fe_mul_sub_mul(v[0], v[1], v[2], v[3]); scan = fe_mul_sub_mul_scan(v[0], v[1], v[2], v[3]); break;
    case OP_MUL_ADD_MUL: col = fe_mul_add_mul(v[0], v[1], v[2], v[3]); scan = fe_mul_add_mul_scan(v[0], v[1], v[2], v[3]); break;
    default: col = fe_mul3_add(v[0], v[1], v[2], v[3], v[4], v[5]); scan = fe_mul3_add_scan(v[0], v[1], v[2], v[3], v[4], v[5]); break;
  }
}

extern "C" {
// in: 6 elements; out: N_OPS x (column result, scan result)
void t_scan_ops(const int32_t* in, int32_t* out) {
  fe v[6];
  for (int k = 0; k < 6; ++k) v[k] = ld(in + NL * k);
  for (int op = 0; op < N_OPS; ++op) {
    fe c, s;
    both(op, v, c, s);
    st(out + NL * (2 * op), c);
    st(out + NL * (2 * op + 1), s);
  }
}
// n elements; operands of item i are elements i, i + 1, .. i + 5 (cyclic).  Returns -1 when every scan form equals its
// column form limb for limb on every item, else item * 16 + op of the first difference.
long t_scan_compare(const int32_t* elems, long n) {
  for (long i = 0; i < n; ++i) {
    fe v[6];
    for (int k = 0; k < 6; ++k) v[k] = ld(elems + NL * ((i + k) % n));
    for (int op = 0; op < N_OPS; ++op) {
      fe c, s;
      both(op, v, c, s);
      if (!same(c, s)) return i * 16 + op;
    }
  }
  return -1;
}
// every 6-tuple of the npat pattern elements: each pattern in every operand position of every form
long t_scan_compare_tuples(const int32_t* pats, int npat) {
  long total = 1;
  for (int k = 0; k < 6; ++k) total *= npat;
  for (long t = 0; t < total; ++t) {
    fe v[6];
    long r = t;
    for (int k = 0; k < 6; ++k) { v[k] = ld(pats + NL * (r % npat)); r /= npat; }
    for (int op = 0; op < N_OPS; ++op) {
      fe c, s;
      both(op, v, c, s);
      if (!same(c, s)) return t * 16 + op;
    }
  }
  return -1;
}
// The group law with both forms on "points" made of consecutive elements (the chord rule does not use the curve
// equation): the lazy differences the formulas feed into products go through the scan forms' bound checks too.
// Returns -1, or item * 16 + the number of the first formula that differs.
long t_scan_compare_xyzz(const int32_t* elems, long n) {
  for (long i = 0; i < n; ++i) {
    fe v[8];
    for (int k = 0; k < 8; ++k) v[k] = ld(elems + NL * ((i + k) % n));
    const aff p{v[0], v[1]}, q{v[2], v[3]};
    const xyzz a{v[0], v[1], v[4], v[5]}, b{v[2], v[3], v[6], v[7]};
    if (!same(xyzz_mmadd<false>(p, q), xyzz_mmadd<true>(p, q))) return i * 16 + 0;
    if (!same(xyzz_madd<false>(a, q), xyzz_madd<true>(a, q))) return i * 16 + 1;
    if (!same(xyzz_add<false>(a, b), xyzz_add<true>(a, b))) return i * 16 + 2;
    fe x0, z0, x1, z1;
    xyzz_madd_x_only<false>(a, q, x0, z0);
    xyzz_madd_x_only<true>(a, q, x1, z1);
    if (!same(x0, x1) || !same(z0, z1)) return i * 16 + 3;
    xyzz_add_x_only<false>(a, b, x0, z0);
    xyzz_add_x_only<true>(a, b, x1, z1);
    if (!same(x0, x1) || !same(z0, z1)) return i * 16 + 4;
  }
  return -1;
}
// canonical limbs (29 bits each) of an N-form or lazy value
void t_canon(const int32_t* limbs, int32_t* out) { st(out, fe_canon(ld(limbs))); }
}
