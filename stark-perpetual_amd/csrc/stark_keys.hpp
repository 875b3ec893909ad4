// One item of the square-root / x-only-key batches (keys.hip), host and device: the kernels run it one item per lane,
// tests/host/felt_sqrt_shim.cpp runs the same code under g++ with the bound checks on.
#pragma once
#include "../../include/starkperp.h"
#include "curve_consts.hpp"

namespace sp {

// KEY = false:  the input itself                                      (sqrt_mod, math_utils.py:43-47)
// KEY = true:   c = in^3 + in + beta, the right-hand side at x = in  (get_y_coordinate, signature.py:84-96)
// WANT_ROOT:    out = the smaller root; false: no root, no tables - the Legendre symbol alone (is_quad_residue,
//               math_utils.py:36-40; with KEY: is_valid_stark_key, signature.py:204-214)
// `in` is a plain 256-bit integer; out is written only for SP_SQRT_OK.  0 counts as a residue with root 0 (sympy's
// is_quad_residue, which the reference calls).  The zero and range tests only choose the answer: every in-range
// non-zero input runs the same field operations.
template <bool KEY, bool WANT_ROOT>
SP_HD uint8_t stark_key_item(const u256& in, const sqrt_tables* tab, u256& out) {
  const fe a = fe_unpack(in);  // limbs 0..7 normalised, limb 8 = the top 24 bits
  if (fe_geq_p_canon_limbs(a)) return SP_SQRT_OUT_OF_RANGE;
  fe c = fe_to_mont(a);
  if (KEY) c = fe_carry(fe_add(fe_add(fe_mul(fe_sqr(c), c), c), fe_to_mont(fe_unpack(CURVE_BETA))));
  const bool zero = fe_is_zero(c);
  if (!WANT_ROOT) {
    const bool qr = fe_is_qr(c);
    return zero || qr ? SP_SQRT_OK : SP_SQRT_NON_RESIDUE;
  }
  fe root;
  const bool residue = fe_sqrt(c, tab, root);
  if (!zero && !residue) return SP_SQRT_NON_RESIDUE;
  out = fe_pack(fe_smaller_root(root));  // c = 0: root = 0
  return SP_SQRT_OK;
}

}  // namespace sp
