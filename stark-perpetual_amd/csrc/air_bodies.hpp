// The constraint expressions of the AIRs (all but the range check), written once: the dense composition kernels
// (stark.hip, builtins.hip) and the verifier's point bodies (verify.hpp, verify_builtins.hpp) both evaluate these
// functions, so the prover and the verifier cannot come to disagree about a constraint.  Nothing here needs HIP.
//
// Each body is a template over three LOADERS - functors cur(c), nxt(c), per(c) returning the fe of column c of the
// row at the point, of the next trace row (4 LDE rows on), and of the periodic tables at the point - so that every
// load stays where its value is used and each caller keeps its own index arithmetic (row shards, halo, col_stride;
// or the two opened rows of a proof).  The alphas are Montgomery; the other constants are named per body.  A body
// returns the sum before the division by Z_H: the caller multiplies by its zinv entry, reduces and stores.
//
// The three bodies of stark.hip take PLAIN operands: only what multiplies another variable is converted to
// Montgomery form, products with one Montgomery factor are plain again, and the single 1/R left by
// `selector * (...)` is absorbed by the caller's zinv (air_zinv, times_r2).  The bounds are stated for any 256-bit
// value a loader returns; felts below p are a subset.
#pragma once
#include "fp29.hpp"

namespace sp {

// Pedersen-step AIR (11 constraints; oracle/stark_ref.py constraint_values).  cur: s, px, py, lam; nxt: s, px, py;
// per: cx, cy, step, mid, end, z252.  sx, sy: SHIFT_POINT, plain.
// Only b and lambda (the two variables that multiply other variables) are converted to Montgomery form.
template <class Cur, class Nxt, class Per>
SP_HD fe air_body_pedersen(Cur cur, Nxt nxt, Per per, const fe* alpha, const fe& sx, const fe& sy) {
  const fe s = cur(0), px = cur(1), py = cur(2), lam = cur(3);
  const fe s_n = nxt(0), px_n = nxt(1), py_n = nxt(2);
  const fe cx = per(0), cy = per(1), step = per(2), mid = per(3), end = per(4), z252 = per(5);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(s, fe_dbl(s_n)));
  const fe bM = fe_to_mont(b), lamM = fe_to_mont(lam);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  const fe dxn = fe_carry(fe_sub(px_n, px));
  const fe dyn = fe_carry(fe_sub(py_n, py));
  // step rows: bM (alpha0 (b - 1) + alpha1 X1 + alpha2 X2 + alpha3 X3) + nbM (alpha4 dx' + alpha5 dy'): sums
  // of products share one reduction (fe_mul3_add / fe_mul_add_mul), and the common factors bM, nbM
  // are applied once - about 20 multiplication-equivalents per point instead of 27
  const fe X1 = fe_carry(fe_sub(fe_mul(lamM, fe_sub(px, cx)), fe_sub(py, cy)));
  const fe X2 = fe_carry(fe_sub(fe_sub(fe_mul(lamM, lam), px), fe_add(cx, px_n)));
  const fe X3 = fe_carry(fe_sub(fe_mul(lamM, fe_sub(px, px_n)), fe_add(py, py_n)));
  const fe in1 = fe_carry(fe_add(fe_mul(alpha[0], fe_carry(fe_sub(b, one))),
                                 fe_mul3_add(alpha[1], X1, alpha[2], X2, alpha[3], X3)));
  const fe in2 = fe_mul_add_mul(alpha[4], dxn, alpha[5], dyn);
  const fe acc_step = fe_mul_add_mul(bM, in1, nbM, in2);
  const fe mids = fe_mul_add_mul(alpha[6], dxn, alpha[7], dyn);
  const fe ends = fe_mul_add_mul(alpha[8], fe_carry(fe_sub(px_n, sx)), alpha[9], fe_carry(fe_sub(py_n, sy)));
  fe acc = fe_mul3_add(step, acc_step, mid, mids, end, ends);
  return fe_weak_reduce(fe_add(acc, fe_mul(alpha[10], fe_mul(z252, s))));
}

// EC-ladder AIR (12 constraints).  cur: m, px, py, qx, qy, la, ld; nxt: m, px, py, qx, qy; per: step, first, z251.
// sx, sy: SHIFT_POINT, plain.  Four conversions (b, la, ld, qx) instead of fifteen.
template <class Cur, class Nxt, class Per>
SP_HD fe air_body_ec_ladder(Cur cur, Nxt nxt, Per per, const fe* alpha, const fe& sx, const fe& sy) {
  const fe m = cur(0), px = cur(1), py = cur(2), qx = cur(3), qy = cur(4), la = cur(5), ld = cur(6);
  const fe m_n = nxt(0), px_n = nxt(1), py_n = nxt(2), qx_n = nxt(3), qy_n = nxt(4);
  const fe step = per(0), first = per(1), z251 = per(2);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(m, fe_dbl(m_n)));
  const fe bM = fe_to_mont(b), laM = fe_to_mont(la), ldM = fe_to_mont(ld), qxM = fe_to_mont(qx);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  fe c[9];
  c[0] = fe_mul(bM, fe_carry(fe_sub(b, one)));
  // doubling: ld 2 qy - 3 qx^2 - 1 ; qx' - ld^2 + 2 qx ; qy' - ld (qx - qx') + qy
  const fe qxx = fe_mul(qxM, qx);
  c[1] = fe_carry(fe_sub(fe_sub(fe_mul(ldM, fe_carry(fe_dbl(qy))), fe_carry(fe_add(fe_dbl(qxx), qxx))), one));
  c[2] = fe_carry(fe_add(fe_sub(qx_n, fe_mul(ldM, ld)), fe_dbl(qx)));
  c[3] = fe_carry(fe_add(fe_sub(qy_n, fe_mul(ldM, fe_sub(qx, qx_n))), qy));
  // addition (gated by b): la (px - qx) - (py - qy) ; px' - la^2 + px + qx ; py' - la (px - px') + py
  c[4] = fe_mul(bM, fe_carry(fe_sub(fe_mul(laM, fe_sub(px, qx)), fe_sub(py, qy))));
  c[5] = fe_mul(bM, fe_carry(fe_add(fe_sub(px_n, fe_mul(laM, la)), fe_add(px, qx))));
  c[6] = fe_mul(bM, fe_carry(fe_add(fe_sub(py_n, fe_mul(laM, fe_sub(px, px_n))), py)));
  c[7] = fe_mul(nbM, fe_carry(fe_sub(px_n, px)));
  c[8] = fe_mul(nbM, fe_carry(fe_sub(py_n, py)));
  fe acc_step = fe_mul(alpha[0], c[0]);
#pragma unroll
  for (int k = 1; k < 9; ++k) acc_step = fe_weak_reduce(fe_add(acc_step, fe_mul(alpha[k], c[k])));
  fe acc = fe_mul(step, acc_step);
  const fe firsts = fe_mul_add_mul(alpha[9], fe_carry(fe_sub(px, sx)), alpha[10], fe_carry(fe_sub(py, sy)));
  acc = fe_weak_reduce(fe_add(acc, fe_mul(first, firsts)));
  return fe_weak_reduce(fe_add(acc, fe_mul(alpha[11], fe_mul(z251, m))));
}

// ECDSA-verification AIR (26 constraints, oracle/stark_ref.py ecdsa_constraint_values).  cur: m, px, py, qx, qy, la,
// ld, cx, cy, cr; nxt: the same columns (la, ld unread); per: 12 tables.  sx, sy: SHIFT_POINT; gx, gy: EC_GEN; beta:
// the curve's - all plain.
template <class Cur, class Nxt, class Per>
SP_HD fe air_body_ecdsa(Cur cur, Nxt nxt, Per per, const fe* alpha, const fe& sx, const fe& sy, const fe& gx,
                        const fe& gy, const fe& beta) {
  const fe m = cur(0), px = cur(1), py = cur(2), qx = cur(3), qy = cur(4), la = cur(5), ld = cur(6), cx = cur(7),
           cy = cur(8), cr = cur(9);
  const fe m_n = nxt(0), px_n = nxt(1), py_n = nxt(2), qx_n = nxt(3), qy_n = nxt(4), cx_n = nxt(7), cy_n = nxt(8),
           cr_n = nxt(9);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(m, fe_dbl(m_n)));
  const fe bM = fe_to_mont(b), laM = fe_to_mont(la), ldM = fe_to_mont(ld), qxM = fe_to_mont(qx), qyM = fe_to_mont(qy);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  const fe qxx = fe_mul(qxM, qx);
  const fe lala = fe_mul(laM, la);
  // ladder rows (selector `step`)
  fe acc = fe_mul(alpha[0], fe_mul(bM, fe_carry(fe_sub(b, one))));
  auto add = [&](int k, const fe& c) { acc = fe_weak_reduce(fe_add(acc, fe_mul(alpha[k], c))); };
  add(1, fe_carry(fe_sub(fe_sub(fe_mul(ldM, fe_carry(fe_dbl(qy))), fe_carry(fe_add(fe_dbl(qxx), qxx))), one)));
  add(2, fe_carry(fe_add(fe_sub(qx_n, fe_mul(ldM, ld)), fe_dbl(qx))));
  add(3, fe_carry(fe_add(fe_sub(qy_n, fe_mul(ldM, fe_sub(qx, qx_n))), qy)));
  add(4, fe_mul(bM, fe_carry(fe_sub(fe_mul(laM, fe_sub(px, qx)), fe_sub(py, qy)))));
  add(5, fe_mul(bM, fe_carry(fe_add(fe_sub(px_n, lala), fe_add(px, qx)))));
  add(6, fe_mul(bM, fe_carry(fe_add(fe_sub(py_n, fe_mul(laM, fe_sub(px, px_n))), py))));
  add(7, fe_mul(nbM, fe_carry(fe_sub(px_n, px))));
  add(8, fe_mul(nbM, fe_carry(fe_sub(py_n, py))));
  fe total = fe_mul(per(0), acc);  // every term below carries the same single 1/R (absorbed by zinv)
  auto term = [&](const fe& selector, const fe& value) { total = fe_weak_reduce(fe_add(total, fe_mul(selector, value))); };
  const fe first = per(1);
  term(first, fe_mul(alpha[9], fe_carry(fe_sub(px, sx))));
  // alpha10 (first * py - start_y): start_y is plain, so alpha10 * start_y is plain and must lose one R like the rest
  term(first, fe_mul(alpha[10], py));
  total = fe_weak_reduce(fe_sub(total, fe_mul(one, fe_mul(alpha[10], per(2)))));
  term(per(3), fe_mul(alpha[11], m));
  const fe gbase = per(4);
  term(gbase, fe_mul_add_mul(alpha[12], fe_carry(fe_sub(qx, gx)), alpha[13], fe_carry(fe_sub(qy, gy))));
  // on-curve: qy^2 - qx^3 - qx - beta
  term(per(5), fe_mul(alpha[14], fe_carry(fe_sub(fe_sub(fe_mul(qyM, qy), fe_mul(qxM, qxx)), fe_add(qx, beta)))));
  term(per(6), fe_mul_add_mul(alpha[15], fe_carry(fe_sub(cx_n, px)), alpha[16], fe_carry(fe_sub(cy_n, py))));
  term(per(7), fe_mul_add_mul(alpha[17], fe_carry(fe_sub(cx_n, cx)), alpha[18], fe_carry(fe_sub(cy_n, cy))));
  {
    const fe a0 = fe_carry(fe_sub(fe_mul(laM, fe_sub(px, cx)), fe_sub(py, cy)));
    const fe a1 = fe_carry(fe_add(fe_sub(qx_n, lala), fe_add(px, cx)));
    const fe a2 = fe_carry(fe_add(fe_sub(qy_n, fe_mul(laM, fe_sub(px, qx_n))), py));
    term(per(8), fe_mul3_add(alpha[19], a0, alpha[20], a1, alpha[21], a2));
  }
  term(per(9), fe_mul(alpha[22], fe_carry(fe_sub(cr, m))));
  term(per(10), fe_mul(alpha[23], fe_carry(fe_sub(cr_n, cr))));
  {
    const fe f0 = fe_carry(fe_sub(fe_mul(laM, fe_sub(px, sx)), fe_add(py, sy)));
    const fe f1 = fe_carry(fe_add(fe_sub(cr, lala), fe_add(px, sx)));
    term(per(11), fe_mul_add_mul(alpha[24], f0, alpha[25], f1));
  }
  return total;
}

// The range-check AIR (two constraints) is not here: air_eval_range_check_kernel (stark.hip) and
// points_body_range_check (verify.hpp) keep a copy each, see the comment in verify.hpp.

// rc16 AIR: the numerators C0 .. C7 of oracle/stark_ref.rc16_constraint_values combined as rc16_composition_value.
// Unlike the three bodies above it keeps its Montgomery factors itself: the loaders return MONTGOMERY operands, zinv
// carries no R^2, and the Montgomery result is the whole composition value - the caller only converts and stores.
// cur, nxt: a, acc, s and, as column 3, the second-phase column p; per: first8, step8.  zinv: the caller's entry of
// 1 / (x^n - 1) for the point; z, rc_min, rc_max, two16: Montgomery; dl = x - g^(n-1), il = 1 / dl, i1 = 1 / (x - 1)
// at the point, Montgomery (the dense kernel reads them from tables, a verifier's lane derives them from x).
template <class Cur, class Nxt, class Per>
SP_HD fe air_body_rc16(Cur cur, Nxt nxt, Per per, const fe* alpha, const fe& zinv, const fe& z, const fe& rc_min,
                       const fe& rc_max, const fe& two16, const fe dl, const fe il, const fe i1) {
  const fe a = cur(0), acc = cur(1), s = cur(2);
  const fe an = nxt(0), accn = nxt(1), sn = nxt(2);
  const fe pc = cur(3), pn = nxt(3);
  const fe first8 = per(0), step8 = per(1);
  // numerators, all Montgomery N-form
  const fe c0 = fe_mul(first8, fe_sub(acc, a));
  const fe c1 = fe_mul(step8, fe_carry(fe_sub(fe_sub(accn, fe_mul(acc, two16)), an)));
  const fe d = fe_carry(fe_sub(sn, s));
  const fe c2 = fe_mul(d, fe_carry(fe_sub(d, FE_ONE_M)));
  const fe c3 = fe_mul_sub_mul(pn, fe_carry(fe_sub(z, sn)), pc, fe_carry(fe_sub(z, an)));
  const fe c4 = fe_carry(fe_sub(fe_mul(pc, fe_carry(fe_sub(z, s))), fe_sub(z, a)));
  const fe c5 = fe_carry(fe_sub(pc, FE_ONE_M));
  const fe c6 = fe_carry(fe_sub(s, rc_min));
  const fe c7 = fe_carry(fe_sub(s, rc_max));
  const fe t_all = fe_mul_add_mul(alpha[0], c0, alpha[1], c1);
  const fe t_notlast = fe_mul(fe_mul_add_mul(alpha[2], c2, alpha[3], c3), dl);
  const fe trans = fe_mul(fe_carry(fe_add(t_all, t_notlast)), zinv);
  const fe firstp = fe_mul(fe_mul_add_mul(alpha[4], c4, alpha[6], c6), i1);
  const fe lastp = fe_mul(fe_mul_add_mul(alpha[5], c5, alpha[7], c7), il);
  return fe_carry(fe_add(fe_add(trans, firstp), lastp));
}

}  // namespace sp
