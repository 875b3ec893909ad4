// The verifier's two per-item checks (sp_air_eval_points_dev, sp_fri_check_queries_dev): everything a lane of the
// kernels of verify.hip does for its item, and the argument rules of the two calls.  Nothing here needs HIP: a plain
// C++ compiler builds it for the CPU tests (tests/host/verify_shim.cpp), which run the same item functions over host
// arrays.
//
// A verifier's memory follows the proof, not the trace: neither item reads a table proportional to the LDE size.  The
// composition item takes its two rows from the caller and the periodic values from the 4 * period entries of
// stark.periodic_lde; the fold item computes its own x = shift^(2^k) w^(2^k jk) by square-and-multiply from the ONE
// root of unity w of order 2^log_m and inverts 2 x with fe_inv.
//
// Arrays are packed felts (4 x u64 little-endian, plain form).  As in stark.hip no operand is converted to Montgomery
// form unless it multiplies another variable; the constants (alphas, 1 / Z_H, betas, shift, w) are Montgomery.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "curve_consts.hpp"
#include "fp29.hpp"
#include "u256.hpp"

namespace sp {

// ---- the AIRs (values of SP_AIR_* in include/starkperp.h) ----
constexpr int VAIR_PEDERSEN = 0, VAIR_EC_LADDER = 1, VAIR_ECDSA = 2, VAIR_RANGE_CHECK = 3, VAIR_COUNT = 4;
struct VerifyAirShape {
  unsigned n_cols, n_per, per_len /* 4 * period */, n_alpha, min_log_n;
};
SP_HD VerifyAirShape verify_air_shape(int air) {
  switch (air) {
    case VAIR_PEDERSEN: return {4, 6, 2048, 11, 9};
    case VAIR_EC_LADDER: return {7, 3, 1024, 12, 8};
    case VAIR_ECDSA: return {10, 12, 4096, 26, 10};
    default: return {1, 2, 512, 2, 7};
  }
}
constexpr unsigned VERIFY_MAX_LOG_N = 30;           // the dense calls' upper bound
constexpr size_t VERIFY_MAX_ITEMS = (size_t)1 << 30;  // per call: one launch (2^24 blocks of 64 lanes)
constexpr unsigned VERIFY_TPB = 64;
constexpr unsigned FRI_MAX_LOG_M = 32, FRI_MAX_LAYERS = 31;

constexpr uint8_t VERIFY_OK = 0, VERIFY_OUT_OF_RANGE = 1;                // sp_air_eval_points_dev status
constexpr uint8_t FRI_OK = 0, FRI_MISMATCH = 1, FRI_OUT_OF_RANGE = 2;    // sp_fri_check_queries_dev status

SP_HD unsigned verify_blocks(size_t items) { return (unsigned)((items + VERIFY_TPB - 1) / VERIFY_TPB); }

// ---- argument rules: nullptr, or the text for sp_last_error ----
SP_HD const char* points_check_args(int air, unsigned log_n, size_t n_points) {
  if (air < 0 || air >= VAIR_COUNT) return "unknown air (SP_AIR_PEDERSEN, _EC_LADDER, _ECDSA, _RANGE_CHECK)";
  if (log_n < verify_air_shape(air).min_log_n || log_n > VERIFY_MAX_LOG_N) return "log_n out of range for this air";
  if (n_points > VERIFY_MAX_ITEMS) return "more than 2^30 points";
  return nullptr;
}
SP_HD const char* fri_check_args(unsigned log_m, unsigned n_layers, size_t n_queries) {
  if (log_m > FRI_MAX_LOG_M || n_layers < 1 || n_layers >= log_m) return "needs 1 <= n_layers < log_m <= 32";
  if (n_queries > VERIFY_MAX_ITEMS) return "more than 2^30 queries";
  return nullptr;
}

// ---- packed felts ----
SP_HD u256 vf_load(const uint64_t* p) {
  u256 r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w;
  r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
#else
  memcpy(r.w, p, 32);
#endif
  return r;
}
SP_HD void vf_store(uint64_t* p, const u256& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  q[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
#else
  memcpy(p, v.w, 32);
#endif
}
SP_HD fe vf_fe(const uint64_t* p) { return fe_unpack(vf_load(p)); }
SP_HD bool vf_is_felt(const uint64_t* p) { return u256_lt(vf_load(p), U256_P); }

// primitive 2^log_n-th root of unity, Montgomery: 3^((p-1) / 2^log_n), p - 1 = 2^192 (2^59 + 17)
SP_HD fe verify_root_of_unity(unsigned log_n) {
  const fe three = fe_to_mont(fe{{3, 0, 0, 0, 0, 0, 0, 0, 0}});
  const uint64_t e = ((uint64_t)1 << 59) + 17;
  fe c = FE_ONE_M;
  for (int i = 63; i >= 0; --i) {
    c = fe_sqr(c);
    if ((e >> i) & 1) c = fe_mul(c, three);
  }
  return fe_sqr_n(c, 192 - (int)log_n);
}

// ---- composition value at one LDE position from its two opened rows ----
struct PointsAirParams {
  fe alpha[26];             // Montgomery; the AIR's first n_alpha are set
  fe zinv[4];               // air_zinv(times_r2 = true): R * Montgomery form of 1 / (x^n - 1) for pos mod 4
  fe sx, sy, gx, gy, beta;  // plain: SHIFT_POINT, EC_GEN, the curve's beta
};
SP_HD void points_params(int air, const uint64_t* alphas_host, PointsAirParams* prm) {
  const unsigned na = verify_air_shape(air).n_alpha;
  for (unsigned k = 0; k < 26; ++k) prm->alpha[k] = k < na ? fe_to_mont(vf_fe(alphas_host + 4 * k)) : FE_ZERO;
  prm->sx = fe_unpack(PT_SHIFT_X);
  prm->sy = fe_unpack(PT_SHIFT_Y);
  prm->gx = fe_unpack(PT_GEN_X);
  prm->gy = fe_unpack(PT_GEN_Y);
  prm->beta = fe_unpack(CURVE_BETA);
}

// The four bodies below are DUPLICATES of the dense composition kernels of stark.hip - the same expressions in the
// same order on the same lazy-limb bounds, with the row at i read from `cur`, the row at i + 4 from `nxt` and the
// periodic values from `per` at pos mod (4 * period).  Each names its twin: a change to one is a change to both, and
// tests/test_gpu_verify.py (dense parity, bit for bit) fails when they part.  The inputs here are felts below p,
// a subset of the 256-bit values the dense kernels' bounds are stated for.
//
// twin: air_eval_kernel (stark.hip), the Pedersen-step AIR
SP_HD fe points_body_pedersen(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                              const PointsAirParams& prm) {
  auto pcol = [&](int c) { return vf_fe(per + 4 * ((size_t)c * 2048 + (pos & 2047))); };
  const fe s = vf_fe(cur), px = vf_fe(cur + 4), py = vf_fe(cur + 8), lam = vf_fe(cur + 12);
  const fe s_n = vf_fe(nxt), px_n = vf_fe(nxt + 4), py_n = vf_fe(nxt + 8);
  const fe cx = pcol(0), cy = pcol(1), step = pcol(2), mid = pcol(3), end = pcol(4), z252 = pcol(5);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(s, fe_dbl(s_n)));
  const fe bM = fe_to_mont(b), lamM = fe_to_mont(lam);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  const fe dxn = fe_carry(fe_sub(px_n, px));
  const fe dyn = fe_carry(fe_sub(py_n, py));
  const fe X1 = fe_carry(fe_sub(fe_mul(lamM, fe_sub(px, cx)), fe_sub(py, cy)));
  const fe X2 = fe_carry(fe_sub(fe_sub(fe_mul(lamM, lam), px), fe_add(cx, px_n)));
  const fe X3 = fe_carry(fe_sub(fe_mul(lamM, fe_sub(px, px_n)), fe_add(py, py_n)));
  const fe in1 = fe_carry(fe_add(fe_mul(prm.alpha[0], fe_carry(fe_sub(b, one))),
                                 fe_mul3_add(prm.alpha[1], X1, prm.alpha[2], X2, prm.alpha[3], X3)));
  const fe in2 = fe_mul_add_mul(prm.alpha[4], dxn, prm.alpha[5], dyn);
  const fe acc_step = fe_mul_add_mul(bM, in1, nbM, in2);
  const fe mids = fe_mul_add_mul(prm.alpha[6], dxn, prm.alpha[7], dyn);
  const fe ends = fe_mul_add_mul(prm.alpha[8], fe_carry(fe_sub(px_n, prm.sx)), prm.alpha[9],
                                 fe_carry(fe_sub(py_n, prm.sy)));
  fe acc = fe_mul3_add(step, acc_step, mid, mids, end, ends);
  acc = fe_weak_reduce(fe_add(acc, fe_mul(prm.alpha[10], fe_mul(z252, s))));
  return fe_canon(fe_mul(acc, prm.zinv[pos & 3]));
}

// twin: air_eval_ec_ladder_kernel (stark.hip)
SP_HD fe points_body_ec_ladder(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                               const PointsAirParams& prm) {
  auto pcol = [&](int c) { return vf_fe(per + 4 * ((size_t)c * 1024 + (pos & 1023))); };
  const fe m = vf_fe(cur), px = vf_fe(cur + 4), py = vf_fe(cur + 8), qx = vf_fe(cur + 12), qy = vf_fe(cur + 16),
           la = vf_fe(cur + 20), ld = vf_fe(cur + 24);
  const fe m_n = vf_fe(nxt), px_n = vf_fe(nxt + 4), py_n = vf_fe(nxt + 8), qx_n = vf_fe(nxt + 12), qy_n = vf_fe(nxt + 16);
  const fe step = pcol(0), first = pcol(1), z251 = pcol(2);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(m, fe_dbl(m_n)));
  const fe bM = fe_to_mont(b), laM = fe_to_mont(la), ldM = fe_to_mont(ld), qxM = fe_to_mont(qx);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  fe c[9];
  c[0] = fe_mul(bM, fe_carry(fe_sub(b, one)));
  const fe qxx = fe_mul(qxM, qx);
  c[1] = fe_carry(fe_sub(fe_sub(fe_mul(ldM, fe_carry(fe_dbl(qy))), fe_carry(fe_add(fe_dbl(qxx), qxx))), one));
  c[2] = fe_carry(fe_add(fe_sub(qx_n, fe_mul(ldM, ld)), fe_dbl(qx)));
  c[3] = fe_carry(fe_add(fe_sub(qy_n, fe_mul(ldM, fe_sub(qx, qx_n))), qy));
  c[4] = fe_mul(bM, fe_carry(fe_sub(fe_mul(laM, fe_sub(px, qx)), fe_sub(py, qy))));
  c[5] = fe_mul(bM, fe_carry(fe_add(fe_sub(px_n, fe_mul(laM, la)), fe_add(px, qx))));
  c[6] = fe_mul(bM, fe_carry(fe_add(fe_sub(py_n, fe_mul(laM, fe_sub(px, px_n))), py)));
  c[7] = fe_mul(nbM, fe_carry(fe_sub(px_n, px)));
  c[8] = fe_mul(nbM, fe_carry(fe_sub(py_n, py)));
  fe acc_step = fe_mul(prm.alpha[0], c[0]);
#pragma unroll
  for (int k = 1; k < 9; ++k) acc_step = fe_weak_reduce(fe_add(acc_step, fe_mul(prm.alpha[k], c[k])));
  fe acc = fe_mul(step, acc_step);
  const fe firsts = fe_mul_add_mul(prm.alpha[9], fe_carry(fe_sub(px, prm.sx)), prm.alpha[10],
                                   fe_carry(fe_sub(py, prm.sy)));
  acc = fe_weak_reduce(fe_add(acc, fe_mul(first, firsts)));
  acc = fe_weak_reduce(fe_add(acc, fe_mul(prm.alpha[11], fe_mul(z251, m))));
  return fe_canon(fe_mul(acc, prm.zinv[pos & 3]));
}

// twin: air_eval_ecdsa_kernel (stark.hip)
SP_HD fe points_body_ecdsa(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                           const PointsAirParams& prm) {
  auto pcol = [&](int c) { return vf_fe(per + 4 * ((size_t)c * 4096 + (pos & 4095))); };
  const fe m = vf_fe(cur), px = vf_fe(cur + 4), py = vf_fe(cur + 8), qx = vf_fe(cur + 12), qy = vf_fe(cur + 16),
           la = vf_fe(cur + 20), ld = vf_fe(cur + 24), cx = vf_fe(cur + 28), cy = vf_fe(cur + 32), cr = vf_fe(cur + 36);
  const fe m_n = vf_fe(nxt), px_n = vf_fe(nxt + 4), py_n = vf_fe(nxt + 8), qx_n = vf_fe(nxt + 12), qy_n = vf_fe(nxt + 16),
           cx_n = vf_fe(nxt + 28), cy_n = vf_fe(nxt + 32), cr_n = vf_fe(nxt + 36);
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(m, fe_dbl(m_n)));
  const fe bM = fe_to_mont(b), laM = fe_to_mont(la), ldM = fe_to_mont(ld), qxM = fe_to_mont(qx), qyM = fe_to_mont(qy);
  const fe nbM = fe_carry(fe_sub(FE_ONE_M, bM));
  const fe qxx = fe_mul(qxM, qx);
  const fe lala = fe_mul(laM, la);
  fe acc = fe_mul(prm.alpha[0], fe_mul(bM, fe_carry(fe_sub(b, one))));
  auto add = [&](int k, const fe& c) { acc = fe_weak_reduce(fe_add(acc, fe_mul(prm.alpha[k], c))); };
  add(1, fe_carry(fe_sub(fe_sub(fe_mul(ldM, fe_carry(fe_dbl(qy))), fe_carry(fe_add(fe_dbl(qxx), qxx))), one)));
  add(2, fe_carry(fe_add(fe_sub(qx_n, fe_mul(ldM, ld)), fe_dbl(qx))));
  add(3, fe_carry(fe_add(fe_sub(qy_n, fe_mul(ldM, fe_sub(qx, qx_n))), qy)));
  add(4, fe_mul(bM, fe_carry(fe_sub(fe_mul(laM, fe_sub(px, qx)), fe_sub(py, qy)))));
  add(5, fe_mul(bM, fe_carry(fe_add(fe_sub(px_n, lala), fe_add(px, qx)))));
  add(6, fe_mul(bM, fe_carry(fe_add(fe_sub(py_n, fe_mul(laM, fe_sub(px, px_n))), py))));
  add(7, fe_mul(nbM, fe_carry(fe_sub(px_n, px))));
  add(8, fe_mul(nbM, fe_carry(fe_sub(py_n, py))));
  fe total = fe_mul(pcol(0), acc);
  auto term = [&](const fe& selector, const fe& value) { total = fe_weak_reduce(fe_add(total, fe_mul(selector, value))); };
  const fe first = pcol(1);
  term(first, fe_mul(prm.alpha[9], fe_carry(fe_sub(px, prm.sx))));
  term(first, fe_mul(prm.alpha[10], py));
  total = fe_weak_reduce(fe_sub(total, fe_mul(one, fe_mul(prm.alpha[10], pcol(2)))));
  term(pcol(3), fe_mul(prm.alpha[11], m));
  const fe gbase = pcol(4);
  term(gbase, fe_mul_add_mul(prm.alpha[12], fe_carry(fe_sub(qx, prm.gx)), prm.alpha[13], fe_carry(fe_sub(qy, prm.gy))));
  term(pcol(5), fe_mul(prm.alpha[14], fe_carry(fe_sub(fe_sub(fe_mul(qyM, qy), fe_mul(qxM, qxx)), fe_add(qx, prm.beta)))));
  term(pcol(6), fe_mul_add_mul(prm.alpha[15], fe_carry(fe_sub(cx_n, px)), prm.alpha[16], fe_carry(fe_sub(cy_n, py))));
  term(pcol(7), fe_mul_add_mul(prm.alpha[17], fe_carry(fe_sub(cx_n, cx)), prm.alpha[18], fe_carry(fe_sub(cy_n, cy))));
  {
    const fe a0 = fe_carry(fe_sub(fe_mul(laM, fe_sub(px, cx)), fe_sub(py, cy)));
    const fe a1 = fe_carry(fe_add(fe_sub(qx_n, lala), fe_add(px, cx)));
    const fe a2 = fe_carry(fe_add(fe_sub(qy_n, fe_mul(laM, fe_sub(px, qx_n))), py));
    term(pcol(8), fe_mul3_add(prm.alpha[19], a0, prm.alpha[20], a1, prm.alpha[21], a2));
  }
  term(pcol(9), fe_mul(prm.alpha[22], fe_carry(fe_sub(cr, m))));
  term(pcol(10), fe_mul(prm.alpha[23], fe_carry(fe_sub(cr_n, cr))));
  {
    const fe f0 = fe_carry(fe_sub(fe_mul(laM, fe_sub(px, prm.sx)), fe_add(py, prm.sy)));
    const fe f1 = fe_carry(fe_add(fe_sub(cr, lala), fe_add(px, prm.sx)));
    term(pcol(11), fe_mul_add_mul(prm.alpha[24], f0, prm.alpha[25], f1));
  }
  return fe_canon(fe_mul(total, prm.zinv[pos & 3]));
}

// twin: air_eval_range_check_kernel (stark.hip)
SP_HD fe points_body_range_check(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                                 const PointsAirParams& prm) {
  const fe v = vf_fe(cur), v_n = vf_fe(nxt);
  const fe step = vf_fe(per + 4 * (pos & 511)), last = vf_fe(per + 4 * (512 + (pos & 511)));
  const fe one = {{1, 0, 0, 0, 0, 0, 0, 0, 0}};
  const fe b = fe_carry(fe_sub(v, fe_dbl(v_n)));
  const fe c0 = fe_mul(fe_to_mont(b), fe_carry(fe_sub(b, one)));
  const fe c1 = fe_mul(fe_to_mont(v), fe_carry(fe_sub(v, one)));
  const fe acc = fe_mul_add_mul(step, fe_mul(prm.alpha[0], c0), last, fe_mul(prm.alpha[1], c1));
  return fe_canon(fe_mul(acc, prm.zinv[pos & 3]));
}

// Item i of sp_air_eval_points_dev: out[i] and status[i].  A position at or above M = 4 * 2^log_n, or a felt of the
// two rows at or above p, gives OUT_OF_RANGE and a zero value; the periodic table is read at pos mod (4 * period)
// only, so nothing is read out of bounds whatever pos holds.
template <int AIR>
SP_HD void points_item(unsigned log_n, const uint64_t* per, const PointsAirParams& prm, size_t i, const uint64_t* pos,
                       const uint64_t* cur, const uint64_t* nxt, uint64_t* out, uint8_t* status) {
  const unsigned n_cols = verify_air_shape(AIR).n_cols;
  const uint64_t p = pos[i];
  const uint64_t* c = cur + 4 * i * n_cols;
  const uint64_t* n = nxt + 4 * i * n_cols;
  bool ok = p < ((uint64_t)4 << log_n);
  for (unsigned k = 0; k < n_cols; ++k) ok = ok & vf_is_felt(c + 4 * k) & vf_is_felt(n + 4 * k);
  u256 r;
  for (int k = 0; k < 8; ++k) r.w[k] = 0;
  if (ok) {
    fe v;
    if constexpr (AIR == VAIR_PEDERSEN) v = points_body_pedersen(c, n, per, p, prm);
    else if constexpr (AIR == VAIR_EC_LADDER) v = points_body_ec_ladder(c, n, per, p, prm);
    else if constexpr (AIR == VAIR_ECDSA) v = points_body_ecdsa(c, n, per, p, prm);
    else v = points_body_range_check(c, n, per, p, prm);
    r = fe_pack(v);
  }
  vf_store(out + 4 * i, r);
  status[i] = ok ? VERIFY_OK : VERIFY_OUT_OF_RANGE;
}

// ---- one fold step of one query ----
struct FriCheckParams {
  fe beta[FRI_MAX_LAYERS];  // Montgomery
  fe shift, w;              // Montgomery: the coset shift of layer 0, the primitive 2^log_m-th root of unity
};
SP_HD void fri_params(unsigned log_m, unsigned n_layers, const uint64_t* shift_host, const uint64_t* betas_host,
                      FriCheckParams* prm) {
  for (unsigned k = 0; k < FRI_MAX_LAYERS; ++k) prm->beta[k] = k < n_layers ? fe_to_mont(vf_fe(betas_host + 4 * k)) : FE_ZERO;
  prm->shift = fe_to_mont(vf_fe(shift_host));
  prm->w = verify_root_of_unity(log_m);
}
// position of query index j in layer k: j mod 2^(log_m - k - 1)
SP_HD uint64_t fri_layer_pos(unsigned log_m, unsigned k, uint64_t j) { return j & (((uint64_t)1 << (log_m - k - 1)) - 1); }
// which member of the next layer's pair the folded value is: 0 below a quarter of this layer, else 1
SP_HD unsigned fri_next_side(unsigned log_m, unsigned k, uint64_t jk) { return jk < ((uint64_t)1 << (log_m - k - 2)) ? 0u : 1u; }

// Item (q, k) of sp_fri_check_queries_dev (oracle/stark_ref.py verify_proof, "FRI consistency"):
//   jk = index[q] mod 2^(log_m - k - 1),  x = shift^(2^k) w_{2^(log_m - k)}^jk,
//   folded = (a + b) / 2 + beta_k (a - b) / (2 x)   - the arithmetic of fri_fold_kernel (stark.hip), which takes 1 / x
//   from a table where this takes it from fe_inv -
//   compared with pairs[q][k + 1][side] (k + 1 < n_layers) or final_layer[jk].
// OUT_OF_RANGE: index[q] >= 2^(log_m - 1) (every layer of the query), or one of a, b and the value compared with is
// not below p.  About 2 k + 2 (log_m - k - 1) + 4 multiplications and one inversion.
SP_HD uint8_t fri_check_item(unsigned log_m, unsigned n_layers, const FriCheckParams& prm, size_t q, unsigned k,
                             const uint64_t* index, const uint64_t* pairs, const uint64_t* final_layer) {
  const uint64_t j = index[q];
  if (j >> (log_m - 1)) return FRI_OUT_OF_RANGE;
  const uint64_t jk = fri_layer_pos(log_m, k, j);
  const uint64_t* pa = pairs + 8 * (q * n_layers + k);
  const uint64_t* pt = k + 1 < n_layers ? pairs + 8 * (q * n_layers + k + 1) + 4 * fri_next_side(log_m, k, jk)
                                        : final_layer + 4 * jk;
  if (!(vf_is_felt(pa) & vf_is_felt(pa + 4) & vf_is_felt(pt))) return FRI_OUT_OF_RANGE;
  fe s = prm.shift, wk = prm.w;
  for (unsigned t = 0; t < k; ++t) {
    s = fe_sqr(s);
    wk = fe_sqr(wk);
  }
  fe x = s;  // times wk^jk, most significant bit first
  fe pw = FE_ONE_M;
  for (int bit = (int)(log_m - k - 1) - 1; bit >= 0; --bit) {
    pw = fe_sqr(pw);
    if ((jk >> bit) & 1) pw = fe_mul(pw, wk);
  }
  x = fe_mul(x, pw);
  const fe c2 = fe_mul(prm.beta[k], fe_inv(fe_carry(fe_dbl(x))));  // beta / (2 x), Montgomery
  const fe a = vf_fe(pa), b = vf_fe(pa + 4);
  const fe odd = fe_mul(fe_sub(a, b), c2);
  const fe even = fe_half(fe_add(a, b));
  const u256 folded = fe_pack(fe_canon(fe_carry(fe_add(even, odd))));
  const u256 want = vf_load(pt);
  uint32_t diff = 0;
  for (int i = 0; i < 8; ++i) diff |= folded.w[i] ^ want.w[i];
  return diff ? FRI_MISMATCH : FRI_OK;
}

}  // namespace sp
