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

#include "air_bodies.hpp"
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

// The first three bodies below evaluate the constraint functions of air_bodies.hpp - the ones the dense composition
// kernels of stark.hip evaluate - with the row at i read from `cur`, the row at i + 4 from `nxt` and the periodic
// values from `per` at pos mod (4 * period).  The inputs here are felts below p, a subset of the 256-bit values the
// bodies' bounds are stated for.
struct PointsRow {
  const uint64_t* row;
  SP_HD fe operator()(int c) const { return vf_fe(row + 4 * c); }
};
struct PointsPeriodic {
  const uint64_t* per;
  size_t per_len, at;  // 4 * period, pos mod per_len
  SP_HD fe operator()(int c) const { return vf_fe(per + 4 * ((size_t)c * per_len + at)); }
};
SP_HD fe points_body_pedersen(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                              const PointsAirParams& prm) {
  const fe acc = air_body_pedersen(PointsRow{cur}, PointsRow{nxt}, PointsPeriodic{per, 2048, pos & 2047}, prm.alpha,
                                   prm.sx, prm.sy);
  return fe_canon(fe_mul(acc, prm.zinv[pos & 3]));
}
SP_HD fe points_body_ec_ladder(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                               const PointsAirParams& prm) {
  const fe acc = air_body_ec_ladder(PointsRow{cur}, PointsRow{nxt}, PointsPeriodic{per, 1024, pos & 1023}, prm.alpha,
                                    prm.sx, prm.sy);
  return fe_canon(fe_mul(acc, prm.zinv[pos & 3]));
}
SP_HD fe points_body_ecdsa(const uint64_t* cur, const uint64_t* nxt, const uint64_t* per, uint64_t pos,
                           const PointsAirParams& prm) {
  const fe total = air_body_ecdsa(PointsRow{cur}, PointsRow{nxt}, PointsPeriodic{per, 4096, pos & 4095}, prm.alpha,
                                  prm.sx, prm.sy, prm.gx, prm.gy, prm.beta);
  return fe_canon(fe_mul(total, prm.zinv[pos & 3]));
}
// The range-check AIR alone is still written twice.  This body is a DUPLICATE of air_eval_range_check_kernel
// (stark.hip) - the same expressions in the same order on the same lazy-limb bounds; a change to one is a change to
// both, and tests/test_gpu_verify.py (dense parity, bit for bit) fails when they part.  Sharing it cost that kernel
// nothing in the code (one shift less) but its launch time missed the A/B margin by a microsecond
// (profiles/air_bodies_ab.txt), so it stays as it was.
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
