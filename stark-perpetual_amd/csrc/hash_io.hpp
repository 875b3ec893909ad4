// The boundary constraints that bind a Pedersen proof to its statement (sp_hash_io_boundary_dev,
// sp_hash_io_boundary_points_dev): everything a lane of the kernels of hash_io.hip does, the parameter preparation and
// the argument rules of the two calls.  Like verify.hpp nothing here needs HIP: a plain C++ compiler builds it for
// tests/host/hash_io_shim.cpp, which replays the launch plans over host arrays.
//
// The statement.  n = 512 k rows, k hashes, g = w_n, omega = g^512 of order k.  With X, Y, H the
// polynomials of degree < k that take x_i, y_i, h_i at omega^i, the composition gains
//   B(x) = a0 (s(x) - X(x)) / (x^k - 1) + a1 (s(x) - Y(x g^-256)) / (x^k + 1) + a2 (px(x) - H(x g^-511)) / (x^k - g^-k)
// - s at row 512 i is x_i, s at row 512 i + 256 is y_i, px at row 512 i + 511 is h_i.  On the LDE coset
// x_j = shift w_M^j, M = 4 n = 2048 k, so x_j^k = shift^k w_2048^j: each denominator takes 2048 values whatever n is.
//
// Arrays are packed felts (4 x u64 little-endian, plain form).  As in verify.hpp only the constants - the alphas, the
// inverse denominators, the powers of the evaluation points - are Montgomery; trace values, public columns and
// coefficients stay plain, so every product (constant) * (value) is the plain product.
#pragma once
#include "boundary.hpp"

namespace sp {

constexpr unsigned HIO_MIN_LOG_N = 9;          // one hash is 512 rows
constexpr unsigned HIO_DENSE_MAX_LOG_N = 24;   // sp_lde_dev makes the public columns up to 2^26 points
constexpr unsigned HIO_POINTS_MAX_LOG_N = 30;  // the points calls' bound (verify.hpp)
constexpr unsigned HIO_PERIOD = 2048, HIO_PERIOD_LOG = 11;  // distinct values of x^k on the coset
constexpr unsigned HIO_INV_K = 16;             // table build: consecutive entries behind one inversion
constexpr unsigned HIO_TABLE_THREADS = 3 * HIO_PERIOD / HIO_INV_K, HIO_TABLE_TPB = 64;
constexpr unsigned HIO_DENSE_TPB = 256;
constexpr unsigned HIO_POINT_TPB = 256, HIO_POINT_TPB_LOG = 8;  // lanes of a point's block = stride of its Horner rule

// ---- argument rules: nullptr, or the text for sp_last_error ----
SP_HD const char* hash_io_dense_check_args(unsigned log_n, size_t col_stride, const void* trace_lde, const void* pub_lde,
                                           const void* alphas_host, const void* shift_host, const void* out) {
  if (log_n < HIO_MIN_LOG_N || log_n > HIO_DENSE_MAX_LOG_N) return "log_n out of range (9 .. 24)";
  if (col_stride < ((size_t)4 << log_n)) return "col_stride below 4 * 2^log_n";
  if (!trace_lde) return "trace_lde is NULL";
  if (!pub_lde) return "pub_lde is NULL";
  if (!alphas_host) return "alphas_host is NULL";
  if (!shift_host) return "shift_host is NULL";
  if (!out) return "out is NULL";
  return nullptr;
}
SP_HD const char* hash_io_points_check_args(unsigned log_n, size_t n_points) {
  if (log_n < HIO_MIN_LOG_N || log_n > HIO_POINTS_MAX_LOG_N) return "log_n out of range (9 .. 30)";
  if (n_points > VERIFY_MAX_ITEMS) return "n_points above 2^30";
  return nullptr;
}

// ---- the dense call: 3 x 2048 entries alpha_c / den_c(t), Montgomery, canonical limbs ----
// den_0 = x^k - 1, den_1 = x^k + 1, den_2 = x^k - g^-k at x^k = shift^k w_2048^t.
struct HashIoTableParams {
  fe alpha[3];              // Montgomery
  fe sub[3];                // Montgomery: what den_c subtracts from x^k: 1, -1, g^-k
  fe xk0;                   // Montgomery: shift^k
  fe wpow[HIO_PERIOD_LOG];  // Montgomery: w_2048^(2^b)
  fe winv;                  // Montgomery: 1 / w_2048
};
SP_HD void hash_io_table_params(unsigned log_n, const uint64_t* alphas_host, const uint64_t* shift_host,
                                HashIoTableParams* prm) {
  for (int c = 0; c < 3; ++c) prm->alpha[c] = fe_to_mont(vf_fe(alphas_host + 4 * c));
  prm->sub[0] = FE_ONE_M;
  prm->sub[1] = fe_carry(fe_neg(FE_ONE_M));
  prm->sub[2] = fe_inv(verify_root_of_unity(9));  // g^k = w_n^(n / 512) = w_512
  prm->xk0 = fe_sqr_n(fe_to_mont(vf_fe(shift_host)), (int)(log_n - 9));
  fe w = verify_root_of_unity(HIO_PERIOD_LOG);
  prm->winv = fe_inv(w);
  for (unsigned b = 0; b < HIO_PERIOD_LOG; ++b) {
    prm->wpow[b] = w;
    w = fe_sqr(w);
  }
}
// Thread `t` of the table build, t < HIO_TABLE_THREADS: HIO_INV_K consecutive entries of one of the three tables behind
// ONE inversion (Montgomery's trick).  The prefix products wait in the entries' own slots; the way back divides x^k by
// w_2048 instead of keeping the denominators.  No denominator is 0: the call refuses a shift with shift^(4n) = 1.
SP_HD void hash_io_table_item(const HashIoTableParams& prm, unsigned t, uint64_t* table /* [3][2048] */) {
  const unsigned per_table = HIO_PERIOD / HIO_INV_K;
  const unsigned c = t / per_table, first = (t % per_table) * HIO_INV_K;
  uint64_t* slot = table + 4 * ((size_t)c * HIO_PERIOD + first);
  fe xw = prm.xk0;
  for (unsigned b = 0; b < HIO_PERIOD_LOG; ++b)
    if ((first >> b) & 1) xw = fe_mul(xw, prm.wpow[b]);
  fe run = FE_ONE_M;
  for (unsigned j = 0; j < HIO_INV_K; ++j) {
    vf_store(slot + 4 * j, fe_pack(fe_canon(run)));
    run = fe_mul(run, fe_carry(fe_sub(xw, prm.sub[c])));
    if (j + 1 < HIO_INV_K) xw = fe_mul(xw, prm.wpow[0]);
  }
  fe inv = fe_inv(run);
  for (int j = (int)HIO_INV_K - 1; j >= 0; --j) {
    const fe pre = vf_fe(slot + 4 * j);
    vf_store(slot + 4 * j, fe_pack(fe_canon(fe_mul(prm.alpha[c], fe_mul(inv, pre)))));
    inv = fe_mul(inv, fe_carry(fe_sub(xw, prm.sub[c])));
    xw = fe_mul(xw, prm.winv);
  }
}
// Point j of the dense call: out[j] = (acc ? acc[j] : 0) + B(x_j).  Seven felts moved and ONE reduction: the three
// products (alpha_c / den_c) * (difference) share it.  Bounds: a difference of two 256-bit values has limbs inside
// (-2^29, 2^29) before the carry pass, the table entries are canonical; 27 * 2^58 < 2^63.  The sum is below p in
// magnitude (3 * p * 32 p / 2^261), acc adds less than 32 p: fe_canon's range.  acc[j] is read before out[j] is
// written, so acc may be out.
SP_HD void hash_io_dense_item(const uint64_t* trace, size_t col_stride, const uint64_t* pub, size_t M,
                              const uint64_t* table, const uint64_t* acc, uint64_t* out, size_t j) {
  const fe s = vf_fe(trace + 4 * j), px = vf_fe(trace + 4 * (col_stride + j));
  const fe X = vf_fe(pub + 4 * j), Y = vf_fe(pub + 4 * (M + j)), H = vf_fe(pub + 4 * (2 * M + j));
  const size_t t = j & (HIO_PERIOD - 1);
  const fe t0 = vf_fe(table + 4 * t), t1 = vf_fe(table + 4 * (HIO_PERIOD + t)), t2 = vf_fe(table + 4 * (2 * HIO_PERIOD + t));
  fe b = fe_mul3_add(t0, fe_carry(fe_sub(s, X)), t1, fe_carry(fe_sub(s, Y)), t2, fe_carry(fe_sub(px, H)));
  if (acc) b = fe_add(b, vf_fe(acc + 4 * j));
  vf_store(out + 4 * j, fe_pack(fe_canon(b)));
}

// ---- the points call ----
// x, a lane's share of X, Y, H (log_period 9, arg[c]), the tree step, the store and the pointer rule are boundary.hpp's
// boundary_point_x, _lane_share, _share_add, _point_store and _points_check_pointers: one block plan for both calls.
static_assert(HIO_POINT_TPB == BND_POINT_TPB && HIO_POINT_TPB_LOG == BND_POINT_TPB_LOG, "boundary_lane_share's stride");
struct HashIoPointParams {
  fe alpha[3];   // Montgomery
  fe shift, w;   // Montgomery: the coset shift, the primitive M-th root of unity
  fe arg[3];     // Montgomery: what x is multiplied by before X, Y, H take it: 1, g^-256, g^-511
  fe gk_inv;     // Montgomery: g^-k
  unsigned log_n;
};
SP_HD void hash_io_point_params(unsigned log_n, const uint64_t* alphas_host, const uint64_t* shift_host,
                                HashIoPointParams* prm) {
  for (int c = 0; c < 3; ++c) prm->alpha[c] = fe_to_mont(vf_fe(alphas_host + 4 * c));
  prm->shift = fe_to_mont(vf_fe(shift_host));
  prm->w = verify_root_of_unity(log_n + 2);
  const fe g = verify_root_of_unity(log_n);
  const fe g256 = fe_sqr_n(g, 8);
  prm->arg[0] = FE_ONE_M;
  prm->arg[1] = fe_inv(g256);
  prm->arg[2] = fe_mul(fe_inv(fe_sqr(g256)), g);
  prm->gk_inv = fe_inv(verify_root_of_unity(9));
  prm->log_n = log_n;
}
// whether item i has a value at all: pos[i] below M and the four felts of its row below p
SP_HD bool hash_io_point_ok(unsigned log_n, const uint64_t* pos, const uint64_t* cur, size_t i) {
  bool ok = pos[i] < ((uint64_t)4 << log_n);
  for (unsigned c = 0; c < 4; ++c) ok = ok & vf_is_felt(cur + 4 * (4 * i + c));
  return ok;
}
// The names this call had for the shared helpers, for a caller that holds HashIoPointParams: each is boundary.hpp's.
inline const char* hash_io_points_check_pointers(const void* coef, const void* alphas_host, const void* shift_host,
                                                 const void* pos, const void* cur, const void* out, const void* status) {
  return boundary_points_check_pointers(coef, alphas_host, shift_host, pos, cur, out, status);
}
SP_HD fe hash_io_point_x(const HashIoPointParams& prm, uint64_t pos) {
  return boundary_point_x(prm.shift, prm.w, prm.log_n, pos);
}
SP_HD fe hash_io_lane_share(const HashIoPointParams& prm, const uint64_t* coef, const fe& x, unsigned c, unsigned lane) {
  return boundary_lane_share(prm.log_n, 9, prm.arg[c], coef, x, c, lane);
}
SP_HD fe hash_io_share_add(const fe& a, const fe& b) { return boundary_share_add(a, b); }
SP_HD void hash_io_point_store(bool ok, const fe& value, size_t i, uint64_t* out, uint8_t* status) {
  boundary_point_store(ok, value, i, out, status);
}
// What lane 0 does with the three sums: the three denominators from x^k, ONE inversion for the three of them, the
// three products behind one reduction as in the dense item.  Canonical.
SP_HD fe hash_io_point_value(const HashIoPointParams& prm, const fe& x, const uint64_t* cur, const fe& X, const fe& Y,
                             const fe& H) {
  const fe xk = fe_sqr_n(x, (int)(prm.log_n - 9));
  const fe d0 = fe_carry(fe_sub(xk, FE_ONE_M)), d1 = fe_carry(fe_add(xk, FE_ONE_M)), d2 = fe_carry(fe_sub(xk, prm.gk_inv));
  const fe d01 = fe_mul(d0, d1);
  const fe inv = fe_inv(fe_mul(d01, d2));
  const fe i2 = fe_mul(inv, d01), i01 = fe_mul(inv, d2);
  const fe i0 = fe_mul(i01, d1), i1 = fe_mul(i01, d0);
  const fe s = vf_fe(cur), px = vf_fe(cur + 4);
  return fe_canon(fe_mul3_add(fe_mul(prm.alpha[0], i0), fe_carry(fe_sub(s, X)), fe_mul(prm.alpha[1], i1),
                              fe_carry(fe_sub(s, Y)), fe_mul(prm.alpha[2], i2), fe_carry(fe_sub(px, H))));
}
}  // namespace sp
