// Boundary constraints for ANY periodic AIR (sp_boundary_dev, sp_boundary_points_dev): the descriptor, the argument
// rules, the parameter preparation and everything a lane of the kernels of boundary.hip does.  Like hash_io.hpp, of
// which this is the generalisation, nothing here needs HIP: a plain C++ compiler builds it for
// tests/host/boundary_shim.cpp, which replays the launch plans over host arrays.
//
// The statement.  An AIR of period p = 2^log_period, n = p k rows, g = w_n, omega = g^p of order k,
// M = 4 n.  A boundary GROUP d is a row o_d < p with terms (column c_t, public list v_t): "column c_t at row
// p i + o_d is v_t[i]".  With one challenge a_t per term and C_d the polynomial of degree < k through
// sum_{t in d} a_t v_t[i] at omega^i - ONE public polynomial per group - the composition gains
//   B(x) = sum_d ( sum_{t in d} a_t col_{c_t}(x) - C_d(x g^-o_d) ) / (x^k - w_p^o_d).
// On the LDE coset x_j = shift w_M^j, so x_j^k = shift^k w_{4p}^j: each denominator takes 4 p values whatever n is.
//
// Arrays are packed felts (4 x u64 little-endian, plain form).  As in verify.hpp only the constants - the alphas, the
// inverse denominators, the powers of the evaluation points - are Montgomery; trace values, public columns and
// coefficients stay plain, so every product (constant) * (value) is the plain product.
#pragma once
#include "verify.hpp"

namespace sp {

constexpr unsigned BND_MIN_LOG_PERIOD = 7, BND_MAX_LOG_PERIOD = 10;
constexpr unsigned BND_MAX_COLS = 16, BND_MAX_GROUPS = 4, BND_MAX_TERMS = 8;
constexpr unsigned BND_DENSE_MAX_LOG_N = 24;   // sp_lde_dev makes the public columns up to 2^26 points
constexpr unsigned BND_POINTS_MAX_LOG_N = 30;  // the points calls' bound (verify.hpp)
constexpr unsigned BND_INV_K = 16;             // table build: consecutive entries behind one inversion
constexpr unsigned BND_TABLE_TPB = 64, BND_DENSE_TPB = 256;
constexpr unsigned BND_POINT_TPB = 256, BND_POINT_TPB_LOG = 8;  // lanes of a point's block = stride of its Horner rule

// The descriptor as the calls take it: host arrays, read before the call returns.
struct BoundaryDesc {
  unsigned log_period, n_cols, n_groups;
  const unsigned* group_rows;   // [n_groups] distinct, below the period
  unsigned n_terms;
  const unsigned* term_cols;    // [n_terms] below n_cols
  const unsigned* term_groups;  // [n_terms] below n_groups; every group has a term
};

// ---- argument rules: nullptr, or the text for sp_last_error ----
inline const char* boundary_check_desc(const BoundaryDesc& d) {
  if (d.log_period < BND_MIN_LOG_PERIOD || d.log_period > BND_MAX_LOG_PERIOD) return "log_period out of range (7 .. 10)";
  if (d.n_cols < 1 || d.n_cols > BND_MAX_COLS) return "n_cols out of range (1 .. 16)";
  if (d.n_groups < 1 || d.n_groups > BND_MAX_GROUPS) return "n_groups out of range (1 .. 4)";
  if (d.n_terms < 1 || d.n_terms > BND_MAX_TERMS) return "n_terms out of range (1 .. 8)";
  if (!d.group_rows) return "group_rows is NULL";
  if (!d.term_cols) return "term_cols is NULL";
  if (!d.term_groups) return "term_groups is NULL";
  for (unsigned a = 0; a < d.n_groups; ++a) {
    if (d.group_rows[a] >= 1u << d.log_period) return "group_rows holds a row at or above the period";
    for (unsigned b = 0; b < a; ++b)
      if (d.group_rows[a] == d.group_rows[b]) return "group_rows holds a row twice";
  }
  unsigned used = 0;
  for (unsigned t = 0; t < d.n_terms; ++t) {
    if (d.term_cols[t] >= d.n_cols) return "term_cols holds a column at or above n_cols";
    if (d.term_groups[t] >= d.n_groups) return "term_groups holds a group at or above n_groups";
    used |= 1u << d.term_groups[t];
  }
  if (used != (1u << d.n_groups) - 1) return "term_groups leaves a group without a term";
  return nullptr;
}
inline const char* boundary_dense_check_args(const BoundaryDesc& d, unsigned log_n, size_t col_stride,
                                             const void* trace_lde, const void* pub_lde, const void* alphas_host,
                                             const void* shift_host, const void* out) {
  if (log_n < d.log_period || log_n > BND_DENSE_MAX_LOG_N) return "log_n out of range (log_period .. 24)";
  if (col_stride < ((size_t)4 << log_n)) return "col_stride below 4 * 2^log_n";
  if (!trace_lde) return "trace_lde is NULL";
  if (!pub_lde) return "pub_lde is NULL";
  if (!alphas_host) return "alphas_host is NULL";
  if (!shift_host) return "shift_host is NULL";
  if (!out) return "out is NULL";
  return nullptr;
}
inline const char* boundary_points_check_args(const BoundaryDesc& d, unsigned log_n, size_t n_points) {
  if (log_n < d.log_period || log_n > BND_POINTS_MAX_LOG_N) return "log_n out of range (log_period .. 30)";
  if (n_points > VERIFY_MAX_ITEMS) return "n_points above 2^30";
  return nullptr;
}
inline const char* boundary_points_check_pointers(const void* coef, const void* alphas_host, const void* shift_host,
                                                  const void* pos, const void* cur, const void* out,
                                                  const void* status) {
  if (!coef) return "coef is NULL";
  if (!alphas_host) return "alphas_host is NULL";
  if (!shift_host) return "shift_host is NULL";
  if (!pos) return "pos is NULL";
  if (!cur) return "cur is NULL";
  if (!out) return "out is NULL";
  if (!status) return "status is NULL";
  return nullptr;
}

// ---- what the kernels get of a checked descriptor: the terms ordered by group, their challenges with them ----
struct BoundaryTerms {
  fe alpha[BND_MAX_TERMS];            // Montgomery, in the order of col[]
  unsigned col[BND_MAX_TERMS];
  unsigned first[BND_MAX_GROUPS + 1];  // the terms of group d are first[d] .. first[d + 1] - 1
  unsigned n_groups, n_cols, log_period;
};
inline fe boundary_pow(fe base, unsigned e) {  // Montgomery base^e, host
  fe r = FE_ONE_M;
  for (; e; e >>= 1) {
    if (e & 1) r = fe_mul(r, base);
    base = fe_sqr(base);
  }
  return r;
}
inline void boundary_terms(const BoundaryDesc& d, const uint64_t* alphas_host, BoundaryTerms* tm) {
  unsigned at = 0;
  for (unsigned g = 0; g < BND_MAX_GROUPS; ++g) {
    tm->first[g] = at;
    for (unsigned t = 0; g < d.n_groups && t < d.n_terms; ++t)
      if (d.term_groups[t] == g) {
        tm->alpha[at] = fe_to_mont(vf_fe(alphas_host + 4 * t));
        tm->col[at++] = d.term_cols[t];
      }
  }
  tm->first[BND_MAX_GROUPS] = at;
  for (; at < BND_MAX_TERMS; ++at) tm->alpha[at] = FE_ZERO, tm->col[at] = 0;
  tm->n_groups = d.n_groups, tm->n_cols = d.n_cols, tm->log_period = d.log_period;
}

// The arithmetic both calls end in: sum_d inv_d * (sum_{t in d} alpha_t col_t - C_d), N-form, below 2p in magnitude.
// col(t), pub(d), inv(d) fetch a plain trace felt, the plain value of C_d and the Montgomery inverse denominator.
// AT MOST THREE PRODUCTS SHARE A REDUCTION, the bound fe_mul3_add documents (27 * 2^58 < 2^63):
//   inner: alpha_t is N-form, a plain 256-bit value has limbs below 2^29, so a run of up to three terms goes through
//     one fe_reduce; its result lies inside (-p, 3 p 2^256 / 2^261] = (-p, p / 8).  A group of eight terms is three
//     runs; their fe_add has limbs below 3 * 2^29 and a value inside (-3p, 3p / 8).
//   C_d is below 2^256 < 32 p; the difference has limbs inside (-2^29, 2^31 - 2^29) and fe_carry makes it N-form
//     with a value inside (-35 p, p).
//   outer: inv_d is canonical; three products of a canonical felt and such a difference stay below
//     3 * p * 35 p / 2^261 < p / 8 in magnitude after the one reduction they share, a fourth group is a run of its
//     own.  The sum of the two runs is inside (-2p, 2p).
template <class Col, class Pub, class Inv>
SP_HD fe boundary_combine(const BoundaryTerms& tm, Col col, Pub pub, Inv inv) {
  fe total = FE_ZERO;
  cols outer;
  cols_zero(outer);
  unsigned in_outer = 0;
  for (unsigned d = 0; d < tm.n_groups; ++d) {
    fe u = FE_ZERO;
    for (unsigned t = tm.first[d]; t < tm.first[d + 1]; t += 3) {
      cols inner;
      cols_zero(inner);
      for (unsigned i = t; i < t + 3 && i < tm.first[d + 1]; ++i) cols_mac(inner, tm.alpha[i], col(i));
      u = fe_add(u, fe_reduce(inner));
    }
    cols_mac(outer, inv(d), fe_carry(fe_sub(u, pub(d))));
    if (++in_outer == 3 || d + 1 == tm.n_groups) {
      total = fe_add(total, fe_reduce(outer));
      cols_zero(outer);
      in_outer = 0;
    }
  }
  return total;
}

// ---- the dense call: n_groups x 4p entries 1 / den_d(t), Montgomery, canonical limbs ----
// den_d = x^k - w_p^o_d at x^k = shift^k w_4p^t.
struct BoundaryTableParams {
  fe sub[BND_MAX_GROUPS];          // Montgomery: w_p^o_d
  fe xk0;                          // Montgomery: shift^k
  fe wpow[BND_MAX_LOG_PERIOD + 2];  // Montgomery: w_4p^(2^b)
  fe winv;                         // Montgomery: 1 / w_4p
  unsigned log_4p, n_groups;
};
inline void boundary_table_params(const BoundaryDesc& d, unsigned log_n, const uint64_t* shift_host,
                                  BoundaryTableParams* prm) {
  const fe wp = verify_root_of_unity(d.log_period);
  for (unsigned g = 0; g < BND_MAX_GROUPS; ++g) prm->sub[g] = g < d.n_groups ? boundary_pow(wp, d.group_rows[g]) : FE_ZERO;
  prm->xk0 = fe_sqr_n(fe_to_mont(vf_fe(shift_host)), (int)(log_n - d.log_period));
  prm->log_4p = d.log_period + 2;
  prm->n_groups = d.n_groups;
  fe w = verify_root_of_unity(prm->log_4p);
  prm->winv = fe_inv(w);
  for (unsigned b = 0; b < BND_MAX_LOG_PERIOD + 2; ++b) {
    prm->wpow[b] = w;
    w = fe_sqr(w);
  }
}
SP_HD unsigned boundary_table_threads(const BoundaryTableParams& prm) { return (prm.n_groups << prm.log_4p) / BND_INV_K; }
// Thread `t` of the table build, t < boundary_table_threads: BND_INV_K consecutive entries of one group's table behind
// ONE inversion (Montgomery's trick), as hash_io_table_item does it: the prefix products wait in the entries' own
// slots; the way back divides x^k by w_4p instead of keeping the denominators.  No denominator is 0: the call refuses
// a shift with shift^(4n) = 1.  4p is a multiple of BND_INV_K, so a thread's entries belong to one group.
SP_HD void boundary_table_item(const BoundaryTableParams& prm, unsigned t, uint64_t* table /* [n_groups][4p] */) {
  const unsigned per_table = (1u << prm.log_4p) / BND_INV_K;
  const unsigned d = t / per_table, first = (t % per_table) * BND_INV_K;
  uint64_t* slot = table + 4 * (((size_t)d << prm.log_4p) + first);
  const fe sub = prm.sub[d];
  fe xw = prm.xk0;
  for (unsigned b = 0; b < prm.log_4p; ++b)
    if ((first >> b) & 1) xw = fe_mul(xw, prm.wpow[b]);
  fe run = FE_ONE_M;
  for (unsigned j = 0; j < BND_INV_K; ++j) {
    vf_store(slot + 4 * j, fe_pack(fe_canon(run)));
    run = fe_mul(run, fe_carry(fe_sub(xw, sub)));
    if (j + 1 < BND_INV_K) xw = fe_mul(xw, prm.wpow[0]);
  }
  fe inv = fe_inv(run);
  for (int j = (int)BND_INV_K - 1; j >= 0; --j) {
    const fe pre = vf_fe(slot + 4 * j);
    vf_store(slot + 4 * j, fe_pack(fe_canon(fe_mul(inv, pre))));
    inv = fe_mul(inv, fe_carry(fe_sub(xw, sub)));
    xw = fe_mul(xw, prm.winv);
  }
}
// Point j of the dense call: out[j] = (acc ? acc[j] : 0) + B(x_j).  Moved: n_terms trace felts, n_groups public felts,
// n_groups table entries at j mod 4p (the table stays in L2), optionally acc, one out.  The sum of boundary_combine
// is below 2p in magnitude, acc adds less than 32 p: fe_canon's range.  acc[j] is read before out[j] is written, so
// acc may be out.
SP_HD void boundary_dense_item(const BoundaryTerms& tm, const uint64_t* trace, size_t col_stride, const uint64_t* pub,
                               size_t M, const uint64_t* table, const uint64_t* acc, uint64_t* out, size_t j) {
  const unsigned log_4p = tm.log_period + 2;
  const size_t tj = j & (((size_t)1 << log_4p) - 1);
  fe b = boundary_combine(
      tm, [&](unsigned t) { return vf_fe(trace + 4 * ((size_t)tm.col[t] * col_stride + j)); },
      [&](unsigned d) { return vf_fe(pub + 4 * ((size_t)d * M + j)); },
      [&](unsigned d) { return vf_fe(table + 4 * (((size_t)d << log_4p) + tj)); });
  if (acc) b = fe_add(b, vf_fe(acc + 4 * j));
  vf_store(out + 4 * j, fe_pack(fe_canon(b)));
}

// ---- the points call ----
struct BoundaryPointParams {
  fe shift, w;               // Montgomery: the coset shift, the primitive M-th root of unity
  fe arg[BND_MAX_GROUPS];    // Montgomery: g^-o_d, what x is multiplied by before C_d takes it
  fe sub[BND_MAX_GROUPS];    // Montgomery: w_p^o_d
  unsigned log_n;
};
inline void boundary_point_params(const BoundaryDesc& d, unsigned log_n, const uint64_t* shift_host,
                                  BoundaryPointParams* prm) {
  prm->shift = fe_to_mont(vf_fe(shift_host));
  prm->w = verify_root_of_unity(log_n + 2);
  const fe g = verify_root_of_unity(log_n), wp = verify_root_of_unity(d.log_period);
  for (unsigned k = 0; k < BND_MAX_GROUPS; ++k) {
    const bool live = k < d.n_groups;
    prm->arg[k] = live ? fe_inv(boundary_pow(g, d.group_rows[k])) : FE_ZERO;
    prm->sub[k] = live ? boundary_pow(wp, d.group_rows[k]) : FE_ZERO;
  }
  prm->log_n = log_n;
}
// whether item i has a value at all: pos[i] below M and the n_cols felts of its row below p
SP_HD bool boundary_point_ok(unsigned log_n, unsigned n_cols, const uint64_t* pos, const uint64_t* cur, size_t i) {
  bool ok = pos[i] < ((uint64_t)4 << log_n);
  for (unsigned c = 0; c < n_cols; ++c) ok = ok & vf_is_felt(cur + 4 * ((size_t)n_cols * i + c));
  return ok;
}
// The helpers from here to boundary_point_store take plain values, not a parameter struct: hash_io.hip, the
// three-term instance written out by hand, runs its points kernel on them too (shift, w, arg and log_n are what
// BoundaryPointParams and HashIoPointParams have in common).
// x = shift w_M^pos, most significant bit first (fri_check_item's rule); shift and w Montgomery
SP_HD fe boundary_point_x(const fe& shift, const fe& w, unsigned log_n, uint64_t pos) {
  fe pw = FE_ONE_M;
  for (int bit = (int)log_n + 1; bit >= 0; --bit) {
    pw = fe_sqr(pw);
    if ((pos >> bit) & 1) pw = fe_mul(pw, w);
  }
  return fe_mul(shift, pw);
}
// Lane `lane` of a point's block, group d: y^lane * sum_m coef_d[lane + 256 m] (y^256)^m with y = x * arg, arg =
// g^-o_d (Montgomery) - the lane's share of C_d(y), Horner in y^256 from its top coefficient down.  Lanes at or above
// k hold no coefficient and return 0, so one plan serves every k from 1 up.  The running value is plain: a product
// with the Montgomery power is below p in magnitude, the coefficient adds less than 2^256, the carry pass keeps the
// limbs below 2^29.  The result is N-form with a value inside (-p, p).
SP_HD fe boundary_lane_share(unsigned log_n, unsigned log_period, const fe& arg, const uint64_t* coef, const fe& x,
                             unsigned d, unsigned lane) {
  const size_t k = (size_t)1 << (log_n - log_period);
  fe pw = fe_mul(x, arg), yl = FE_ONE_M;
  for (unsigned b = 0; b < BND_POINT_TPB_LOG; ++b) {
    if ((lane >> b) & 1) yl = fe_mul(yl, pw);
    pw = fe_sqr(pw);
  }
  if (lane >= k) return FE_ZERO;
  const uint64_t* mine = coef + 4 * ((size_t)d * k + lane);
  const size_t count = (k - lane + BND_POINT_TPB - 1) / BND_POINT_TPB;
  fe acc = vf_fe(mine + 4 * BND_POINT_TPB * (count - 1));
  for (size_t m = count - 1; m-- > 0;) acc = fe_carry(fe_add(fe_mul(acc, pw), vf_fe(mine + 4 * BND_POINT_TPB * m)));
  return fe_mul(acc, yl);
}
// the two helpers above for a caller that holds the call's own parameter struct
SP_HD fe boundary_point_x(const BoundaryPointParams& prm, uint64_t pos) {
  return boundary_point_x(prm.shift, prm.w, prm.log_n, pos);
}
SP_HD fe boundary_lane_share(const BoundaryPointParams& prm, unsigned log_period, const uint64_t* coef, const fe& x,
                             unsigned d, unsigned lane) {
  return boundary_lane_share(prm.log_n, log_period, prm.arg[d], coef, x, d, lane);
}
// one step of the block's tree: both inputs N-form inside (-p, 2p), and so is the sum
SP_HD fe boundary_share_add(const fe& a, const fe& b) { return fe_weak_reduce(fe_add(a, b)); }
// What lane 0 does with the sums.  `sums` holds C_d for d < n_groups in slots sums[d * stride] and has one free slot
// behind each, sums[d * stride + 1], which receives 1 / den_d: the denominators x^k - w_p^o_d, ONE inversion for
// their product (prefix products on the way up, the running inverse on the way down; every loop has constant bounds,
// so nothing is indexed in registers), then boundary_combine.  The sums are inside (-p, 2p), which C_d's bound above
// (below 32 p) covers.  Canonical.
SP_HD fe boundary_point_value(const BoundaryTerms& tm, const BoundaryPointParams& prm, const fe& x, const uint64_t* cur,
                              fe* sums, unsigned stride) {
  const fe xk = fe_sqr_n(x, (int)(prm.log_n - tm.log_period));
  fe run = FE_ONE_M;
  for (unsigned d = 0; d < tm.n_groups; ++d) {
    sums[d * stride + 1] = run;
    run = fe_mul(run, fe_carry(fe_sub(xk, prm.sub[d])));
  }
  fe inv = fe_inv(run);
  for (unsigned d = tm.n_groups; d-- > 0;) {
    const fe pre = sums[d * stride + 1];
    sums[d * stride + 1] = fe_canon(fe_mul(inv, pre));
    inv = fe_mul(inv, fe_carry(fe_sub(xk, prm.sub[d])));
  }
  return fe_canon(boundary_combine(
      tm, [&](unsigned t) { return vf_fe(cur + 4 * tm.col[t]); }, [&](unsigned d) { return sums[d * stride]; },
      [&](unsigned d) { return sums[d * stride + 1]; }));
}
SP_HD void boundary_point_store(bool ok, const fe& value, size_t i, uint64_t* out, uint8_t* status) {
  u256 r;
  for (int k = 0; k < 8; ++k) r.w[k] = 0;
  if (ok) r = fe_pack(value);
  vf_store(out + 4 * i, r);
  status[i] = ok ? VERIFY_OK : VERIFY_OUT_OF_RANGE;
}

}  // namespace sp
