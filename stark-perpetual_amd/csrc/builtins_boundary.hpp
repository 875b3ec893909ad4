// Boundary constraints for the COMBINED builtin trace (sp_boundary_combine_dev, sp_builtins_boundary_dev,
// sp_builtins_boundary_points_dev): the segment table, the argument rules, the parameter preparation
// and everything a lane of the kernels of builtins_boundary.hip does.  Like boundary.hpp, on which it is built,
// nothing here needs HIP: a plain C++ compiler builds it for tests/host/builtins_boundary_shim.cpp, which replays the
// launch plans over host arrays.
//
// The statement.  A combined trace lays the present segments - pedersen, ecdsa, rc16 - side by side (4 + 10 + 3
// columns), each with its own period p_s (512, 1024, 8) and k_s = n / p_s instances.  Every segment brings the groups
// and terms of its descriptor, columns relative to its first column, and
//   B(x) = sum_s sum_{d in s} ( sum_{t in d} a_t col_{c0_s + c_t}(x) - C_d(x g^-o_d) ) / (x^k_s - w_{p_s}^o_d):
// the sum over ALL groups of the quotient of boundary.hpp, each with its own segment's p and k.  A segment is a
// BoundaryDesc plus its first column and first group, so the arithmetic is boundary_combine, the tables are
// boundary_table_item's and a point's share is boundary_lane_share - per segment, through one set of launches.
#pragma once
#include "boundary.hpp"
#include "verify_builtins.hpp"

namespace sp {

// ---- the segments, in the column order of a combined trace: another segment costs an entry ----
struct BuiltinsBoundarySegment {
  unsigned bit;  // BSEG_*
  unsigned log_period, n_cols, n_groups;
  unsigned group_rows[BND_MAX_GROUPS];
  unsigned n_terms;
  unsigned term_cols[BND_MAX_TERMS], term_groups[BND_MAX_TERMS];
};
constexpr BuiltinsBoundarySegment BB_SEGMENTS[BSEG_MAX] = {
    {BSEG_PEDERSEN, 9, 4, 3, {0, 256, 511}, 3, {0, 0, 1}, {0, 1, 2}},              // s = x | s = y | px = h
    {BSEG_ECDSA, 10, 10, 3, {0, 256, 512}, 5, {0, 0, 3, 4, 0}, {0, 1, 1, 1, 2}},  // m = z | m = r, qx, qy | m = w
    {BSEG_RC16, 3, RC16_N_COLS, 1, {7}, 1, {1}, {0}},                              // acc = value at a value's last limb
};
constexpr unsigned BB_MAX_GROUPS = 7, BB_MAX_TERMS = 9;  // 3 + 3 + 1 and 3 + 5 + 1 of the table above
constexpr unsigned BB_MAX_LOG_K = 30;                    // sp_boundary_combine_dev: felts of a column
constexpr unsigned BB_COMBINE_TPB = 256;

inline BoundaryDesc bb_desc(const BuiltinsBoundarySegment& s) {
  return BoundaryDesc{s.log_period, s.n_cols, s.n_groups, s.group_rows, s.n_terms, s.term_cols, s.term_groups};
}

// ---- argument rules: nullptr, or the text for sp_last_error ----
inline const char* bb_check_segments(unsigned segments) {
  if (segments < 1 || segments > BSEG_ALL) return "segments outside 1 .. 7 (SP_SEG_PEDERSEN | SP_SEG_ECDSA | SP_SEG_RC16)";
  return nullptr;
}
inline const char* bb_dense_check_args(unsigned segments, unsigned log_n, size_t col_stride, const void* trace_lde,
                                       const void* pub_lde, const void* alphas_host, const void* shift_host,
                                       const void* out) {
  if (const char* bad = bb_check_segments(segments)) return bad;
  if (log_n < builtins_shape(segments).min_log_n || log_n > BND_DENSE_MAX_LOG_N)
    return "log_n out of range (the largest minimum of the segments .. 24)";
  if (col_stride < ((size_t)4 << log_n)) return "col_stride below 4 * 2^log_n";
  if (!trace_lde) return "trace_lde is NULL";
  if (!pub_lde) return "pub_lde is NULL";
  if (!alphas_host) return "alphas_host is NULL";
  if (!shift_host) return "shift_host is NULL";
  if (!out) return "out is NULL";
  return nullptr;
}
inline const char* bb_points_check_args(unsigned segments, unsigned log_n, size_t n_points) {
  if (const char* bad = bb_check_segments(segments)) return bad;
  const BuiltinsShape sh = builtins_shape(segments);
  if (log_n < sh.min_log_n || log_n > sh.max_log_n)
    return "log_n out of range (the largest minimum of the segments .. 30, 24 with rc16)";
  if (n_points > VERIFY_MAX_ITEMS) return "n_points above 2^30";
  return nullptr;
}
// the pointer rule of the points call is boundary_points_check_pointers

inline const char* bb_combine_check_args(unsigned n_groups, unsigned n_terms, const unsigned* term_groups,
                                         const uint64_t* const* values_host, size_t k, const void* alphas_host,
                                         const void* out) {
  if (n_groups < 1 || n_groups > BND_MAX_GROUPS) return "n_groups out of range (1 .. 4)";
  if (n_terms < 1 || n_terms > BND_MAX_TERMS) return "n_terms out of range (1 .. 8)";
  if (!term_groups) return "term_groups is NULL";
  unsigned used = 0;
  for (unsigned t = 0; t < n_terms; ++t) {
    if (term_groups[t] >= n_groups) return "term_groups holds a group at or above n_groups";
    used |= 1u << term_groups[t];
  }
  if (used != (1u << n_groups) - 1) return "term_groups leaves a group without a term";
  if (k < 1 || k > ((size_t)1 << BB_MAX_LOG_K)) return "k out of range (1 .. 2^30)";
  if (!values_host) return "values_host is NULL";
  for (unsigned t = 0; t < n_terms; ++t)
    if (!values_host[t]) return "values_host holds a NULL column";
  if (!alphas_host) return "alphas_host is NULL";
  if (!out) return "out is NULL";
  return nullptr;
}

// ---- sp_boundary_combine_dev: out[d][i] = sum_{t in d} a_t v_t[i] mod p ----
struct BbCombineParams {
  fe alpha[BND_MAX_TERMS];              // Montgomery, ordered by group
  const uint64_t* v[BND_MAX_TERMS];     // the terms' columns in the same order
  unsigned first[BND_MAX_GROUPS + 1];   // the terms of group d are first[d] .. first[d + 1] - 1
  unsigned n_groups;
};
inline void bb_combine_params(unsigned n_groups, unsigned n_terms, const unsigned* term_groups,
                              const uint64_t* const* values_host, const uint64_t* alphas_host, BbCombineParams* cp) {
  unsigned at = 0;
  for (unsigned g = 0; g < BND_MAX_GROUPS; ++g) {
    cp->first[g] = at;
    for (unsigned t = 0; g < n_groups && t < n_terms; ++t)
      if (term_groups[t] == g) {
        cp->alpha[at] = fe_to_mont(vf_fe(alphas_host + 4 * t));
        cp->v[at++] = values_host[t];
      }
  }
  cp->first[BND_MAX_GROUPS] = at;
  for (; at < BND_MAX_TERMS; ++at) cp->alpha[at] = FE_ZERO, cp->v[at] = nullptr;
  cp->n_groups = n_groups;
}
// Item i < k.  AT MOST THREE PRODUCTS SHARE A REDUCTION - the inner bound of boundary_combine: a_t is N-form, a plain
// 256-bit value has limbs below 2^29 (27 * 2^58 < 2^63 per column), a run's fe_reduce lies inside (-p, p / 8); a
// group of eight terms is three runs, whose fe_add has limbs below 3 * 2^29 and a value inside (-3p, 3p / 8):
// fe_canon's range (|value| < 2^261).  Canonical, so equal to the integers' sum mod p bit for bit.
SP_HD void bb_combine_item(const BbCombineParams& cp, size_t k, uint64_t* out, size_t i) {
  for (unsigned d = 0; d < cp.n_groups; ++d) {
    fe u = FE_ZERO;
    for (unsigned t = cp.first[d]; t < cp.first[d + 1]; t += 3) {
      cols inner;
      cols_zero(inner);
      for (unsigned a = t; a < t + 3 && a < cp.first[d + 1]; ++a) cols_mac(inner, cp.alpha[a], vf_fe(cp.v[a] + 4 * i));
      u = fe_add(u, fe_reduce(inner));
    }
    vf_store(out + 4 * ((size_t)d * k + i), fe_pack(fe_canon(u)));
  }
}

// ---- what the kernels get of a checked mask: per present segment the checked descriptor's parameters of boundary.hpp
// and where the segment's columns, groups, table entries and coefficients start ----
struct BbDenseSeg {
  BoundaryTerms tm;
  unsigned col0, group0;  // first column of trace_lde, first column of pub_lde
  unsigned table0;        // first felt of the segment's n_groups x 4p table entries
};
struct BbDenseParams {
  BbDenseSeg seg[BSEG_MAX];
  unsigned n_segs;
};
struct BbTableParams {
  BoundaryTableParams prm[BSEG_MAX];
  unsigned table0[BSEG_MAX];
  unsigned n_segs, n_threads, n_felts;  // threads of the build, felts of the whole table
};
inline void bb_dense_params(unsigned segments, unsigned log_n, const uint64_t* alphas_host, const uint64_t* shift_host,
                            BbTableParams* tp, BbDenseParams* dp) {
  unsigned n = 0, col0 = 0, group0 = 0, term0 = 0, table0 = 0, threads = 0;
  for (unsigned e = 0; e < BSEG_MAX; ++e) {
    const BuiltinsBoundarySegment& sg = BB_SEGMENTS[e];
    if (!(segments & sg.bit)) continue;
    const BoundaryDesc desc = bb_desc(sg);
    boundary_table_params(desc, log_n, shift_host, &tp->prm[n]);
    boundary_terms(desc, alphas_host + 4 * term0, &dp->seg[n].tm);
    tp->table0[n] = dp->seg[n].table0 = table0;
    dp->seg[n].col0 = col0, dp->seg[n].group0 = group0;
    col0 += sg.n_cols, group0 += sg.n_groups, term0 += sg.n_terms;
    table0 += sg.n_groups << (sg.log_period + 2);
    threads += boundary_table_threads(tp->prm[n]);
    ++n;
  }
  for (unsigned e = n; e < BSEG_MAX; ++e) {  // never read: the loops stop at n_segs
    tp->prm[e] = tp->prm[0], tp->table0[e] = 0;
    dp->seg[e] = dp->seg[0];
  }
  tp->n_segs = dp->n_segs = n;
  tp->n_threads = threads, tp->n_felts = table0;
}
// Thread t < n_threads of the ONE table build: the segments' threads stand one after the other, each segment's share
// is boundary_table_item on its own part of the table (3 * 2048 + 3 * 4096 + 32 felts at most).  4p is a multiple of
// BND_INV_K for every segment (the smallest, rc16, has 4p = 32), so a thread's entries belong to one group.
SP_HD void bb_table_item(const BbTableParams& tp, unsigned t, uint64_t* table) {
  for (unsigned s = 0; s < tp.n_segs; ++s) {
    const unsigned mine = boundary_table_threads(tp.prm[s]);
    if (t < mine) {
      boundary_table_item(tp.prm[s], t, table + 4 * (size_t)tp.table0[s]);
      return;
    }
    t -= mine;
  }
}
// Point j of the dense call: out[j] = (acc ? acc[j] : 0) + B(x_j).  Per segment boundary_combine over the segment's
// own columns, public felts and table entries at j mod 4 p_s.  RANGES: a segment has at most three groups, so its
// boundary_combine is ONE outer run: N-form, inside (-p / 8, p / 8) (boundary.hpp states (-2p, 2p) for any
// descriptor).  Each partial sum goes through fe_carry, so no limb leaves 29 bits whatever the number of segments;
// three segments stay inside (-6p, 6p), acc (any 256-bit value) adds less than 32 p: |value| < 38 p, far inside
// fe_canon's range of |value| < 2^261 = 1024 p.  acc[j] is read before out[j] is written, so acc may be out.
SP_HD void bb_dense_item(const BbDenseParams& dp, const uint64_t* trace, size_t col_stride, const uint64_t* pub, size_t M,
                         const uint64_t* table, const uint64_t* acc, uint64_t* out, size_t j) {
  fe b = FE_ZERO;
  for (unsigned s = 0; s < dp.n_segs; ++s) {
    const BbDenseSeg& sg = dp.seg[s];
    const unsigned log_4p = sg.tm.log_period + 2;
    const size_t tj = j & (((size_t)1 << log_4p) - 1);
    const fe part = boundary_combine(
        sg.tm, [&](unsigned t) { return vf_fe(trace + 4 * ((size_t)(sg.col0 + sg.tm.col[t]) * col_stride + j)); },
        [&](unsigned d) { return vf_fe(pub + 4 * ((size_t)(sg.group0 + d) * M + j)); },
        [&](unsigned d) { return vf_fe(table + 4 * ((size_t)sg.table0 + ((size_t)d << log_4p) + tj)); });
    b = fe_carry(fe_add(b, part));
  }
  if (acc) b = fe_add(b, vf_fe(acc + 4 * j));
  vf_store(out + 4 * j, fe_pack(fe_canon(b)));
}

// ---- the points call ----
struct BbPointSeg {
  BoundaryTerms tm;
  BoundaryPointParams prm;
  unsigned col0;  // first felt of the opened row
  size_t coef0;   // first felt of the segment's n_groups x k_s coefficients
};
struct BbPointParams {
  BbPointSeg seg[BSEG_MAX];
  unsigned n_segs, n_cols, log_n;  // n_cols: felts of a whole opened phase-1 row
};
inline void bb_point_params(unsigned segments, unsigned log_n, const uint64_t* alphas_host, const uint64_t* shift_host,
                            BbPointParams* pp) {
  unsigned n = 0, col0 = 0, term0 = 0;
  size_t coef0 = 0;
  for (unsigned e = 0; e < BSEG_MAX; ++e) {
    const BuiltinsBoundarySegment& sg = BB_SEGMENTS[e];
    if (!(segments & sg.bit)) continue;
    const BoundaryDesc desc = bb_desc(sg);
    boundary_point_params(desc, log_n, shift_host, &pp->seg[n].prm);
    boundary_terms(desc, alphas_host + 4 * term0, &pp->seg[n].tm);
    pp->seg[n].col0 = col0, pp->seg[n].coef0 = coef0;
    col0 += sg.n_cols, term0 += sg.n_terms;
    coef0 += (size_t)sg.n_groups << (log_n - sg.log_period);
    ++n;
  }
  for (unsigned e = n; e < BSEG_MAX; ++e) pp->seg[e] = pp->seg[0];  // never read
  pp->n_segs = n, pp->n_cols = col0, pp->log_n = log_n;
}
// A point's block runs the segments one after the other through the same shares: per segment every lane's
// boundary_lane_share per group, the tree of boundary_share_add, then lane 0's bb_point_segment_value, and a barrier
// before the next segment overwrites the shares (lane 0 keeps 1 / den_d in slot 1 of each row meanwhile).  Lane 0's
// running sum adds canonical values: at most three, limbs below 3 * 2^29, below 3 p - fe_canon's range.
SP_HD fe bb_point_segment_value(const BbPointSeg& sg, const fe& x, const uint64_t* row, fe* sums, unsigned stride) {
  return boundary_point_value(sg.tm, sg.prm, x, row + 4 * sg.col0, sums, stride);
}

}  // namespace sp
