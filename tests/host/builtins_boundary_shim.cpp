// Host build of csrc/builtins_boundary.hpp (the per-lane logic of sp_boundary_combine_dev, sp_builtins_boundary_dev
// and sp_builtins_boundary_points_dev) for tests/test_builtins_io_ref_cpu.py:
//   g++ -O2 -shared -fPIC -o builtins_boundary_shim.so builtins_boundary_shim.cpp
// bbs_combine, bbs_dense and bbs_points are the library calls over HOST arrays: the same argument rules, the same
// parameter preparation, and the kernels' launch plans replayed - thread by thread, and for a point's block lane by
// lane, segment after segment, with the tree of the kernel - through the same item functions.  Only the shift rule is
// restated here (the library takes it from air_zinv of stark.hip, which needs HIP).
// With -DBUILTINS_BOUNDARY_SHIM_MAIN it is a stand-alone program that runs exactly-sized cases itself - the form to
// run under -fsanitize=address,undefined:
//   g++ -O1 -g -fsanitize=address,undefined -DBUILTINS_BOUNDARY_SHIM_MAIN -o bb_check builtins_boundary_shim.cpp
#include <cstdio>
#include <vector>

#include "../../stark-perpetual_amd/csrc/builtins_boundary.hpp"

using namespace sp;

static int refuse(const char* bad, char* err, size_t err_len) {
  if (err && err_len) snprintf(err, err_len, "%s", bad);
  return -3;  // SP_ERR_BAD_ARGUMENT
}
// shift below p, not 0, shift^(4n) != 1
static bool shift_ok(const uint64_t* shift, unsigned log_n) {
  if (!vf_is_felt(shift)) return false;
  const fe s = fe_to_mont(vf_fe(shift));
  return !fe_is_zero(s) && !fe_eq(fe_sqr_n(s, (int)log_n + 2), FE_ONE_M);
}

extern "C" {

int bbs_combine(unsigned n_groups, unsigned n_terms, const unsigned* term_groups, const uint64_t* const* values, size_t k,
                const uint64_t* alphas, uint64_t* out, char* err, size_t err_len) {
  if (const char* bad = bb_combine_check_args(n_groups, n_terms, term_groups, values, k, alphas, out))
    return refuse(bad, err, err_len);
  BbCombineParams cp;
  bb_combine_params(n_groups, n_terms, term_groups, values, alphas, &cp);
  for (size_t i = 0; i < k; ++i) bb_combine_item(cp, k, out, i);
  return 0;
}

int bbs_dense(unsigned segments, unsigned log_n, const uint64_t* trace, size_t col_stride, const uint64_t* pub,
              const uint64_t* alphas, const uint64_t* shift, const uint64_t* acc, uint64_t* out, char* err,
              size_t err_len) {
  if (const char* bad = bb_dense_check_args(segments, log_n, col_stride, trace, pub, alphas, shift, out))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  BbTableParams tp;
  BbDenseParams dp;
  bb_dense_params(segments, log_n, alphas, shift, &tp, &dp);
  std::vector<uint64_t> table(4 * (size_t)tp.n_felts);  // exactly what the call reserves
  for (unsigned t = 0; t < tp.n_threads; ++t) bb_table_item(tp, t, table.data());
  const size_t M = (size_t)4 << log_n;
  for (size_t j = 0; j < M; ++j) bb_dense_item(dp, trace, col_stride, pub, M, table.data(), acc, out, j);
  return 0;
}

int bbs_points(unsigned segments, unsigned log_n, const uint64_t* coef, const uint64_t* alphas, const uint64_t* shift,
               size_t n, const uint64_t* pos, const uint64_t* cur, uint64_t* out, uint8_t* status, char* err,
               size_t err_len) {
  if (const char* bad = bb_points_check_args(segments, log_n, n)) return refuse(bad, err, err_len);
  if (n == 0) return 0;
  if (const char* bad = boundary_points_check_pointers(coef, alphas, shift, pos, cur, out, status))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  BbPointParams pp;
  bb_point_params(segments, log_n, alphas, shift, &pp);
  std::vector<fe> share(BND_MAX_GROUPS * BND_POINT_TPB);  // the block's LDS
  for (size_t i = 0; i < n; ++i) {  // one block per point
    if (!boundary_point_ok(pp.log_n, pp.n_cols, pos, cur, i)) {
      boundary_point_store(false, FE_ZERO, i, out, status);
      continue;
    }
    const fe x = boundary_point_x(pp.seg[0].prm.shift, pp.seg[0].prm.w, pp.log_n, pos[i]);
    fe total = FE_ZERO;
    for (unsigned s = 0; s < pp.n_segs; ++s) {
      const BbPointSeg& sg = pp.seg[s];
      for (unsigned lane = 0; lane < BND_POINT_TPB; ++lane)
        for (unsigned d = 0; d < sg.tm.n_groups; ++d)
          share[d * BND_POINT_TPB + lane] =
              boundary_lane_share(pp.log_n, sg.tm.log_period, sg.prm.arg[d], coef + 4 * sg.coef0, x, d, lane);
      for (unsigned half = BND_POINT_TPB / 2; half > 0; half >>= 1)
        for (unsigned lane = 0; lane < half; ++lane)
          for (unsigned d = 0; d < sg.tm.n_groups; ++d)
            share[d * BND_POINT_TPB + lane] =
                boundary_share_add(share[d * BND_POINT_TPB + lane], share[d * BND_POINT_TPB + lane + half]);
      total = fe_add(total, bb_point_segment_value(sg, x, cur + 4 * (size_t)pp.n_cols * i, share.data(), BND_POINT_TPB));
    }
    boundary_point_store(true, fe_canon(total), i, out, status);
  }
  return 0;
}
}

#ifdef BUILTINS_BOUNDARY_SHIM_MAIN
// Exactly-sized arrays, so that an index one past an array is an AddressSanitizer report.  The expectations in
// integers are the Python tests'; this program checks bounds, statuses and that refused calls write nothing.
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static void rand_felts(std::vector<uint64_t>& v) {
  for (size_t i = 0; i < v.size(); i += 4)
    v[i] = rnd(), v[i + 1] = rnd(), v[i + 2] = rnd(), v[i + 3] = rnd() & 0x07ffffffffffffffull;  // below 2^251 < p
}
struct Shape {
  unsigned n_cols = 0, n_groups = 0, n_terms = 0, min_log_n = 0;
  size_t coef(unsigned log_n, unsigned segments) const {
    size_t c = 0;
    for (const auto& s : BB_SEGMENTS)
      if (segments & s.bit) c += (size_t)s.n_groups << (log_n - s.log_period);
    return c;
  }
};
static Shape shape_of(unsigned segments) {
  Shape sh;
  for (const auto& s : BB_SEGMENTS)
    if (segments & s.bit) {
      sh.n_cols += s.n_cols, sh.n_groups += s.n_groups, sh.n_terms += s.n_terms;
      if (s.log_period > sh.min_log_n) sh.min_log_n = s.log_period;
    }
  return sh;
}
static bool dense_case(unsigned segments, unsigned log_n, int acc_mode /* 0 none, 1 separate, 2 in place */) {
  const Shape sh = shape_of(segments);
  const size_t M = (size_t)4 << log_n;
  std::vector<uint64_t> trace(4 * sh.n_cols * M), pub(4 * sh.n_groups * M), alphas(4 * sh.n_terms), acc(acc_mode ? 4 * M : 0);
  std::vector<uint64_t> shift = {3, 0, 0, 0}, out(4 * M, ~0ull);
  for (auto* v : {&trace, &pub, &alphas, &acc}) rand_felts(*v);
  for (size_t i = 0; i < trace.size(); i += 7) trace[i] = ~0ull;  // values up to 2^256 - 1 are a column's right
  char err[128] = "";
  uint64_t* dst = acc_mode == 2 ? acc.data() : out.data();
  if (bbs_dense(segments, log_n, trace.data(), M, pub.data(), alphas.data(), shift.data(), acc_mode ? acc.data() : nullptr,
                dst, err, sizeof err) != 0)
    return false;
  for (size_t j = 0; j < M; ++j)
    if (!vf_is_felt(&dst[4 * j])) return false;
  return true;
}
static bool points_case(unsigned segments, unsigned log_n, size_t n) {
  const Shape sh = shape_of(segments);
  const uint64_t M = (uint64_t)4 << log_n;
  std::vector<uint64_t> coef(4 * sh.coef(log_n, segments)), alphas(4 * sh.n_terms), shift = {5, 0, 0, 0};
  std::vector<uint64_t> pos(n), cur(4 * n * sh.n_cols), out(4 * n, ~0ull);
  std::vector<uint8_t> status(n, 0xee);
  for (auto* v : {&coef, &alphas, &cur}) rand_felts(*v);
  for (size_t i = 0; i < n; ++i) pos[i] = i % 3 == 0 ? M - 1 - (i % M) : rnd() % M;
  if (n > 3) {
    pos[1] = M;  // out of range
    pos[2] = ~(uint64_t)0;
    cur[4 * (3 * sh.n_cols + sh.n_cols - 1) + 3] = ~(uint64_t)0;  // a felt >= p in the last column
  }
  char err[128] = "";
  if (bbs_points(segments, log_n, coef.data(), alphas.data(), shift.data(), n, pos.data(), cur.data(), out.data(),
                 status.data(), err, sizeof err) != 0)
    return false;
  for (size_t i = 0; i < n; ++i) {
    const bool bad = n > 3 && (i == 1 || i == 2 || i == 3);
    if (status[i] != (bad ? VERIFY_OUT_OF_RANGE : VERIFY_OK)) return false;
    if (!vf_is_felt(&out[4 * i])) return false;
    if (bad && (out[4 * i] | out[4 * i + 1] | out[4 * i + 2] | out[4 * i + 3]) != 0) return false;
  }
  return true;
}
static bool combine_case(unsigned n_groups, std::vector<unsigned> groups, size_t k) {
  const unsigned n_terms = (unsigned)groups.size();
  std::vector<std::vector<uint64_t>> cols(n_terms, std::vector<uint64_t>(4 * k));
  std::vector<const uint64_t*> ptr;
  for (auto& c : cols) {
    rand_felts(c);
    c[4 * (k - 1) + 3] = ~0ull;  // any 256-bit value
    ptr.push_back(c.data());
  }
  std::vector<uint64_t> alphas(4 * n_terms), out(4 * n_groups * k, ~0ull);
  rand_felts(alphas);
  char err[128] = "";
  if (bbs_combine(n_groups, n_terms, groups.data(), ptr.data(), k, alphas.data(), out.data(), err, sizeof err) != 0)
    return false;
  for (size_t j = 0; j < n_groups * k; ++j)
    if (!vf_is_felt(&out[4 * j])) return false;
  return true;
}
int main() {
  bool ok = true;
  for (unsigned segments = 1; segments <= 7; ++segments) {
    const unsigned lo = shape_of(segments).min_log_n;
    ok = ok && dense_case(segments, lo, 0) && dense_case(segments, lo + 1, 1) && dense_case(segments, lo, 2);
    for (size_t n : {(size_t)1, (size_t)5}) ok = ok && points_case(segments, lo, n) && points_case(segments, lo + 1, n);
  }
  ok = ok && points_case(BSEG_RC16, 3 + 9, 4);  // k = 512: two coefficients per lane
  ok = ok && combine_case(1, {0}, 1) && combine_case(3, {0, 1, 1, 1, 2}, 5) && combine_case(4, {3, 0, 0, 0, 0, 1, 2, 0}, 300);
  // refused calls write nothing and read no pointer
  char err[128] = "";
  uint8_t st = 0xee;
  uint64_t word = 0x5555;
  auto bare = [&](unsigned segments, unsigned log_n, size_t n) {
    return bbs_points(segments, log_n, nullptr, nullptr, nullptr, n, nullptr, nullptr, &word, &st, err, sizeof err);
  };
  ok = ok && bare(0, 10, 1) == -3 && bare(8, 10, 1) == -3 && bare(1, 8, 1) == -3 && bare(2, 9, 1) == -3;
  ok = ok && bare(4, 2, 1) == -3 && bare(5, 8, 1) == -3 && bare(4, 25, 1) == -3 && bare(3, 31, 1) == -3;
  ok = ok && bare(7, 10, ((size_t)1 << 30) + 1) == -3 && bare(7, 10, 1) == -3;  // the last: NULL
  ok = ok && bare(7, 10, 0) == 0;
  ok = ok && bbs_dense(7, 10, nullptr, 4096, nullptr, nullptr, nullptr, nullptr, &word, err, sizeof err) == -3;
  ok = ok && bbs_dense(4, 25, &word, (size_t)1 << 28, &word, &word, &word, nullptr, &word, err, sizeof err) == -3;
  const unsigned grp[2] = {0, 0};
  ok = ok && bbs_combine(2, 2, grp, nullptr, 1, nullptr, &word, err, sizeof err) == -3;  // group 1 empty
  ok = ok && bbs_combine(1, 9, grp, nullptr, 1, nullptr, &word, err, sizeof err) == -3;
  ok = ok && st == 0xee && word == 0x5555;
  printf(ok ? "builtins boundary check passed\n" : "builtins boundary check FAILED\n");
  return ok ? 0 : 1;
}
#endif
