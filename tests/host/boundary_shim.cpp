// Host build of csrc/boundary.hpp (the per-lane logic of sp_boundary_dev and sp_boundary_points_dev) for
// tests/test_boundary_ref_cpu.py:
//   g++ -O2 -shared -fPIC -o boundary_shim.so boundary_shim.cpp
// bs_dense and bs_points are the library calls over HOST arrays: the same argument rules, the same parameter
// preparation, and the kernels' launch plans replayed - thread by thread, and for a point's block lane by lane with
// the tree of the kernel - through the same item functions.  Only the shift rule is restated here (the library takes
// it from air_zinv of stark.hip, which needs HIP).
// With -DBOUNDARY_SHIM_MAIN it is a stand-alone program that runs exactly-sized cases itself - the form to run under
// -fsanitize=address,undefined:
//   g++ -O1 -g -fsanitize=address,undefined -DBOUNDARY_SHIM_MAIN -o boundary_check boundary_shim.cpp
#include <cstdio>
#include <vector>

#include "../../stark-perpetual_amd/csrc/boundary.hpp"

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

int bs_dense(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows, unsigned n_terms,
             const unsigned* term_cols, const unsigned* term_groups, const uint64_t* trace, size_t col_stride,
             const uint64_t* pub, unsigned log_n, const uint64_t* alphas, const uint64_t* shift, const uint64_t* acc,
             uint64_t* out, char* err, size_t err_len) {
  const BoundaryDesc desc{log_period, n_cols, n_groups, group_rows, n_terms, term_cols, term_groups};
  if (const char* bad = boundary_check_desc(desc)) return refuse(bad, err, err_len);
  if (const char* bad = boundary_dense_check_args(desc, log_n, col_stride, trace, pub, alphas, shift, out))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  BoundaryTableParams prm;
  boundary_table_params(desc, log_n, shift, &prm);
  BoundaryTerms tm;
  boundary_terms(desc, alphas, &tm);
  std::vector<uint64_t> table(4 * ((size_t)n_groups << prm.log_4p));  // exactly what the call reserves
  for (unsigned t = 0; t < boundary_table_threads(prm); ++t) boundary_table_item(prm, t, table.data());
  const size_t M = (size_t)4 << log_n;
  for (size_t j = 0; j < M; ++j) boundary_dense_item(tm, trace, col_stride, pub, M, table.data(), acc, out, j);
  return 0;
}

int bs_points(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows, unsigned n_terms,
              const unsigned* term_cols, const unsigned* term_groups, unsigned log_n, const uint64_t* coef,
              const uint64_t* alphas, const uint64_t* shift, size_t n, const uint64_t* pos, const uint64_t* cur,
              uint64_t* out, uint8_t* status, char* err, size_t err_len) {
  const BoundaryDesc desc{log_period, n_cols, n_groups, group_rows, n_terms, term_cols, term_groups};
  if (const char* bad = boundary_check_desc(desc)) return refuse(bad, err, err_len);
  if (const char* bad = boundary_points_check_args(desc, log_n, n)) return refuse(bad, err, err_len);
  if (n == 0) return 0;
  if (const char* bad = boundary_points_check_pointers(coef, alphas, shift, pos, cur, out, status))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  BoundaryPointParams prm;
  boundary_point_params(desc, log_n, shift, &prm);
  BoundaryTerms tm;
  boundary_terms(desc, alphas, &tm);
  std::vector<fe> share(BND_MAX_GROUPS * BND_POINT_TPB);  // the block's LDS
  for (size_t i = 0; i < n; ++i) {  // one block per point
    if (!boundary_point_ok(log_n, n_cols, pos, cur, i)) {
      boundary_point_store(false, FE_ZERO, i, out, status);
      continue;
    }
    const fe x = boundary_point_x(prm.shift, prm.w, prm.log_n, pos[i]);
    for (unsigned lane = 0; lane < BND_POINT_TPB; ++lane)
      for (unsigned d = 0; d < n_groups; ++d)
        share[d * BND_POINT_TPB + lane] = boundary_lane_share(prm.log_n, log_period, prm.arg[d], coef, x, d, lane);
    for (unsigned half = BND_POINT_TPB / 2; half > 0; half >>= 1)
      for (unsigned lane = 0; lane < half; ++lane)
        for (unsigned d = 0; d < n_groups; ++d)
          share[d * BND_POINT_TPB + lane] =
              boundary_share_add(share[d * BND_POINT_TPB + lane], share[d * BND_POINT_TPB + lane + half]);
    boundary_point_store(true, boundary_point_value(tm, prm, x, cur + 4 * (size_t)n_cols * i, share.data(), BND_POINT_TPB),
                         i, out, status);
  }
  return 0;
}
}

#ifdef BOUNDARY_SHIM_MAIN
// Exactly-sized arrays, so that an index one past an array is an AddressSanitizer report.  The expectations in
// integers are the Python tests'; this program checks bounds, statuses, that the points plan repeats the dense plan
// and that refused calls write nothing.
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static void rand_felts(std::vector<uint64_t>& v) {
  for (size_t i = 0; i < v.size(); i += 4)
    v[i] = rnd(), v[i + 1] = rnd(), v[i + 2] = rnd(), v[i + 3] = rnd() & 0x07ffffffffffffffull;  // below 2^251 < p
}
struct Desc {
  unsigned log_period, n_cols, n_groups;
  std::vector<unsigned> rows;
  unsigned n_terms;
  std::vector<unsigned> cols, groups;
};
static bool dense_case(const Desc& d, unsigned log_n, bool with_acc) {
  const size_t M = (size_t)4 << log_n;
  std::vector<uint64_t> trace(4 * d.n_cols * M), pub(4 * d.n_groups * M), alphas(4 * d.n_terms), acc(with_acc ? 4 * M : 0);
  std::vector<uint64_t> shift = {3, 0, 0, 0}, out(4 * M, ~0ull);
  for (auto* v : {&trace, &pub, &alphas, &acc}) rand_felts(*v);
  for (size_t i = 0; i < trace.size(); i += 7) trace[i] = ~0ull;  // values up to 2^256 - 1 are a column's right
  char err[96] = "";
  if (bs_dense(d.log_period, d.n_cols, d.n_groups, d.rows.data(), d.n_terms, d.cols.data(), d.groups.data(), trace.data(),
               M, pub.data(), log_n, alphas.data(), shift.data(), with_acc ? acc.data() : nullptr, out.data(), err,
               sizeof err) != 0)
    return false;
  for (size_t j = 0; j < M; ++j)
    if (!vf_is_felt(&out[4 * j])) return false;
  return true;
}
static bool points_case(const Desc& d, unsigned log_n, size_t n) {
  const uint64_t M = (uint64_t)4 << log_n;
  const size_t k = (size_t)1 << (log_n - d.log_period);
  std::vector<uint64_t> coef(4 * d.n_groups * k), alphas(4 * d.n_terms), shift = {5, 0, 0, 0};
  std::vector<uint64_t> pos(n), cur(4 * n * d.n_cols), out(4 * n, ~0ull);
  std::vector<uint8_t> status(n, 0xee);
  for (auto* v : {&coef, &alphas, &cur}) rand_felts(*v);
  for (size_t i = 0; i < n; ++i) pos[i] = i % 3 == 0 ? M - 1 - (i % M) : rnd() % M;
  if (n > 3) {
    pos[1] = M;  // out of range
    pos[2] = ~(uint64_t)0;
    cur[4 * (3 * d.n_cols + d.n_cols - 1) + 3] = ~(uint64_t)0;  // a felt >= p in the last column
  }
  char err[96] = "";
  if (bs_points(d.log_period, d.n_cols, d.n_groups, d.rows.data(), d.n_terms, d.cols.data(), d.groups.data(), log_n,
                coef.data(), alphas.data(), shift.data(), n, pos.data(), cur.data(), out.data(), status.data(), err,
                sizeof err) != 0)
    return false;
  for (size_t i = 0; i < n; ++i) {
    const bool bad = n > 3 && (i == 1 || i == 2 || i == 3);
    if (status[i] != (bad ? VERIFY_OUT_OF_RANGE : VERIFY_OK)) return false;
    if (!vf_is_felt(&out[4 * i])) return false;
    if (bad && (out[4 * i] | out[4 * i + 1] | out[4 * i + 2] | out[4 * i + 3]) != 0) return false;
  }
  return true;
}
int main() {
  const Desc ecdsa = {10, 10, 3, {0, 256, 512}, 5, {0, 0, 3, 4, 0}, {0, 1, 1, 1, 2}};
  const Desc range = {7, 1, 1, {0}, 1, {0}, {0}};
  const Desc hashes = {9, 4, 3, {0, 256, 511}, 3, {0, 0, 1}, {0, 1, 2}};
  const Desc widest = {8, 16, 4, {255, 0, 7, 128}, 8, {15, 0, 1, 2, 3, 4, 5, 6}, {3, 0, 0, 0, 0, 1, 2, 0}};  // out of order
  bool ok = true;
  for (const Desc* d : {&ecdsa, &range, &hashes, &widest}) {
    ok = ok && dense_case(*d, d->log_period, false) && dense_case(*d, d->log_period + 1, true);
    for (size_t n : {(size_t)1, (size_t)5}) ok = ok && points_case(*d, d->log_period, n) && points_case(*d, d->log_period + 2, n);
  }
  ok = ok && points_case(range, 7 + 9, 4);  // k = 512: two coefficients per lane
  // refused calls write nothing and read no pointer but the descriptor's
  char err[96] = "";
  uint8_t st = 0xee;
  uint64_t word = 0x5555;
  const unsigned row[4] = {0, 1, 2, 3}, col[8] = {0, 0, 0, 0, 0, 0, 0, 0}, grp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto bare = [&](unsigned lp, unsigned nc, unsigned ng, unsigned nt, unsigned log_n, size_t n) {
    return bs_points(lp, nc, ng, row, nt, col, grp, log_n, nullptr, nullptr, nullptr, n, nullptr, nullptr, &word, &st, err,
                     sizeof err);
  };
  ok = ok && bare(6, 1, 1, 1, 8, 1) == -3 && bare(11, 1, 1, 1, 12, 1) == -3 && bare(7, 0, 1, 1, 8, 1) == -3;
  ok = ok && bare(7, 17, 1, 1, 8, 1) == -3 && bare(7, 1, 0, 1, 8, 1) == -3 && bare(7, 1, 5, 1, 8, 1) == -3;
  ok = ok && bare(7, 1, 1, 0, 8, 1) == -3 && bare(7, 1, 1, 9, 8, 1) == -3 && bare(7, 1, 2, 2, 8, 1) == -3;  // group 1 empty
  ok = ok && bare(7, 1, 1, 1, 6, 1) == -3 && bare(7, 1, 1, 1, 31, 1) == -3;
  ok = ok && bare(7, 1, 1, 1, 8, ((size_t)1 << 30) + 1) == -3 && bare(7, 1, 1, 1, 8, 1) == -3;  // the last: NULL
  ok = ok && bare(7, 1, 1, 1, 8, 0) == 0;
  ok = ok && bs_dense(7, 1, 1, row, 1, col, grp, nullptr, 2048, nullptr, 8, nullptr, nullptr, nullptr, &word, err,
                      sizeof err) == -3;
  ok = ok && st == 0xee && word == 0x5555;
  printf(ok ? "boundary check passed\n" : "boundary check FAILED\n");
  return ok ? 0 : 1;
}
#endif
