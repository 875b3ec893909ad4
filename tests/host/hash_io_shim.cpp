// Host build of csrc/hash_io.hpp (the per-lane logic of sp_hash_io_boundary_dev and sp_hash_io_boundary_points_dev)
// for tests/test_hash_io_ref_cpu.py:
//   g++ -O2 -shared -fPIC -o hash_io_shim.so hash_io_shim.cpp
// hs_dense and hs_points are the library calls over HOST arrays: the same argument rules, the same parameter
// preparation, and the kernels' launch plans replayed - thread by thread, and for a point's block lane by lane with
// the tree of the kernel - through the same item functions.  Only the shift rule is restated here (the library takes
// it from air_zinv of stark.hip, which needs HIP).
#include <cstdio>
#include <vector>

#include "../../stark-perpetual_amd/csrc/hash_io.hpp"

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

int hs_dense(const uint64_t* trace, size_t col_stride, const uint64_t* pub, unsigned log_n, const uint64_t* alphas,
             const uint64_t* shift, const uint64_t* acc, uint64_t* out, char* err, size_t err_len) {
  if (const char* bad = hash_io_dense_check_args(log_n, col_stride, trace, pub, alphas, shift, out))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  std::vector<uint64_t> table(4 * 3 * HIO_PERIOD);
  HashIoTableParams prm;
  hash_io_table_params(log_n, alphas, shift, &prm);
  for (unsigned t = 0; t < HIO_TABLE_THREADS; ++t) hash_io_table_item(prm, t, table.data());
  const size_t M = (size_t)4 << log_n;
  for (size_t j = 0; j < M; ++j) hash_io_dense_item(trace, col_stride, pub, M, table.data(), acc, out, j);
  return 0;
}

int hs_points(unsigned log_n, const uint64_t* coef, const uint64_t* alphas, const uint64_t* shift, size_t n,
              const uint64_t* pos, const uint64_t* cur, uint64_t* out, uint8_t* status, char* err, size_t err_len) {
  if (const char* bad = hash_io_points_check_args(log_n, n)) return refuse(bad, err, err_len);
  if (n == 0) return 0;
  if (const char* bad = boundary_points_check_pointers(coef, alphas, shift, pos, cur, out, status))
    return refuse(bad, err, err_len);
  if (!shift_ok(shift, log_n)) return refuse("bad shift", err, err_len);
  HashIoPointParams prm;
  hash_io_point_params(log_n, alphas, shift, &prm);
  std::vector<fe> share(3 * HIO_POINT_TPB);
  for (size_t i = 0; i < n; ++i) {  // one block per point
    if (!hash_io_point_ok(log_n, pos, cur, i)) {
      boundary_point_store(false, FE_ZERO, i, out, status);
      continue;
    }
    const fe x = boundary_point_x(prm.shift, prm.w, prm.log_n, pos[i]);
    for (unsigned lane = 0; lane < HIO_POINT_TPB; ++lane)
      for (unsigned c = 0; c < 3; ++c)
        share[c * HIO_POINT_TPB + lane] = boundary_lane_share(prm.log_n, 9, prm.arg[c], coef, x, c, lane);
    for (unsigned half = HIO_POINT_TPB / 2; half > 0; half >>= 1)
      for (unsigned lane = 0; lane < half; ++lane)
        for (unsigned c = 0; c < 3; ++c)
          share[c * HIO_POINT_TPB + lane] =
              boundary_share_add(share[c * HIO_POINT_TPB + lane], share[c * HIO_POINT_TPB + lane + half]);
    boundary_point_store(true, hash_io_point_value(prm, x, cur + 16 * i, share[0], share[HIO_POINT_TPB],
                                                  share[2 * HIO_POINT_TPB]), i, out, status);
  }
  return 0;
}
}
