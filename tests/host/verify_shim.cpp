// Host build of csrc/verify.hpp (the per-item logic of sp_air_eval_points_dev and sp_fri_check_queries_dev) for
// tests/test_verify_cpu.py:
//   g++ -O2 -shared -fPIC -o verify_shim.so verify_shim.cpp
// vs_points and vs_fri are the library calls over HOST arrays: the same argument rules, the same parameter
// preparation, and the kernels' launch plans replayed - block by block, lane by lane - through the same item functions.
// Only 1 / Z_H is computed here (the library takes it from air_zinv of stark.hip, which needs HIP).
// With -DVERIFY_SHIM_MAIN it is a stand-alone program that runs exactly-sized cases itself - the form to run under
// -fsanitize=address,undefined:
//   g++ -O1 -g -fsanitize=address,undefined -DVERIFY_SHIM_MAIN -o verify_check verify_shim.cpp && ./verify_check
#include <cstdio>
#include <vector>

#include "../../stark-perpetual_amd/csrc/verify.hpp"

using namespace sp;

// what air_zinv(times_r2 = true) returns; false when x^n - 1 vanishes on the coset
static bool shim_zinv(const uint64_t* shift, unsigned log_n, fe zinv[4]) {
  fe sn = fe_to_mont(vf_fe(shift));
  if (fe_is_zero(sn)) return false;
  sn = fe_sqr_n(sn, (int)log_n);
  const fe w4 = verify_root_of_unity(2);
  fe wk = FE_ONE_M;
  for (int k = 0; k < 4; ++k) {
    if (fe_eq(fe_mul(sn, wk), FE_ONE_M)) return false;
    zinv[k] = fe_mul(fe_inv(fe_carry(fe_sub(fe_mul(sn, wk), FE_ONE_M))), FE_R2);
    wk = fe_mul(wk, w4);
  }
  return true;
}

template <int AIR>
static void run_points(unsigned log_n, const uint64_t* per, const PointsAirParams& prm, size_t n, const uint64_t* pos,
                       const uint64_t* cur, const uint64_t* nxt, uint64_t* out, uint8_t* status) {
  for (size_t block = 0; block < verify_blocks(n); ++block) {
    for (unsigned lane = 0; lane < VERIFY_TPB; ++lane) {
      const size_t i = block * VERIFY_TPB + lane;
      if (i >= n) continue;
      points_item<AIR>(log_n, per, prm, i, pos, cur, nxt, out, status);
    }
  }
}

extern "C" {

unsigned vs_blocks(size_t items) { return verify_blocks(items); }
uint64_t vs_layer_pos(unsigned log_m, unsigned k, uint64_t j) { return fri_layer_pos(log_m, k, j); }
unsigned vs_next_side(unsigned log_m, unsigned k, uint64_t jk) { return fri_next_side(log_m, k, jk); }
int vs_is_felt(const uint64_t* v) { return vf_is_felt(v) ? 1 : 0; }

static int refuse(const char* bad, char* err, size_t err_len) {
  if (err && err_len) snprintf(err, err_len, "%s", bad);
  return -3;  // SP_ERR_BAD_ARGUMENT
}

int vs_points(int air, unsigned log_n, const uint64_t* per, const uint64_t* alphas, const uint64_t* shift, size_t n,
              const uint64_t* pos, const uint64_t* cur, const uint64_t* nxt, uint64_t* out, uint8_t* status, char* err,
              size_t err_len) {
  if (const char* bad = points_check_args(air, log_n, n)) return refuse(bad, err, err_len);
  if (n == 0) return 0;
  if (!per || !alphas || !shift || !pos || !cur || !nxt || !out || !status) return refuse("NULL", err, err_len);
  if (!vf_is_felt(shift)) return refuse("bad shift", err, err_len);
  PointsAirParams prm;
  points_params(air, alphas, &prm);
  if (!shim_zinv(shift, log_n, prm.zinv)) return refuse("bad shift", err, err_len);
  switch (air) {
    case VAIR_PEDERSEN: run_points<VAIR_PEDERSEN>(log_n, per, prm, n, pos, cur, nxt, out, status); break;
    case VAIR_EC_LADDER: run_points<VAIR_EC_LADDER>(log_n, per, prm, n, pos, cur, nxt, out, status); break;
    case VAIR_ECDSA: run_points<VAIR_ECDSA>(log_n, per, prm, n, pos, cur, nxt, out, status); break;
    default: run_points<VAIR_RANGE_CHECK>(log_n, per, prm, n, pos, cur, nxt, out, status); break;
  }
  return 0;
}

int vs_fri(unsigned log_m, unsigned n_layers, const uint64_t* shift, const uint64_t* betas, size_t n_queries,
           const uint64_t* index, const uint64_t* pairs, const uint64_t* final_layer, uint8_t* status, char* err,
           size_t err_len) {
  if (const char* bad = fri_check_args(log_m, n_layers, n_queries)) return refuse(bad, err, err_len);
  if (n_queries == 0) return 0;
  if (!shift || !betas || !index || !pairs || !final_layer || !status) return refuse("NULL", err, err_len);
  if (!vf_is_felt(shift) || u256_is_zero(vf_load(shift))) return refuse("bad shift", err, err_len);
  FriCheckParams prm;
  fri_params(log_m, n_layers, shift, betas, &prm);
  for (unsigned k = 0; k < n_layers; ++k) {  // grid.y
    for (size_t block = 0; block < verify_blocks(n_queries); ++block) {
      for (unsigned lane = 0; lane < VERIFY_TPB; ++lane) {
        const size_t q = block * VERIFY_TPB + lane;
        if (q >= n_queries) continue;
        status[q * n_layers + k] = fri_check_item(log_m, n_layers, prm, q, k, index, pairs, final_layer);
      }
    }
  }
  return 0;
}
}

#ifdef VERIFY_SHIM_MAIN
// Exactly-sized arrays, so that an index one past an array is an AddressSanitizer report.  The fold cases are
// self-made chains: layer k + 1 is whatever the item of layer k says it folds to, found by trying the status - the
// expectations in integers are the Python tests'; this program checks bounds, statuses and determinism.
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static void rand_felt(uint64_t* f) {
  f[0] = rnd(), f[1] = rnd(), f[2] = rnd(), f[3] = rnd() & 0x07ffffffffffffffull;  // below 2^251 < p
}
static bool points_case(int air, unsigned log_n, size_t n) {
  const VerifyAirShape sh = verify_air_shape(air);
  const uint64_t M = (uint64_t)4 << log_n;
  std::vector<uint64_t> per(4 * (size_t)sh.n_per * sh.per_len), alphas(4 * sh.n_alpha), shift = {3, 0, 0, 0};
  std::vector<uint64_t> pos(n), cur(4 * n * sh.n_cols), nxt(4 * n * sh.n_cols), out(4 * n, ~0ull);
  std::vector<uint8_t> status(n, 0xee);
  for (size_t i = 0; i < per.size(); i += 4) rand_felt(&per[i]);
  for (size_t i = 0; i < alphas.size(); i += 4) rand_felt(&alphas[i]);
  for (size_t i = 0; i < cur.size(); i += 4) rand_felt(&cur[i]), rand_felt(&nxt[i]);
  for (size_t i = 0; i < n; ++i) pos[i] = i % 3 == 0 ? M - 1 - (i % M) : rnd() % M;
  if (n > 2) {
    pos[1] = M;              // out of range: the periodic table must still be read inside
    pos[2] = ~(uint64_t)0;
    if (n > 3) cur[4 * 3 * sh.n_cols + 3] = ~(uint64_t)0;  // a felt >= p
  }
  char err[64] = "";
  if (vs_points(air, log_n, per.data(), alphas.data(), shift.data(), n, pos.data(), cur.data(), nxt.data(), out.data(),
                status.data(), err, sizeof err) != 0)
    return false;
  for (size_t i = 0; i < n; ++i) {
    const bool bad = n > 2 && (i == 1 || i == 2 || (i == 3 && n > 3));
    if (status[i] != (bad ? VERIFY_OUT_OF_RANGE : VERIFY_OK)) return false;
    if (!vf_is_felt(&out[4 * i])) return false;
    if (bad && (out[4 * i] | out[4 * i + 1] | out[4 * i + 2] | out[4 * i + 3]) != 0) return false;
  }
  return true;
}
static bool fri_case(unsigned log_m, unsigned n_layers, size_t nq) {
  std::vector<uint64_t> shift = {3, 0, 0, 0}, betas(4 * n_layers), index(nq), pairs(8 * nq * n_layers);
  std::vector<uint64_t> fin(4 * ((size_t)1 << (log_m - n_layers)));
  std::vector<uint8_t> status(nq * n_layers, 0xee);
  for (size_t i = 0; i < betas.size(); i += 4) rand_felt(&betas[i]);
  for (size_t i = 0; i < pairs.size(); i += 4) rand_felt(&pairs[i]);
  for (size_t i = 0; i < fin.size(); i += 4) rand_felt(&fin[i]);
  const uint64_t half = (uint64_t)1 << (log_m - 1);
  for (size_t q = 0; q < nq; ++q) index[q] = q == 0 ? 0 : q == 1 ? half - 1 : rnd() % half;
  if (nq > 2) index[2] = half;                                  // out of range: every layer flagged
  if (nq > 3) pairs[8 * (3 * n_layers) + 3] = ~(uint64_t)0;     // a of (3, 0) >= p
  char err[64] = "";
  if (vs_fri(log_m, n_layers, shift.data(), betas.data(), nq, index.data(), pairs.data(), fin.data(), status.data(),
             err, sizeof err) != 0)
    return false;
  for (size_t q = 0; q < nq; ++q) {
    for (unsigned k = 0; k < n_layers; ++k) {
      const uint8_t s = status[q * n_layers + k];
      if (q == 2 && nq > 2) { if (s != FRI_OUT_OF_RANGE) return false; }
      else if (q == 3 && k == 0) { if (s != FRI_OUT_OF_RANGE) return false; }
      else if (s != FRI_MISMATCH) return false;  // random targets never match
    }
  }
  return true;
}
int main() {
  bool ok = true;
  const unsigned min_log[4] = {9, 8, 10, 7};
  for (int air = 0; air < 4; ++air) {
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65}) ok = ok && points_case(air, min_log[air], n);
  }
  ok = ok && fri_case(7, 1, 5) && fri_case(9, 3, 65) && fri_case(12, 6, 7) && fri_case(32, 31, 4) && fri_case(2, 1, 4);
  // refused calls write nothing
  char err[64] = "";
  uint8_t st = 0xee;
  ok = ok && vs_points(4, 9, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, &st, err, sizeof err) == -3;
  ok = ok && vs_points(0, 8, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, &st, err, sizeof err) == -3;
  ok = ok && vs_points(0, 9, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &st, err, sizeof err) == 0;
  ok = ok && vs_fri(7, 7, nullptr, nullptr, 1, nullptr, nullptr, nullptr, &st, err, sizeof err) == -3;
  ok = ok && vs_fri(33, 1, nullptr, nullptr, 1, nullptr, nullptr, nullptr, &st, err, sizeof err) == -3;
  ok = ok && vs_fri(7, 0, nullptr, nullptr, 1, nullptr, nullptr, nullptr, &st, err, sizeof err) == -3;
  ok = ok && vs_fri(7, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &st, err, sizeof err) == 0 && st == 0xee;
  std::printf(ok ? "verify check passed\n" : "verify check FAILED\n");
  return ok ? 0 : 1;
}
#endif
