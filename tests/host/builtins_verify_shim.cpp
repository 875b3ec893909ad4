// Host build of csrc/verify_builtins.hpp (the per-point logic of sp_builtins_eval_points_dev) for
// tests/test_builtins_verify_cpu.py:
//   g++ -O2 -shared -fPIC -o builtins_verify_shim.so builtins_verify_shim.cpp
// bvs_points is the library call over HOST arrays: the same argument rules, the same parameter preparation, and the
// kernel's launch plan replayed - block by block, one wave per present segment, lane by lane, the parts parked in a
// block-sized array, then wave 0's sum - through the same functions.  Only 1 / Z_H is computed here, in both of its
// forms (the library takes them from air_zinv of stark.hip, which needs HIP).
// With -DBUILTINS_SHIM_MAIN it is a stand-alone program that runs exactly-sized cases itself - the form to run under
// -fsanitize=address,undefined:
//   g++ -O1 -g -fsanitize=address,undefined -DBUILTINS_SHIM_MAIN -o builtins_check builtins_verify_shim.cpp
#include <cstdio>
#include <vector>

#include "../../stark-perpetual_amd/csrc/verify_builtins.hpp"

using namespace sp;

// what air_zinv returns with times_r2 = true (zinv_r2) and false (zinv); false when x^n - 1 vanishes on the coset
static bool shim_zinv(const uint64_t* shift, unsigned log_n, fe zinv_r2[4], fe zinv[4]) {
  fe sn = fe_to_mont(vf_fe(shift));
  if (fe_is_zero(sn)) return false;
  sn = fe_sqr_n(sn, (int)log_n);
  const fe w4 = verify_root_of_unity(2);
  fe wk = FE_ONE_M;
  for (int k = 0; k < 4; ++k) {
    if (fe_eq(fe_mul(sn, wk), FE_ONE_M)) return false;
    zinv[k] = fe_inv(fe_carry(fe_sub(fe_mul(sn, wk), FE_ONE_M)));
    zinv_r2[k] = fe_mul(zinv[k], FE_R2);
    wk = fe_mul(wk, w4);
  }
  return true;
}

extern "C" {

static int refuse(const char* bad, char* err, size_t err_len) {
  if (err && err_len) snprintf(err, err_len, "%s", bad);
  return -3;  // SP_ERR_BAD_ARGUMENT
}

unsigned bvs_n_cols(unsigned segments) { return builtins_shape(segments).n_cols; }
unsigned bvs_n_alpha(unsigned segments) { return builtins_shape(segments).n_alpha; }
unsigned bvs_block_threads(unsigned segments) { return builtins_shape(segments).n_segs * VERIFY_TPB; }

int bvs_points(unsigned segments, unsigned log_n, const uint64_t* per_pedersen, const uint64_t* per_ecdsa,
               const uint64_t* per_rc16, const uint64_t* alphas, const uint64_t* shift, const uint64_t* z,
               uint64_t rc_min, uint64_t rc_max, size_t n, const uint64_t* pos, const uint64_t* cur,
               const uint64_t* nxt, const uint64_t* pcur, const uint64_t* pnxt, uint64_t* out, uint8_t* status,
               char* err, size_t err_len) {
  if (const char* bad = builtins_check_args(segments, log_n, rc_min, rc_max, n)) return refuse(bad, err, err_len);
  if (n == 0) return 0;
  if (const char* bad = builtins_check_pointers(segments, per_pedersen, per_ecdsa, per_rc16, alphas, shift, z, pos, cur,
                                                nxt, pcur, pnxt, out, status))
    return refuse(bad, err, err_len);
  fe zinv_r2[4], zinv[4];
  if (!shim_zinv(shift, log_n, zinv_r2, zinv)) return refuse("bad shift", err, err_len);
  PointsAirParams ped = {}, ecd = {};
  Rc16PointParams rcp = {};
  BuiltinsShape sh;
  for (unsigned k = 0; k < BSEG_MAX; ++k) {
    const BuiltinsWave w = builtins_wave(segments, k, &sh);
    const uint64_t* al = alphas + 4 * w.alpha0;
    if (w.seg == BSEG_PEDERSEN) points_params(VAIR_PEDERSEN, al, &ped);
    if (w.seg == BSEG_ECDSA) points_params(VAIR_ECDSA, al, &ecd);
    if (w.seg == BSEG_RC16) rc16_point_params(log_n, al, shift, z, rc_min, rc_max, &rcp);
  }
  for (int k = 0; k < 4; ++k) {
    ped.zinv[k] = ecd.zinv[k] = zinv_r2[k];
    rcp.zinv[k] = zinv[k];
  }
  const BuiltinsPointsArgs g = {segments, log_n, per_pedersen, per_ecdsa, per_rc16, n, pos, cur, nxt, pcur, pnxt, out,
                                status};
  for (size_t block = 0; block < verify_blocks(n); ++block) {
    fe parts[BSEG_MAX][VERIFY_TPB];  // the block's LDS
    bool flags[BSEG_MAX][VERIFY_TPB];
    for (unsigned wave = 0; wave < sh.n_segs; ++wave) {
      const BuiltinsWave w = builtins_wave(segments, wave);
      for (unsigned lane = 0; lane < VERIFY_TPB; ++lane) {
        const size_t i = block * VERIFY_TPB + lane;
        if (i >= n) continue;
        parts[wave][lane] = builtins_segment_value(g, w, sh.n_cols, ped, ecd, rcp, i, &flags[wave][lane]);
      }
    }
    for (unsigned lane = 0; lane < VERIFY_TPB; ++lane) {  // wave 0 after the barrier
      const size_t i = block * VERIFY_TPB + lane;
      if (i >= n) continue;
      fe sum = parts[0][lane];
      bool ok = flags[0][lane];
      for (unsigned k = 1; k < sh.n_segs; ++k) {
        sum = fe_add(sum, parts[k][lane]);
        ok = ok & flags[k][lane];
      }
      builtins_store(sum, ok, i, out, status);
    }
  }
  return 0;
}
}

#ifdef BUILTINS_SHIM_MAIN
// Exactly-sized arrays, so that an index one past an array is an AddressSanitizer report.  The expectations in
// integers are the Python tests'; this program checks bounds, statuses and that refused calls write nothing.
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}
static void rand_felt(uint64_t* f) {
  f[0] = rnd(), f[1] = rnd(), f[2] = rnd(), f[3] = rnd() & 0x07ffffffffffffffull;  // below 2^251 < p
}
static void rand_felts(std::vector<uint64_t>& v) {
  for (size_t i = 0; i < v.size(); i += 4) rand_felt(&v[i]);
}
static bool points_case(unsigned segments, size_t n) {
  const BuiltinsShape sh = builtins_shape(segments);
  const unsigned log_n = sh.min_log_n;
  const uint64_t M = (uint64_t)4 << log_n;
  const bool ped = segments & BSEG_PEDERSEN, ecd = segments & BSEG_ECDSA, rc = segments & BSEG_RC16;
  std::vector<uint64_t> per_p(ped ? 4 * 6 * 2048 : 0), per_e(ecd ? 4 * 12 * 4096 : 0), per_r(rc ? 4 * 2 * 32 : 0);
  std::vector<uint64_t> alphas(4 * sh.n_alpha), shift = {3, 0, 0, 0}, z(rc ? 4 : 0);
  std::vector<uint64_t> pos(n), cur(4 * n * sh.n_cols), nxt(4 * n * sh.n_cols), pcur(rc ? 4 * n : 0), pnxt(rc ? 4 * n : 0);
  std::vector<uint64_t> out(4 * n, ~0ull);
  std::vector<uint8_t> status(n, 0xee);
  for (auto* v : {&per_p, &per_e, &per_r, &alphas, &z, &cur, &nxt, &pcur, &pnxt}) rand_felts(*v);
  for (size_t i = 0; i < n; ++i) pos[i] = i % 3 == 0 ? M - 1 - (i % M) : rnd() % M;
  if (n > 2) {
    pos[1] = M;  // out of range: the periodic tables must still be read inside
    pos[2] = ~(uint64_t)0;
    if (n > 3) nxt[4 * (3 * sh.n_cols + sh.n_cols - 1) + 3] = ~(uint64_t)0;  // a felt >= p in the last column
    if (n > 4 && rc) pnxt[4 * 4 + 3] = ~(uint64_t)0;
  }
  char err[96] = "";
  if (bvs_points(segments, log_n, ped ? per_p.data() : nullptr, ecd ? per_e.data() : nullptr, rc ? per_r.data() : nullptr,
                 alphas.data(), shift.data(), rc ? z.data() : nullptr, 3, 40000, n, pos.data(), cur.data(), nxt.data(),
                 rc ? pcur.data() : nullptr, rc ? pnxt.data() : nullptr, out.data(), status.data(), err, sizeof err) != 0)
    return false;
  for (size_t i = 0; i < n; ++i) {
    const bool bad = n > 2 && (i == 1 || i == 2 || (i == 3 && n > 3) || (i == 4 && n > 4 && rc));
    if (status[i] != (bad ? VERIFY_OUT_OF_RANGE : VERIFY_OK)) return false;
    if (!vf_is_felt(&out[4 * i])) return false;
    if (bad && (out[4 * i] | out[4 * i + 1] | out[4 * i + 2] | out[4 * i + 3]) != 0) return false;
  }
  return true;
}
int main() {
  bool ok = true;
  for (unsigned segments = 1; segments <= BSEG_ALL; ++segments) {
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65}) ok = ok && points_case(segments, n);
  }
  // refused calls write nothing and read no pointer
  char err[96] = "";
  uint8_t st = 0xee;
  auto bare = [&](unsigned segments, unsigned log_n, uint64_t lo, uint64_t hi, size_t n) {
    return bvs_points(segments, log_n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lo, hi, n, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, &st, err, sizeof err);
  };
  ok = ok && bare(0, 10, 0, 1, 1) == -3 && bare(8, 10, 0, 1, 1) == -3;
  ok = ok && bare(1, 8, 0, 1, 1) == -3 && bare(2, 9, 0, 1, 1) == -3 && bare(4, 2, 0, 1, 1) == -3;
  ok = ok && bare(4, 25, 0, 1, 1) == -3 && bare(3, 31, 0, 1, 1) == -3;
  ok = ok && bare(4, 3, 2, 1, 1) == -3 && bare(4, 3, 0, 65536, 1) == -3;
  ok = ok && bare(7, 10, 0, 1, ((size_t)1 << 30) + 1) == -3;
  ok = ok && bare(7, 10, 0, 1, 1) == -3;  // NULL
  ok = ok && bare(7, 10, 0, 1, 0) == 0 && st == 0xee;
  std::printf(ok ? "builtins verify check passed\n" : "builtins verify check FAILED\n");
  return ok ? 0 : 1;
}
#endif
