// The composition value of a prove_builtins proof at opened points on the device (sp_builtins_eval_points_dev,
// include/starkperp.h "Verifying a proof").  The per-point logic and the argument rules are csrc/verify_builtins.hpp,
// shared with the host tests.
//
// Lane plan.  A block serves 64 points with ONE WAVE PER PRESENT SEGMENT (64, 128 or 192 threads): lane l of every
// wave holds point 64 * blockIdx.x + l, and a wave-uniform branch on the wave index - formed through readfirstlane,
// so it is a scalar branch - sends wave k into the body of the k-th present segment: points_body_pedersen,
// points_body_ecdsa (verify.hpp, unchanged) or points_body_rc16 (verify_builtins.hpp).  Each wave parks its canonical
// part and its range flag in LDS (64 x 36 B + 64 B per wave); after one barrier wave 0 adds the parts mod p and
// stores value and status.  No wave carries more than one body, so the launch lasts as long as its longest segment -
// the rc16 wave's one fe_inv and log_m squarings, or the ECDSA body - not their sum.  Nothing that grows with the
// trace is read: the periodic tables have 2048, 4096 and 32 rows.
#include <string>

#include "context.hpp"
#include "verify_builtins.hpp"

namespace sp {

__global__ void __launch_bounds__(BSEG_MAX * VERIFY_TPB)
builtins_points_kernel(BuiltinsPointsArgs g, PointsAirParams ped, PointsAirParams ecd, Rc16PointParams rc) {
  __shared__ fe parts[BSEG_MAX][VERIFY_TPB];
  __shared__ uint8_t flags[BSEG_MAX][VERIFY_TPB];
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x / VERIFY_TPB);
  const unsigned lane = threadIdx.x % VERIFY_TPB;
  const size_t i = (size_t)blockIdx.x * VERIFY_TPB + lane;
  const bool live = i < g.n_points;
  BuiltinsShape sh;
  const BuiltinsWave w = builtins_wave(g.segments, wave, &sh);
  if (live) {
    bool ok;
    parts[wave][lane] = builtins_segment_value(g, w, sh.n_cols, ped, ecd, rc, i, &ok);
    flags[wave][lane] = ok ? 1 : 0;
  }
  __syncthreads();
  if (wave != 0 || !live) return;
  fe sum = parts[0][lane];
  bool ok = flags[0][lane] != 0;
  for (unsigned k = 1; k < sh.n_segs; ++k) {
    sum = fe_add(sum, parts[k][lane]);
    ok = ok & (flags[k][lane] != 0);
  }
  builtins_store(sum, ok, i, g.out, g.status);
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_builtins_eval_points_dev(unsigned segments, unsigned log_n, const uint64_t* per_pedersen,
                                const uint64_t* per_ecdsa, const uint64_t* per_rc16, const uint64_t* alphas_host,
                                const uint64_t* shift_host, const uint64_t* z_host, uint64_t rc_min, uint64_t rc_max,
                                size_t n_points, const uint64_t* pos, const uint64_t* cur, const uint64_t* nxt,
                                const uint64_t* pcur, const uint64_t* pnxt, uint64_t* out, uint8_t* status,
                                void* stream) {
  static const char* who = "sp_builtins_eval_points_dev";
  SP_REQUIRE_READY();
  if (const char* bad = builtins_check_args(segments, log_n, rc_min, rc_max, n_points)) return refuse(who, bad);
  if (n_points == 0) return SP_OK;
  if (const char* bad = builtins_check_pointers(segments, per_pedersen, per_ecdsa, per_rc16, alphas_host, shift_host,
                                                z_host, pos, cur, nxt, pcur, pnxt, out, status))
    return refuse(who, bad);
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  // both forms of 1 / Z_H: the Pedersen and ECDSA bodies want it times R^2, the rc16 body keeps its factors itself
  fe zinv_r2[4], zinv[4];
  int rc = air_zinv(who, shift_host, log_n, true, zinv_r2);
  if (rc == SP_OK) rc = air_zinv(who, shift_host, log_n, false, zinv);
  if (rc != SP_OK) return rc;
  PointsAirParams ped = {}, ecd = {};
  Rc16PointParams rcp = {};
  BuiltinsShape sh;
  for (unsigned k = 0; k < BSEG_MAX; ++k) {
    const BuiltinsWave w = builtins_wave(segments, k, &sh);
    const uint64_t* al = alphas_host + 4 * w.alpha0;
    if (w.seg == BSEG_PEDERSEN) points_params(VAIR_PEDERSEN, al, &ped);
    if (w.seg == BSEG_ECDSA) points_params(VAIR_ECDSA, al, &ecd);
    if (w.seg == BSEG_RC16) rc16_point_params(log_n, al, shift_host, z_host, rc_min, rc_max, &rcp);
  }
  for (int k = 0; k < 4; ++k) {
    ped.zinv[k] = ecd.zinv[k] = zinv_r2[k];
    rcp.zinv[k] = zinv[k];
  }
  const BuiltinsPointsArgs g = {segments, log_n, per_pedersen, per_ecdsa, per_rc16, n_points, pos, cur, nxt, pcur, pnxt,
                                out, status};
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(builtins_points_kernel, dim3(verify_blocks(n_points)), dim3(sh.n_segs * VERIFY_TPB), 0, st, g, ped,
                     ecd, rcp);
  if (prof) profile_launch_end(st, n_points);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

}  // extern "C"
