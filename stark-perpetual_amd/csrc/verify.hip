// The verifier's field arithmetic on the device: the composition value at arbitrary LDE positions from opened rows
// (sp_air_eval_points_dev) and the fold chain of every query (sp_fri_check_queries_dev) - include/starkperp.h
// "Verifying a proof".  The per-item logic and the argument rules are csrc/verify.hpp, shared with the host tests.
//
// Lane plans.  Both kernels give one item to one lane, 64 lanes per block, and read nothing that grows with the trace:
//   air_points_kernel<AIR>   lane i: pos[i], the 2 n_cols felts of its two rows, n_per periodic felts at pos mod
//                            (4 * period); the body of the dense kernel of the same AIR (verify.hpp names the twins).
//   fri_check_kernel         grid.y = the layer k, so beta_k and the 2 k squarings of shift and w are wave-uniform;
//                            lane q of grid.x: index[q], the pair of layer k, the value it folds to.
// A proof has 2 Q composition points and Q n_layers fold items (Q = 8 .. 64): a launch is a handful of waves and lasts
// as long as its longest lane - one fe_inv and log_m squarings for a fold item.
#include <string>

#include "context.hpp"
#include "verify.hpp"

namespace sp {

template <int AIR>
__global__ void __launch_bounds__(VERIFY_TPB)
air_points_kernel(unsigned log_n, const uint64_t* __restrict__ per, PointsAirParams prm, size_t n_points,
                  const uint64_t* __restrict__ pos, const uint64_t* __restrict__ cur, const uint64_t* __restrict__ nxt,
                  uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * VERIFY_TPB + threadIdx.x;
  if (i >= n_points) return;
  points_item<AIR>(log_n, per, prm, i, pos, cur, nxt, out, status);
}

__global__ void __launch_bounds__(VERIFY_TPB)
fri_check_kernel(unsigned log_m, unsigned n_layers, FriCheckParams prm, size_t n_queries,
                 const uint64_t* __restrict__ index, const uint64_t* __restrict__ pairs,
                 const uint64_t* __restrict__ final_layer, uint8_t* __restrict__ status) {
  const size_t q = (size_t)blockIdx.x * VERIFY_TPB + threadIdx.x;
  const unsigned k = blockIdx.y;
  if (q >= n_queries) return;
  status[q * n_layers + k] = fri_check_item(log_m, n_layers, prm, q, k, index, pairs, final_layer);
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_air_eval_points_dev(int air, unsigned log_n, const uint64_t* periodic_lde, const uint64_t* alphas_host,
                           const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                           const uint64_t* nxt, uint64_t* out, uint8_t* status, void* stream) {
  static const char* who = "sp_air_eval_points_dev";
  SP_REQUIRE_READY();
  if (const char* bad = points_check_args(air, log_n, n_points)) return refuse(who, bad);
  if (n_points == 0) return SP_OK;
  if (!periodic_lde || !alphas_host || !shift_host || !pos || !cur || !nxt || !out || !status)
    return refuse(who, "a NULL pointer with points to evaluate");
  if (!vf_is_felt(shift_host)) return refuse(who, "bad shift (not below p)");
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  PointsAirParams prm;
  points_params(air, alphas_host, &prm);
  const int rc = air_zinv(who, shift_host, log_n, true, prm.zinv);
  if (rc != SP_OK) return rc;
  const dim3 grid(verify_blocks(n_points)), block(VERIFY_TPB);
  const bool prof = profile_launch_begin(st);
  switch (air) {
    case VAIR_PEDERSEN:
      hipLaunchKernelGGL(air_points_kernel<VAIR_PEDERSEN>, grid, block, 0, st, log_n, periodic_lde, prm, n_points, pos,
                         cur, nxt, out, status);
      break;
    case VAIR_EC_LADDER:
      hipLaunchKernelGGL(air_points_kernel<VAIR_EC_LADDER>, grid, block, 0, st, log_n, periodic_lde, prm, n_points, pos,
                         cur, nxt, out, status);
      break;
    case VAIR_ECDSA:
      hipLaunchKernelGGL(air_points_kernel<VAIR_ECDSA>, grid, block, 0, st, log_n, periodic_lde, prm, n_points, pos,
                         cur, nxt, out, status);
      break;
    default:
      hipLaunchKernelGGL(air_points_kernel<VAIR_RANGE_CHECK>, grid, block, 0, st, log_n, periodic_lde, prm, n_points,
                         pos, cur, nxt, out, status);
      break;
  }
  if (prof) profile_launch_end(st, n_points);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_fri_check_queries_dev(unsigned log_m, unsigned n_layers, const uint64_t* shift_host, const uint64_t* betas_host,
                             size_t n_queries, const uint64_t* index, const uint64_t* pairs,
                             const uint64_t* final_layer, uint8_t* status, void* stream) {
  static const char* who = "sp_fri_check_queries_dev";
  SP_REQUIRE_READY();
  if (const char* bad = fri_check_args(log_m, n_layers, n_queries)) return refuse(who, bad);
  if (n_queries == 0) return SP_OK;
  if (!shift_host || !betas_host || !index || !pairs || !final_layer || !status)
    return refuse(who, "a NULL pointer with queries to check");
  if (!vf_is_felt(shift_host) || u256_is_zero(vf_load(shift_host)))
    return refuse(who, "bad shift (0 or not below p: the fold divides by 2 x)");
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  FriCheckParams prm;
  fri_params(log_m, n_layers, shift_host, betas_host, &prm);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(fri_check_kernel, dim3(verify_blocks(n_queries), n_layers), dim3(VERIFY_TPB), 0, st, log_m,
                     n_layers, prm, n_queries, index, pairs, final_layer, status);
  if (prof) profile_launch_end(st, n_queries * n_layers);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

}  // extern "C"
