// Boundary quotients that bind a proof of the COMBINED builtin trace to its statement - hashes, signatures and
// range-checked values - on the device: the public columns combined before extension (sp_boundary_combine_dev), the
// dense column the prover adds to its composition (sp_builtins_boundary_dev) and its value at opened points for the
// verifier (sp_builtins_boundary_points_dev) - include/starkperp.h "Boundary constraints of the builtins proof",
// DESIGN.md 6.6.  The segment table, the per-lane logic, the parameter preparation and the argument rules are
// csrc/builtins_boundary.hpp, shared with the host tests; the arithmetic is boundary.hpp's.
//
// Lane plans.
//   bb_combine_kernel   one item per lane, 256 lanes per block: the terms' felts at index i in, one felt per group
//                       out; a group's terms in runs of at most three products behind one reduction.
//   bb_table_kernel     ONE launch for every group of every present segment: sum_s n_groups_s * 4 p_s / 16 threads
//                       (at most 1154) in blocks of one wave, thread t inverts 16 consecutive entries of one group's
//                       denominator table behind one fe_inv.  The table (3 * 2048 + 3 * 4096 + 32 felts = 577 KiB per
//                       stream at most) is all the call allocates: it does not grow with M.
//   bb_dense_kernel     ONE launch, one point per lane, 256 lanes per block: per present segment the terms' trace
//                       felts, the groups' public felts and table entries at j mod 4 p_s, optionally acc, one out.
//                       The descriptors are kernel arguments read through wave-uniform loop counters.
//   bb_points_kernel    one BLOCK per point, 256 lanes.  Whether the point has a value - pos below M, every felt of
//                       the WHOLE opened row below p - is the same for all lanes and decided before the first barrier.
//                       The segments run one after the other through the same 4 x 256 x 36 B = 36 KiB of LDS: shares,
//                       the tree of eight barriers, lane 0's inversion and partial value, one more barrier.
#include <map>

#include "builtins_boundary.hpp"
#include "context.hpp"

namespace sp {

__global__ void __launch_bounds__(BB_COMBINE_TPB)
bb_combine_kernel(BbCombineParams cp, size_t k, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BB_COMBINE_TPB + threadIdx.x;
  if (i >= k) return;
  bb_combine_item(cp, k, out, i);
}

__global__ void __launch_bounds__(BND_TABLE_TPB)
bb_table_kernel(BbTableParams tp, uint64_t* __restrict__ table) {
  const unsigned t = blockIdx.x * BND_TABLE_TPB + threadIdx.x;
  if (t >= tp.n_threads) return;
  bb_table_item(tp, t, table);
}

// acc and out carry no __restrict__: they may be one array
__global__ void __launch_bounds__(BND_DENSE_TPB)
bb_dense_kernel(BbDenseParams dp, const uint64_t* __restrict__ trace, size_t col_stride,
                const uint64_t* __restrict__ pub, size_t M, const uint64_t* __restrict__ table, const uint64_t* acc,
                uint64_t* out) {
  const size_t j = (size_t)blockIdx.x * BND_DENSE_TPB + threadIdx.x;
  if (j >= M) return;
  bb_dense_item(dp, trace, col_stride, pub, M, table, acc, out, j);
}

__global__ void __launch_bounds__(BND_POINT_TPB)
bb_points_kernel(BbPointParams pp, const uint64_t* __restrict__ coef, const uint64_t* __restrict__ pos,
                 const uint64_t* __restrict__ cur, uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  __shared__ fe share[BND_MAX_GROUPS][BND_POINT_TPB];
  const size_t i = blockIdx.x;
  const unsigned lane = threadIdx.x;
  // the same for every lane of the block, so the whole block leaves here or none of it does: no barrier is skipped
  if (!boundary_point_ok(pp.log_n, pp.n_cols, pos, cur, i)) {
    if (lane == 0) boundary_point_store(false, FE_ZERO, i, out, status);
    return;
  }
  const fe x = boundary_point_x(pp.seg[0].prm.shift, pp.seg[0].prm.w, pp.log_n, pos[i]);
  fe total = FE_ZERO;  // lane 0's running sum
#pragma unroll 1
  for (unsigned s = 0; s < pp.n_segs; ++s) {
    const BbPointSeg& sg = pp.seg[s];
#pragma unroll 1
    for (unsigned d = 0; d < sg.tm.n_groups; ++d)
      share[d][lane] = boundary_lane_share(pp.log_n, sg.tm.log_period, sg.prm.arg[d], coef + 4 * sg.coef0, x, d, lane);
    __syncthreads();
#pragma unroll 1
    for (unsigned half = BND_POINT_TPB / 2; half > 0; half >>= 1) {
      if (lane < half) {
#pragma unroll 1
        for (unsigned d = 0; d < sg.tm.n_groups; ++d) share[d][lane] = boundary_share_add(share[d][lane], share[d][lane + half]);
      }
      __syncthreads();
    }
    // slot 1 of every row is free now: lane 0 read it in the last step of the tree, before the barrier
    if (lane == 0)
      total = fe_add(total, bb_point_segment_value(sg, x, cur + 4 * (size_t)pp.n_cols * i, &share[0][0], BND_POINT_TPB));
    __syncthreads();  // the next segment's shares overwrite what lane 0 has just used
  }
  if (lane == 0) boundary_point_store(true, fe_canon(total), i, out, status);
}

static std::map<hipStream_t, DeviceBuffer> g_bb_table;  // per stream, like the table of boundary.hip
void release_builtins_boundary_state() {
  for (auto& kv : g_bb_table) kv.second.release();
  g_bb_table.clear();
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_boundary_combine_dev(unsigned n_groups, unsigned n_terms, const unsigned* term_groups,
                            const uint64_t* const* values_host, size_t k, const uint64_t* alphas_host, uint64_t* out,
                            void* stream) {
  static const char* who = "sp_boundary_combine_dev";
  SP_REQUIRE_READY();
  if (const char* bad = bb_combine_check_args(n_groups, n_terms, term_groups, values_host, k, alphas_host, out))
    return refuse(who, bad);
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  BbCombineParams cp;
  bb_combine_params(n_groups, n_terms, term_groups, values_host, alphas_host, &cp);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(bb_combine_kernel, dim3((unsigned)((k + BB_COMBINE_TPB - 1) / BB_COMBINE_TPB)), dim3(BB_COMBINE_TPB),
                     0, st, cp, k, out);
  if (prof) profile_launch_end(st, k);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_builtins_boundary_dev(unsigned segments, unsigned log_n, const uint64_t* trace_lde, size_t col_stride,
                             const uint64_t* pub_lde, const uint64_t* alphas_host, const uint64_t* shift_host,
                             const uint64_t* acc, uint64_t* out, void* stream) {
  static const char* who = "sp_builtins_boundary_dev";
  SP_REQUIRE_READY();
  if (const char* bad = bb_dense_check_args(segments, log_n, col_stride, trace_lde, pub_lde, alphas_host, shift_host, out))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)4 << log_n;
  BbTableParams tp;
  BbDenseParams dp;
  bb_dense_params(segments, log_n, alphas_host, shift_host, &tp, &dp);
  DeviceBuffer& table = g_bb_table[st];
  SP_HIP(table.reserve((size_t)tp.n_felts * 32));
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(bb_table_kernel, dim3((tp.n_threads + BND_TABLE_TPB - 1) / BND_TABLE_TPB), dim3(BND_TABLE_TPB), 0, st,
                     tp, (uint64_t*)table.ptr);
  hipLaunchKernelGGL(bb_dense_kernel, dim3((unsigned)((M + BND_DENSE_TPB - 1) / BND_DENSE_TPB)), dim3(BND_DENSE_TPB), 0, st,
                     dp, trace_lde, col_stride, pub_lde, M, (const uint64_t*)table.ptr, acc, out);
  if (prof) profile_launch_end(st, M);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_builtins_boundary_points_dev(unsigned segments, unsigned log_n, const uint64_t* coef, const uint64_t* alphas_host,
                                    const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                                    uint64_t* out, uint8_t* status, void* stream) {
  static const char* who = "sp_builtins_boundary_points_dev";
  SP_REQUIRE_READY();
  if (const char* bad = bb_points_check_args(segments, log_n, n_points)) return refuse(who, bad);
  if (n_points == 0) return SP_OK;
  if (const char* bad = boundary_points_check_pointers(coef, alphas_host, shift_host, pos, cur, out, status))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  BbPointParams pp;
  bb_point_params(segments, log_n, alphas_host, shift_host, &pp);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(bb_points_kernel, dim3((unsigned)n_points), dim3(BND_POINT_TPB), 0, st, pp, coef, pos, cur, out,
                     status);
  if (prof) profile_launch_end(st, n_points);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

}  // extern "C"
