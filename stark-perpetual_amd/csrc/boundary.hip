// Boundary quotients that bind a proof of ANY periodic AIR to its statement, on the device: the dense column the
// prover adds to its composition (sp_boundary_dev) and its value at opened points for the verifier
// (sp_boundary_points_dev) - include/starkperp.h "Boundary constraints from a descriptor", DESIGN.md 6.5.  The
// descriptor, the per-lane logic, the parameter preparation and the argument rules are csrc/boundary.hpp, shared with
// the host tests.  hash_io.hip is the three-term, period-512 instance written out by hand; it stays as it is and the
// tests hold the two against each other.
//
// Lane plans.
//   boundary_table_kernel   n_groups * 4p / 16 threads in blocks of one wave: thread t inverts 16 consecutive entries
//                           of one group's 4p-entry denominator table behind one fe_inv and leaves 1 / den_d there.
//                           The table (n_groups * 4p felts per stream: 384 KiB for the ECDSA descriptor, 16 KiB for
//                           the range check's) is all the call allocates: it does not grow with M.
//   boundary_dense_kernel   one point per lane, 256 lanes per block: n_terms trace felts and n_groups public felts
//                           in, optionally acc, one out, n_groups table entries at j mod 4p (the table stays in L2).
//                           Arithmetic: a group's terms in runs of at most three products behind one reduction, then
//                           the groups' products with their inverse denominators in runs of at most three
//                           (boundary_combine states the bound) - by byte count a streaming kernel.
//   boundary_points_kernel  one BLOCK per point, 256 lanes, for every k >= 1.  Every lane derives x = shift w^pos
//                           itself (log_m squarings), then for each group takes the coefficients lane, lane + 256,
//                           ... of C_d by Horner in y^256, y = x g^-o_d, and scales by y^lane; a tree in LDS
//                           (4 x 256 x 36 B = 36 KiB static, eight barriers, the same for every k) adds the 256
//                           shares, and lane 0 forms the denominators from x^k, inverts their product once and stores
//                           value and status.  Whether a point has a value is the same for all lanes of its block and
//                           decided before the first barrier.
#include <map>
#include <string>

#include "boundary.hpp"
#include "context.hpp"

namespace sp {

__global__ void __launch_bounds__(BND_TABLE_TPB)
boundary_table_kernel(BoundaryTableParams prm, uint64_t* __restrict__ table) {
  const unsigned t = blockIdx.x * BND_TABLE_TPB + threadIdx.x;
  if (t >= boundary_table_threads(prm)) return;
  boundary_table_item(prm, t, table);
}

// acc and out carry no __restrict__: they may be one array
__global__ void __launch_bounds__(BND_DENSE_TPB)
boundary_dense_kernel(BoundaryTerms tm, const uint64_t* __restrict__ trace, size_t col_stride,
                      const uint64_t* __restrict__ pub, size_t M, const uint64_t* __restrict__ table,
                      const uint64_t* acc, uint64_t* out) {
  const size_t j = (size_t)blockIdx.x * BND_DENSE_TPB + threadIdx.x;
  if (j >= M) return;
  boundary_dense_item(tm, trace, col_stride, pub, M, table, acc, out, j);
}

__global__ void __launch_bounds__(BND_POINT_TPB)
boundary_points_kernel(BoundaryTerms tm, BoundaryPointParams prm, const uint64_t* __restrict__ coef,
                       const uint64_t* __restrict__ pos, const uint64_t* __restrict__ cur, uint64_t* __restrict__ out,
                       uint8_t* __restrict__ status) {
  __shared__ fe share[BND_MAX_GROUPS][BND_POINT_TPB];
  const size_t i = blockIdx.x;
  const unsigned lane = threadIdx.x;
  // the same for every lane of the block, so the whole block leaves here or none of it does: no barrier is skipped
  if (!boundary_point_ok(prm.log_n, tm.n_cols, pos, cur, i)) {
    if (lane == 0) boundary_point_store(false, FE_ZERO, i, out, status);
    return;
  }
  const fe x = boundary_point_x(prm.shift, prm.w, prm.log_n, pos[i]);
#pragma unroll 1
  for (unsigned d = 0; d < tm.n_groups; ++d)
    share[d][lane] = boundary_lane_share(prm.log_n, tm.log_period, prm.arg[d], coef, x, d, lane);
  __syncthreads();
#pragma unroll 1
  for (unsigned half = BND_POINT_TPB / 2; half > 0; half >>= 1) {
    if (lane < half) {
#pragma unroll 1
      for (unsigned d = 0; d < tm.n_groups; ++d) share[d][lane] = boundary_share_add(share[d][lane], share[d][lane + half]);
    }
    __syncthreads();
  }
  if (lane != 0) return;
  // slot 1 of every row is free now: lane 0 read it in the last step of the tree, before the barrier
  boundary_point_store(true, boundary_point_value(tm, prm, x, cur + 4 * (size_t)tm.n_cols * i, &share[0][0], BND_POINT_TPB),
                       i, out, status);
}

static std::map<hipStream_t, DeviceBuffer> g_boundary_table;  // per stream, like the work buffers of stark.hip
void release_boundary_state() {
  for (auto& kv : g_boundary_table) kv.second.release();
  g_boundary_table.clear();
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_boundary_dev(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows,
                    unsigned n_terms, const unsigned* term_cols, const unsigned* term_groups, const uint64_t* trace_lde,
                    size_t col_stride, const uint64_t* pub_lde, unsigned log_n, const uint64_t* alphas_host,
                    const uint64_t* shift_host, const uint64_t* acc, uint64_t* out, void* stream) {
  static const char* who = "sp_boundary_dev";
  SP_REQUIRE_READY();
  const BoundaryDesc desc{log_period, n_cols, n_groups, group_rows, n_terms, term_cols, term_groups};
  if (const char* bad = boundary_check_desc(desc)) return refuse(who, bad);
  if (const char* bad = boundary_dense_check_args(desc, log_n, col_stride, trace_lde, pub_lde, alphas_host, shift_host, out))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)4 << log_n;
  BoundaryTableParams prm;
  boundary_table_params(desc, log_n, shift_host, &prm);
  BoundaryTerms tm;
  boundary_terms(desc, alphas_host, &tm);
  DeviceBuffer& table = g_boundary_table[st];
  SP_HIP(table.reserve(((size_t)n_groups << prm.log_4p) * 32));
  const unsigned threads = boundary_table_threads(prm);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(boundary_table_kernel, dim3((threads + BND_TABLE_TPB - 1) / BND_TABLE_TPB), dim3(BND_TABLE_TPB), 0,
                     st, prm, (uint64_t*)table.ptr);
  hipLaunchKernelGGL(boundary_dense_kernel, dim3((unsigned)(M / BND_DENSE_TPB)), dim3(BND_DENSE_TPB), 0, st, tm,
                     trace_lde, col_stride, pub_lde, M, (const uint64_t*)table.ptr, acc, out);
  if (prof) profile_launch_end(st, M);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_boundary_points_dev(unsigned log_period, unsigned n_cols, unsigned n_groups, const unsigned* group_rows,
                           unsigned n_terms, const unsigned* term_cols, const unsigned* term_groups, unsigned log_n,
                           const uint64_t* coef, const uint64_t* alphas_host, const uint64_t* shift_host,
                           size_t n_points, const uint64_t* pos, const uint64_t* cur, uint64_t* out, uint8_t* status,
                           void* stream) {
  static const char* who = "sp_boundary_points_dev";
  SP_REQUIRE_READY();
  const BoundaryDesc desc{log_period, n_cols, n_groups, group_rows, n_terms, term_cols, term_groups};
  if (const char* bad = boundary_check_desc(desc)) return refuse(who, bad);
  if (const char* bad = boundary_points_check_args(desc, log_n, n_points)) return refuse(who, bad);
  if (n_points == 0) return SP_OK;
  if (const char* bad = boundary_points_check_pointers(coef, alphas_host, shift_host, pos, cur, out, status))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  BoundaryPointParams prm;
  boundary_point_params(desc, log_n, shift_host, &prm);
  BoundaryTerms tm;
  boundary_terms(desc, alphas_host, &tm);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(boundary_points_kernel, dim3((unsigned)n_points), dim3(BND_POINT_TPB), 0, st, tm, prm, coef, pos,
                     cur, out, status);
  if (prof) profile_launch_end(st, n_points);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

}  // extern "C"
