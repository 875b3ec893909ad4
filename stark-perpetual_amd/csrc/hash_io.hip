// The boundary quotients that bind the inputs and the output of every hash of a Pedersen proof, on the device:
// the dense column the prover adds to its composition (sp_hash_io_boundary_dev) and its value at opened points for the
// verifier (sp_hash_io_boundary_points_dev) - include/starkperp.h "Binding a Pedersen proof to its hashes", DESIGN.md
// 6.4.  The per-lane logic, the parameter preparation and the argument rules are csrc/hash_io.hpp, shared with the
// host tests.
//
// Lane plans.
//   hash_io_table_kernel    384 threads, 6 blocks of one wave: thread t inverts 16 consecutive entries of one of the
//                           three 2048-entry denominator tables behind one fe_inv and leaves alpha_c / den_c there.
//                           The table (192 KiB, per stream) is all the call allocates: it does not grow with M.
//   hash_io_dense_kernel    one point per lane, 256 lanes per block: 5 felts in (s, px, X, Y, H), optionally acc, one
//                           out, three table entries at j mod 2048 (the table stays in L2) and ONE field reduction -
//                           by byte count a streaming kernel.
//   hash_io_points_kernel   one BLOCK per point, 256 lanes.  Every lane derives x = shift w^pos itself (log_m
//                           squarings), then for each of X, Y, H takes the coefficients lane, lane + 256, ... by
//                           Horner in y^256 and scales by y^lane; a tree in LDS (3 x 256 x 36 B, eight barriers, the
//                           same for every k) adds the 256 shares, and lane 0 forms the three denominators from x^k,
//                           inverts their product once and stores value and status.  A proof has 2 Q points; the
//                           launch lasts as long as k / 256 Horner steps, 3 x 16 powers and one fe_inv.
#include <map>
#include <string>

#include "context.hpp"
#include "hash_io.hpp"

namespace sp {

__global__ void __launch_bounds__(HIO_TABLE_TPB)
hash_io_table_kernel(HashIoTableParams prm, uint64_t* __restrict__ table) {
  const unsigned t = blockIdx.x * HIO_TABLE_TPB + threadIdx.x;
  if (t >= HIO_TABLE_THREADS) return;
  hash_io_table_item(prm, t, table);
}

// acc and out carry no __restrict__: they may be one array
__global__ void __launch_bounds__(HIO_DENSE_TPB)
hash_io_dense_kernel(const uint64_t* __restrict__ trace, size_t col_stride, const uint64_t* __restrict__ pub, size_t M,
                     const uint64_t* __restrict__ table, const uint64_t* acc, uint64_t* out) {
  const size_t j = (size_t)blockIdx.x * HIO_DENSE_TPB + threadIdx.x;
  if (j >= M) return;
  hash_io_dense_item(trace, col_stride, pub, M, table, acc, out, j);
}

__global__ void __launch_bounds__(HIO_POINT_TPB)
hash_io_points_kernel(HashIoPointParams prm, const uint64_t* __restrict__ coef, const uint64_t* __restrict__ pos,
                      const uint64_t* __restrict__ cur, uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  __shared__ fe share[3][HIO_POINT_TPB];
  const size_t i = blockIdx.x;
  const unsigned lane = threadIdx.x;
  // the same for every lane of the block, so the whole block leaves here or none of it does: no barrier is skipped
  if (!hash_io_point_ok(prm.log_n, pos, cur, i)) {
    if (lane == 0) boundary_point_store(false, FE_ZERO, i, out, status);
    return;
  }
  const fe x = boundary_point_x(prm.shift, prm.w, prm.log_n, pos[i]);
#pragma unroll 1
  for (unsigned c = 0; c < 3; ++c) share[c][lane] = boundary_lane_share(prm.log_n, 9, prm.arg[c], coef, x, c, lane);
  __syncthreads();
#pragma unroll 1
  for (unsigned half = HIO_POINT_TPB / 2; half > 0; half >>= 1) {
    if (lane < half) {
#pragma unroll 1
      for (unsigned c = 0; c < 3; ++c) share[c][lane] = boundary_share_add(share[c][lane], share[c][lane + half]);
    }
    __syncthreads();
  }
  if (lane != 0) return;
  boundary_point_store(true, hash_io_point_value(prm, x, cur + 16 * i, share[0][0], share[1][0], share[2][0]), i, out,
                      status);
}

static std::map<hipStream_t, DeviceBuffer> g_hash_io_table;  // per stream, like the work buffers of stark.hip
void release_hash_io_state() {
  for (auto& kv : g_hash_io_table) kv.second.release();
  g_hash_io_table.clear();
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_hash_io_boundary_dev(const uint64_t* trace_lde, size_t col_stride, const uint64_t* pub_lde, unsigned log_n,
                            const uint64_t* alphas_host, const uint64_t* shift_host, const uint64_t* acc, uint64_t* out,
                            void* stream) {
  static const char* who = "sp_hash_io_boundary_dev";
  SP_REQUIRE_READY();
  if (const char* bad = hash_io_dense_check_args(log_n, col_stride, trace_lde, pub_lde, alphas_host, shift_host, out))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)4 << log_n;
  DeviceBuffer& table = g_hash_io_table[st];
  SP_HIP(table.reserve((size_t)3 * HIO_PERIOD * 32));
  HashIoTableParams prm;
  hash_io_table_params(log_n, alphas_host, shift_host, &prm);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(hash_io_table_kernel, dim3(HIO_TABLE_THREADS / HIO_TABLE_TPB), dim3(HIO_TABLE_TPB), 0, st, prm,
                     (uint64_t*)table.ptr);
  hipLaunchKernelGGL(hash_io_dense_kernel, dim3((unsigned)(M / HIO_DENSE_TPB)), dim3(HIO_DENSE_TPB), 0, st, trace_lde,
                     col_stride, pub_lde, M, (const uint64_t*)table.ptr, acc, out);
  if (prof) profile_launch_end(st, M);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_hash_io_boundary_points_dev(unsigned log_n, const uint64_t* coef, const uint64_t* alphas_host,
                                   const uint64_t* shift_host, size_t n_points, const uint64_t* pos, const uint64_t* cur,
                                   uint64_t* out, uint8_t* status, void* stream) {
  static const char* who = "sp_hash_io_boundary_points_dev";
  SP_REQUIRE_READY();
  if (const char* bad = hash_io_points_check_args(log_n, n_points)) return refuse(who, bad);
  if (n_points == 0) return SP_OK;
  if (const char* bad = boundary_points_check_pointers(coef, alphas_host, shift_host, pos, cur, out, status))
    return refuse(who, bad);
  if (const int rc = check_shift(who, shift_host, log_n)) return rc;
  ctx_lock lk(ctx().mu);
  hipStream_t st = (hipStream_t)stream;
  HashIoPointParams prm;
  hash_io_point_params(log_n, alphas_host, shift_host, &prm);
  const bool prof = profile_launch_begin(st);
  hipLaunchKernelGGL(hash_io_points_kernel, dim3((unsigned)n_points), dim3(HIO_POINT_TPB), 0, st, prm, coef, pos, cur,
                     out, status);
  if (prof) profile_launch_end(st, n_points);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

}  // extern "C"
