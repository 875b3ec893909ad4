// Device probe of tests/test_gpu_field_probe.py: runs ONE operation of csrc/fp29.hpp, csrc/curve.hpp or
// csrc/quad.hpp on raw limbs read from a file and writes the raw result limbs (and per-item flags) to a file.
//
//   field_probe <op> <in.bin> <out.bin> [n]
//
// in.bin: n records of KIN x 9 little-endian int32 limbs; out.bin: n records of KOUT x 9 limbs + NFLAG int32.
// One kernel launch with 64-lane blocks; exit 0, or non-zero with a message on any HIP error.  Lane-private ops
// (field_probe_ops.hpp) take one record per lane; quad ops take one record per lane of a DPP quad and n must be a
// multiple of four: the guard is per quad, so all four lanes of a quad are active or none.  Both guards sit in
// front of the arithmetic, as in the library's kernels: a last partial wave runs the wave votes with lanes off.
// Test infrastructure only - never loaded by the product.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I<csrc> field_probe.hip -o field_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "quad.hpp"
#include "field_probe_ops.hpp"

namespace probe {

// ---- quad ops: device only.  k = lane & 3; v, o, f are the lane's own record ----
#define PROBE_QOP(name, kin, kout, nflag)                       \
  struct qop_##name {                                           \
    static constexpr int KIN = kin, KOUT = kout, NFLAG = nflag; \
    static __device__ __forceinline__ void run(const fe* v, fe* o, int32_t* f, int k); \
  };                                                            \
  __device__ __forceinline__ void qop_##name::run(const fe* v, fe* o, int32_t* f, int k)

// flag 0: what the lane-private lehmer_bezout of the same wave answers for the same values (the quad forms run
// the same lehmer_batch on the same doubles and fall back on the same vote)
__device__ __forceinline__ int32_t bezout_flag(const fe& x) {
  fe D;
  int32_t sf;
  return lehmer_bezout(FE_P, x, D, sf);
}
PROBE_QOP(inv_plain_quad, 1, 1, 1) { o[0] = fe_inv_plain_quad(v[0], k); f[0] = bezout_flag(v[0]); }
PROBE_QOP(inv_plain_quad_divsteps, 1, 1, 1) { o[0] = fe_inv_plain_quad_divsteps(v[0], k); f[0] = bezout_flag(v[0]); }
PROBE_QOP(inv_quad, 1, 1, 1) { o[0] = fe_inv_quad<false>(v[0], k); f[0] = bezout_flag(v[0]); }
PROBE_QOP(inv_quad_plain, 1, 1, 1) { o[0] = fe_inv_quad<true>(v[0], k); f[0] = bezout_flag(v[0]); }
PROBE_QOP(inv_shared_quad_1, 1, 1, 0) { (void)f; o[0] = fe_inv_shared_quad<1, false>(v[0], k); }
PROBE_QOP(inv_shared_quad_1_plain, 1, 1, 0) { (void)f; o[0] = fe_inv_shared_quad<1, true>(v[0], k); }
PROBE_QOP(inv_shared_quad_2, 1, 1, 0) { (void)f; o[0] = fe_inv_shared_quad<2, false>(v[0], k); }
PROBE_QOP(inv_shared_quad_2_plain, 1, 1, 0) { (void)f; o[0] = fe_inv_shared_quad<2, true>(v[0], k); }
// qpt layout in and out (a, b); flag: fe_is_zero of the lane's b (ZZ3 or ZZZ3)
PROBE_QOP(qadd, 2, 2, 1) {
  const qpt r = qadd<false>(qpt{v[0], v[1]}, k);
  o[0] = r.a; o[1] = r.b;
  f[0] = fe_is_zero(r.b);
}
PROBE_QOP(qadd_x_only, 2, 2, 1) {
  const qpt r = qadd<true>(qpt{v[0], v[1]}, k);
  o[0] = r.a; o[1] = r.b;
  f[0] = fe_is_zero(r.b);
}
PROBE_QOP(qmmadd, 4, 2, 1) {  // the lane's own pair: x1 y1 x2 y2
  const qpt r = qmmadd(v[0], v[1], v[2], v[3], k);
  o[0] = r.a; o[1] = r.b;
  f[0] = fe_is_zero(r.b);
}
#define FIELD_PROBE_QUAD_OPS(X)                                                                        \
  X(inv_plain_quad) X(inv_plain_quad_divsteps) X(inv_quad) X(inv_quad_plain) X(inv_shared_quad_1)    \
  X(inv_shared_quad_1_plain) X(inv_shared_quad_2) X(inv_shared_quad_2_plain) X(qadd) X(qadd_x_only) X(qmmadd)

template <class OP>
__device__ __forceinline__ void load(const int32_t* in, long item, fe* v) {
#pragma unroll
  for (int e = 0; e < OP::KIN; ++e)
#pragma unroll
    for (int i = 0; i < NL; ++i) v[e].l[i] = in[(item * OP::KIN + e) * NL + i];
}
template <class OP>
__device__ __forceinline__ void store(int32_t* out, long item, const fe* o, const int32_t* f) {
  int32_t* rec = out + item * (OP::KOUT * NL + OP::NFLAG);
#pragma unroll
  for (int e = 0; e < OP::KOUT; ++e)
#pragma unroll
    for (int i = 0; i < NL; ++i) rec[e * NL + i] = o[e].l[i];
#pragma unroll
  for (int e = 0; e < OP::NFLAG; ++e) rec[OP::KOUT * NL + e] = f[e];
}

template <class OP>
__global__ void __launch_bounds__(64) lane_kernel(const int32_t* in, int32_t* out, long n) {
  const long item = (long)blockIdx.x * 64 + threadIdx.x;
  if (item >= n) return;
  fe v[OP::KIN], o[OP::KOUT + 1];
  int32_t f[OP::NFLAG + 1] = {0};
  load<OP>(in, item, v);
  OP::run(v, o, f);
  store<OP>(out, item, o, f);
}
template <class OP>
__global__ void __launch_bounds__(64) quad_kernel(const int32_t* in, int32_t* out, long n) {
  const long item = (long)blockIdx.x * 64 + threadIdx.x;
  if ((item >> 2) >= (n >> 2)) return;  // per quad: n is a multiple of four
  fe v[OP::KIN], o[OP::KOUT + 1];
  int32_t f[OP::NFLAG + 1] = {0};
  load<OP>(in, item, v);
  OP::run(v, o, f, (int)(threadIdx.x & 3));
  store<OP>(out, item, o, f);
}

}  // namespace probe

#define CHECK(expr)                                                                        \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess) {                                                               \
      fprintf(stderr, "field_probe: %s: %s\n", #expr, hipGetErrorString(e__));             \
      exit(3);                                                                             \
    }                                                                                      \
  } while (0)

typedef void (*kernel_t)(const int32_t*, int32_t*, long);
struct entry {
  const char* name;
  int kin, kout, nflag;
  bool quad;
  kernel_t kernel;
};
#define LANE_ENTRY(n) {#n, probe::op_##n::KIN, probe::op_##n::KOUT, probe::op_##n::NFLAG, false, probe::lane_kernel<probe::op_##n>},
#define QUAD_ENTRY(n) {#n, probe::qop_##n::KIN, probe::qop_##n::KOUT, probe::qop_##n::NFLAG, true, probe::quad_kernel<probe::qop_##n>},
static const entry TABLE[] = {FIELD_PROBE_LANE_OPS(LANE_ENTRY) FIELD_PROBE_QUAD_OPS(QUAD_ENTRY)};

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--list")) {  // name kin kout nflag quad: no GPU needed
    for (const entry& e : TABLE) printf("%s %d %d %d %d\n", e.name, e.kin, e.kout, e.nflag, (int)e.quad);
    return 0;
  }
  if (argc < 4 || argc > 5) {
    fprintf(stderr, "usage: field_probe <op> <in.bin> <out.bin> [n]\n");
    return 2;
  }
  const entry* op = nullptr;
  for (const entry& e : TABLE)
    if (!strcmp(e.name, argv[1])) op = &e;
  if (!op) {
    fprintf(stderr, "field_probe: no op %s\n", argv[1]);
    return 2;
  }
  FILE* fi = fopen(argv[2], "rb");
  if (!fi) {
    fprintf(stderr, "field_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  fseek(fi, 0, SEEK_END);
  const long bytes = ftell(fi);
  fseek(fi, 0, SEEK_SET);
  const long rec_in = (long)op->kin * sp::NL * 4, rec_out = ((long)op->kout * sp::NL + op->nflag) * 4;
  const long have = bytes / rec_in;
  const long n = argc == 5 ? atol(argv[4]) : have;
  if (n <= 0 || n > have || bytes % rec_in != 0) {
    fprintf(stderr, "field_probe: %s holds %ld records of %ld bytes, n = %ld\n", argv[2], have, rec_in, n);
    return 2;
  }
  if (op->quad && n % 4 != 0) {
    fprintf(stderr, "field_probe: %s is a quad op, n = %ld leaves a quad with lanes off\n", op->name, n);
    return 2;
  }
  std::vector<int32_t> hin((size_t)(n * rec_in / 4)), hout((size_t)(n * rec_out / 4));
  if (fread(hin.data(), 1, (size_t)(n * rec_in), fi) != (size_t)(n * rec_in)) {
    fprintf(stderr, "field_probe: short read\n");
    return 2;
  }
  fclose(fi);
  int32_t *din, *dout;
  CHECK(hipMalloc(&din, (size_t)(n * rec_in)));
  CHECK(hipMalloc(&dout, (size_t)(n * rec_out)));
  CHECK(hipMemcpy(din, hin.data(), (size_t)(n * rec_in), hipMemcpyHostToDevice));
  CHECK(hipMemset(dout, 0, (size_t)(n * rec_out)));
  op->kernel<<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(din, dout, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(hout.data(), dout, (size_t)(n * rec_out), hipMemcpyDeviceToHost));
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
  FILE* fo = fopen(argv[3], "wb");
  if (!fo || fwrite(hout.data(), 1, (size_t)(n * rec_out), fo) != (size_t)(n * rec_out) || fclose(fo) != 0) {
    fprintf(stderr, "field_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
