// ISA probe for tests/test_field_scan_isa_cpu.py: one kernel per field operation and nothing else that
// multiplies, so the opcode counts of a kernel are the counts of its operation.  PROBE_SCAN=1 builds the
// product-scanning forms of csrc/fp29.hpp, PROBE_SCAN=0 the column forms (fe_reduce with its carry additions).
// Never launched.
#include "fp29.hpp"
using namespace sp;

#ifndef PROBE_SCAN
#define PROBE_SCAN 1
#endif

__device__ __forceinline__ fe probe_load(const int32_t* p) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = p[(size_t)i * 64 + threadIdx.x];
  fe_pin(r);
  return r;
}
__device__ __forceinline__ void probe_store(int32_t* p, const fe& r) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[(size_t)i * 64 + threadIdx.x] = r.l[i];
}

extern "C" __global__ void __launch_bounds__(64) probe_fe_mul(const int32_t* a, const int32_t* b, int32_t* out) {
  probe_store(out, fe_mul_t<PROBE_SCAN != 0>(probe_load(a), probe_load(b)));
}
extern "C" __global__ void __launch_bounds__(64) probe_fe_sqr(const int32_t* a, int32_t* out) {
  probe_store(out, fe_sqr_t<PROBE_SCAN != 0>(probe_load(a)));
}
extern "C" __global__ void __launch_bounds__(64)
probe_fe_mul_sub_mul(const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out) {
  probe_store(out, fe_mul_sub_mul_t<PROBE_SCAN != 0>(probe_load(a), probe_load(b), probe_load(c), probe_load(d)));
}
