// Host twin of tests/gpu/field_probe.hip: the same op table (tests/gpu/field_probe_ops.hpp) compiled with g++ and
// the bound checks on (a limb or column that leaves its budget aborts the process), one item at a time - a "wave"
// of one lane, so lehmer_bezout's flag is the value's own.  Build: g++ -O2 -shared -fPIC -I<csrc>.  Test infrastructure only - never loaded by the product.
#define SP_CHECK_BOUNDS 1
#include "../gpu/field_probe_ops.hpp"
#include <string.h>

template <class OP>
static void run_all(const int32_t* in, int32_t* out, long n) {
  for (long item = 0; item < n; ++item) {
    sp::fe v[OP::KIN], o[OP::KOUT + 1];
    int32_t f[OP::NFLAG + 1] = {0};
    memcpy(v, in + item * OP::KIN * sp::NL, sizeof v);
    OP::run(v, o, f);
    int32_t* rec = out + item * (OP::KOUT * sp::NL + OP::NFLAG);
    memcpy(rec, o, sizeof(sp::fe) * OP::KOUT);
    memcpy(rec + OP::KOUT * sp::NL, f, 4 * OP::NFLAG);
  }
}

extern "C" {
// shape[0..2] = KIN, KOUT, NFLAG; returns 0, or -1 for an unknown op
int probe_shape(const char* op, int* shape) {
#define SHAPE(n) \
  if (!strcmp(op, #n)) { shape[0] = probe::op_##n::KIN; shape[1] = probe::op_##n::KOUT; shape[2] = probe::op_##n::NFLAG; return 0; }
  FIELD_PROBE_LANE_OPS(SHAPE)
  return -1;
}
int probe_run(const char* op, const int32_t* in, int32_t* out, long n) {
#define RUN(name) \
  if (!strcmp(op, #name)) { run_all<probe::op_##name>(in, out, n); return 0; }
  FIELD_PROBE_LANE_OPS(RUN)
  return -1;
}
}
