// Host-side test shim of the batch point arithmetic: compiles csrc/ec_points.hpp - the per-item code the kernels of
// csrc/ec_points.hip run, with the verifier's ladder of csrc/ladder.hpp under it - with g++, bound checks on.  The
// ladder's table is a plain array here (n = 1, e = 0).  Test infrastructure only.
//
// NOT covered here: the table walk of gen_mul (csrc/gen_mul.hpp).  The EC_GEN window table exists on the device only,
// so the fixed-base term a EC_GEN of ep_lincomb comes from hostcurve.hpp's affine double-and-add instead; the walk
// itself is covered by tests/test_gpu_ec_points.py.
#define SP_CHECK_BOUNDS 1
#include "../../stark-perpetual_amd/csrc/ec_points.hpp"
#include "../../stark-perpetual_amd/csrc/hostcurve.hpp"
#include <string.h>
using namespace sp;

static int32_t g_tab[8 * 36];

static u256 felt(const uint32_t* p, size_t i) {
  u256 a;
  memcpy(a.w, p + 8 * i, 32);
  return a;
}
static void put(uint8_t code, const u256& x, const u256& y, uint32_t* rx, uint32_t* ry, uint8_t* status, size_t i) {
  status[i] = code;
  if (code != SP_EC_OK) return;
  memcpy(rx + 8 * i, x.w, 32);
  if (ry) memcpy(ry + 8 * i, y.w, 32);
}

extern "C" {
// felts are 8 little-endian 32-bit words; rx[i] / ry[i] are written only for status 0; ry may be null
void ep_mult(const uint32_t* k, const uint32_t* px, const uint32_t* py, uint32_t* rx, uint32_t* ry, uint8_t* status,
             size_t n) {
  for (size_t i = 0; i < n; ++i) {
    u256 x, y;
    const uint8_t code = ec_mult_item(felt(k, i), felt(px, i), felt(py, i), g_tab, 1, 0, x, y);
    put(code, x, y, rx, ry, status, i);
  }
}
void ep_lincomb(const uint32_t* a, const uint32_t* b, const uint32_t* px, const uint32_t* py, uint32_t* rx,
                uint32_t* ry, uint8_t* status, size_t n) {
  const haff gen = h_make(PT_GEN_X, PT_GEN_Y);
  auto gen_mul_of = [&](const u256& s) {
    uint64_t k[4];
    for (int i = 0; i < 4; ++i) k[i] = (uint64_t)s.w[2 * i] | ((uint64_t)s.w[2 * i + 1] << 32);
    const haff r = h_mul(k, gen);
    aff q;
    q.x = r.x;
    q.y = r.y;
    return xyzz_from_aff(q);
  };
  for (size_t i = 0; i < n; ++i) {
    u256 x, y;
    const uint8_t code = ec_lincomb_item(felt(a, i), felt(b, i), felt(px, i), felt(py, i), gen_mul_of, g_tab, 1, 0, x, y);
    put(code, x, y, rx, ry, status, i);
  }
}
void ep_add(const uint32_t* px, const uint32_t* py, const uint32_t* qx, const uint32_t* qy, int subtract, uint32_t* rx,
            uint32_t* ry, uint8_t* status, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    u256 x, y;
    const uint8_t code = ec_add_item(felt(px, i), felt(py, i), felt(qx, i), felt(qy, i), subtract != 0, x, y);
    put(code, x, y, rx, ry, status, i);
  }
}
}
