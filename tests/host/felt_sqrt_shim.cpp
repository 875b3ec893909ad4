// Host-side test shim of the square-root / x-only-key batches: compiles csrc/stark_keys.hpp - the per-item code the
// kernels of csrc/keys.hip run - with g++, bound checks on, and counts every field multiplication and squaring.
// The tables are built here by the same sqrt_tables_build the library calls.  Test infrastructure only.
#define SP_CHECK_BOUNDS 1
#define SP_COUNT_FIELD_OPS 1
#include "../../stark-perpetual_amd/csrc/stark_keys.hpp"
#include <string.h>
using namespace sp;

namespace sp {
long sp_field_ops = 0;
}
static sqrt_tables g_tab;
static bool g_built = false;

template <bool KEY, bool WANT_ROOT>
static void run(const uint32_t* in, uint32_t* out, uint8_t* status, long* ops, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    u256 a, r;
    memcpy(a.w, in + 8 * i, 32);
    sp_field_ops = 0;
    status[i] = stark_key_item<KEY, WANT_ROOT>(a, &g_tab, r);
    if (ops) ops[i] = sp_field_ops;
    if (WANT_ROOT && status[i] == SP_SQRT_OK) memcpy(out + 8 * i, r.w, 32);
  }
}

extern "C" {
// 1 when the tables could be built (the generator check and the hash search of fp29.hpp)
int fs_build(void) {
  if (!g_built) g_built = sqrt_tables_build(g_tab);
  return g_built ? 1 : 0;
}
size_t fs_table_bytes(void) { return sizeof(sqrt_tables); }
uint32_t fs_hash_mult(void) { return g_tab.mult; }
// felts are 8 little-endian 32-bit words; out[i] is written only for status 0; ops[i] = field operations of item i
void fs_sqrt(const uint32_t* a, uint32_t* root, uint8_t* status, long* ops, size_t n) { run<false, true>(a, root, status, ops, n); }
void fs_key_y(const uint32_t* x, uint32_t* y, uint8_t* status, long* ops, size_t n) { run<true, true>(x, y, status, ops, n); }
void fs_is_residue(const uint32_t* a, uint8_t* status, long* ops, size_t n) { run<false, false>(a, nullptr, status, ops, n); }
void fs_key_valid(const uint32_t* x, uint8_t* status, long* ops, size_t n) { run<true, false>(x, nullptr, status, ops, n); }
}
