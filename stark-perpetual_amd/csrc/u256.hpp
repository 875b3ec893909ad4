// Comparisons of plain 256-bit integers on packed words, and the three bounds the entry points test against.
// Host and device: the kernels use them, and so does the per-item code that the host tests compile with g++.
#pragma once
#include "fp29.hpp"

namespace sp {

// plain integer a < 2^256 compared with p / N / 2^251 on packed words
SP_HD bool u256_lt(const u256& a, const u256& b) {
  bool lt = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (a.w[i] != b.w[i]) lt = a.w[i] < b.w[i];  // highest differing word decides
  }
  return lt;
}
SP_HD bool u256_is_zero(const u256& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.w[i];
  return o == 0;
}
constexpr u256 U256_P = {{1u, 0u, 0u, 0u, 0u, 0u, 0x11u, 0x08000000u}};
constexpr u256 U256_N = {{0xadc64d2fu, 0x1e66a241u, 0xcae7b232u, 0xb781126du, 0xffffffffu, 0xffffffffu,
                          0x10u, 0x08000000u}};
constexpr u256 U256_2P251 = {{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0x08000000u}};

}  // namespace sp
