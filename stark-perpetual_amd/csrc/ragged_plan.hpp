// The per-step fallback of the ragged walks (chains of unequal length, Merkle paths) as a plan: pure host integer
// code, nothing from HIP, so that a plain C++ compiler builds it for the CPU tests (tests/host/ragged_plan_shim.cpp).
//
// The items are sorted by falling step count (a stable sort: ties keep the caller's order), so that the items still
// running at step s are a prefix of the sorted order; step s is one gathered Pedersen launch over that prefix, whose
// index pairs address ONE work buffer of felts:
//   [0, n)                    the running values, in sorted order (written by every step)
//   paths only: [n, 2 n)      the leaves, in the caller's order
//   then `off[n]` felts       the caller's words (a chain's elements / a path's siblings), unchanged
// A chain of len words takes len - 1 steps from its first word; a path of len siblings takes len steps from its leaf,
// and the pair of a step is swapped where the path's side bit of that step is set (the running node is the RIGHT
// child).  A last launch puts values and status bytes back in the caller's order through `perm`.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sp {

struct RaggedPlan {
  // one copy to the device: off[n + 1] | perm[n] | step_off[max_steps] | (pad to 8 bytes) | index pairs (2 x n_pairs)
  std::vector<uint32_t> meta;
  std::vector<size_t> running;  // running[s] = items of more than s steps = the size of step s's launch
  size_t n = 0, max_steps = 0;
  size_t n_pairs = 0;     // sum of running[] = all hashes of the call = the step status bytes
  size_t pairs_at = 0;    // where the pairs start in `meta` (even: a pair is loaded as one 8-byte int2)
  size_t work_felts = 0;  // felts of the work buffer
  const uint32_t* perm() const { return meta.data() + n + 1; }          // sorted position k holds item perm[k]
  const uint32_t* step_off() const { return meta.data() + 2 * n + 1; }  // step s: pairs and status bytes from here
};

// off = n + 1 validated offsets (n >= 1), keys = the paths' side bits or null for chains.  The caller has checked
// that the work buffer stays below 2^31 felts (ragged_work_felts): the gathered launches index it with an int.
inline size_t ragged_work_felts(const uint32_t* off, size_t n, bool sided) { return (sided ? 2 * n : n) + off[n]; }
inline RaggedPlan ragged_plan(const uint32_t* off, const uint64_t* keys, size_t n) {
  const bool sided = keys != nullptr;
  const uint32_t lone = sided ? 0 : 1;  // words of an item that are no step: a chain's first word is its start value
  auto steps_of = [&](uint32_t c) { return (size_t)(off[c + 1] - off[c] - lone); };
  RaggedPlan p;
  p.n = n;
  p.work_felts = ragged_work_felts(off, n, sided);
  std::vector<uint32_t> perm(n);
  for (size_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return steps_of(a) > steps_of(b); });
  p.max_steps = steps_of(perm[0]);
  p.n_pairs = (size_t)off[n] - lone * n;
  p.pairs_at = (2 * n + 1 + p.max_steps + 1) & ~(size_t)1;
  p.meta.assign(p.pairs_at + 2 * p.n_pairs, 0);
  std::memcpy(p.meta.data(), off, (n + 1) * sizeof(uint32_t));
  std::memcpy(p.meta.data() + n + 1, perm.data(), n * sizeof(uint32_t));
  uint32_t* step_off = p.meta.data() + 2 * n + 1;
  uint32_t* pairs = p.meta.data() + p.pairs_at;
  p.running.assign(p.max_steps, 0);
  const uint32_t words_at = (uint32_t)(sided ? 2 * n : n);
  size_t m = n, pos = 0;
  for (size_t s = 0; s < p.max_steps; ++s) {
    while (m > 0 && steps_of(perm[m - 1]) <= s) --m;
    p.running[s] = m;
    step_off[s] = (uint32_t)pos;
    for (size_t k = 0; k < m; ++k) {
      const uint32_t c = perm[k], first = words_at + off[c];
      // the start value (a path's leaf, a chain's first word), later the running value
      const uint32_t h = s != 0 ? (uint32_t)k : (sided ? (uint32_t)n + c : first);
      const uint32_t w = first + lone + (uint32_t)s;  // the word of this step
      const bool right = sided && ((keys[c] >> s) & 1) != 0;
      pairs[2 * (pos + k)] = right ? w : h;
      pairs[2 * (pos + k) + 1] = right ? h : w;
    }
    pos += m;
  }
  return p;
}

}  // namespace sp
