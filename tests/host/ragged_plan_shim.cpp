// Host build of csrc/ragged_plan.hpp (the per-step fallback plan of the ragged walks) for tests/test_ragged_plan_cpu.py:
//   g++ -O2 -shared -fPIC -o ragged_plan_shim.so ragged_plan_shim.cpp
// With -DRAGGED_PLAN_MAIN it is a stand-alone program that replays a few plans itself - the form to run under
// -fsanitize=address,undefined:
//   g++ -O1 -g -fsanitize=address,undefined -DRAGGED_PLAN_MAIN -o ragged_plan_check ragged_plan_shim.cpp && ./ragged_plan_check
#include "../../stark-perpetual_amd/csrc/ragged_plan.hpp"

extern "C" {
// info[5] = meta length (uint32 words), max_steps, n_pairs, pairs_at, work_felts
void rp_sizes(const uint32_t* off, const uint64_t* keys, size_t n, uint64_t* info) {
  const sp::RaggedPlan p = sp::ragged_plan(off, keys, n);
  info[0] = p.meta.size();
  info[1] = p.max_steps;
  info[2] = p.n_pairs;
  info[3] = p.pairs_at;
  info[4] = p.work_felts;
}
// meta: info[0] words, running: info[1] entries
void rp_fill(const uint32_t* off, const uint64_t* keys, size_t n, uint32_t* meta, uint64_t* running) {
  const sp::RaggedPlan p = sp::ragged_plan(off, keys, n);
  std::memcpy(meta, p.meta.data(), p.meta.size() * sizeof(uint32_t));
  for (size_t s = 0; s < p.max_steps; ++s) running[s] = p.running[s];
}
}

#ifdef RAGGED_PLAN_MAIN
#include <cstdio>
// a non-commutative toy hash on 64-bit words
static uint64_t spy(uint64_t a, uint64_t b) { return 3 * a + 5 * b + 1; }
// Replays the plan on a work buffer of words and compares with the direct fold of every item.
static bool replay(const std::vector<uint32_t>& lens, const std::vector<uint64_t>* keys) {
  const size_t n = lens.size();
  const bool sided = keys != nullptr;
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
  std::vector<uint64_t> words(off[n]), leaves(n);
  for (size_t i = 0; i < words.size(); ++i) words[i] = 1000 + 7 * i;
  for (size_t i = 0; i < n; ++i) leaves[i] = 90000 + 11 * i;
  const sp::RaggedPlan p = sp::ragged_plan(off.data(), sided ? keys->data() : nullptr, n);
  std::vector<uint64_t> work(p.work_felts, 0);
  if (sided) std::copy(leaves.begin(), leaves.end(), work.begin() + n);
  std::copy(words.begin(), words.end(), work.end() - words.size());
  const uint32_t* pairs = p.meta.data() + p.pairs_at;
  for (size_t s = 0; s < p.max_steps; ++s) {
    std::vector<uint64_t> got(p.running[s]);
    for (size_t k = 0; k < p.running[s]; ++k) {
      const uint32_t* pr = pairs + 2 * (p.step_off()[s] + k);
      got[k] = spy(work[pr[0]], work[pr[1]]);
    }
    std::copy(got.begin(), got.end(), work.begin());
  }
  for (size_t k = 0; k < n; ++k) {
    const uint32_t c = p.perm()[k];
    uint64_t want = sided ? leaves[c] : words[off[c]];
    for (uint32_t j = sided ? 0 : 1; j < lens[c]; ++j) {
      const uint64_t w = words[off[c] + j];
      want = sided && (((*keys)[c] >> j) & 1) ? spy(w, want) : spy(want, w);
    }
    const uint32_t steps = lens[c] - (sided ? 0 : 1);
    const uint64_t have = steps == 0 ? (sided ? leaves[c] : words[off[c]]) : work[k];
    if (have != want) return false;
  }
  return true;
}
int main() {
  const std::vector<uint64_t> k4 = {0, 1, 2, ~0ull}, k1 = {0}, k5 = {0, 1, 1ull << 63, 0x5555555555555555ull, 3};
  bool ok = replay({1}, nullptr) && replay({0}, &k1) && replay({3, 3, 3, 3}, nullptr) && replay({1, 2, 64, 2}, nullptr) &&
            replay({0, 1, 2, 64}, &k4) && replay({2, 0, 64, 64, 2}, &k5) && replay({7, 1, 2, 3, 1, 7, 2, 3, 1}, nullptr);
  std::printf(ok ? "ragged_plan check passed\n" : "ragged_plan check FAILED\n");
  return ok ? 0 : 1;
}
#endif
