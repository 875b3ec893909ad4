// Sparse Merkle multi-update: root of a height-h (h <= 64) Pedersen tree that holds the given
// leaves at the given keys and `empty_leaf` everywhere else.
//
// Reference shape: cairo-lang's merkle_multi_update as called from
// services/perpetual/cairo/state/state.cairo:155-173 (positions tree, orders tree, height 64);
// the hint-side helper starkware/python/merkle_tree.py:4-26 builds the subtree induced by the
// modified leaves level by level (parents = set(index // 2)).  Same walk here: the host does the
// integer bookkeeping of which two children feed each induced node (the merkle_tree.py part),
// the GPU does every hash: per level one pair of Pedersen launches whose accumulate kernel picks its
// operands through the host's child-index list (gathered mode of csrc/pedersen.hip).
#include <algorithm>
#include <climits>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "context.hpp"
#include "pedersen.hpp"

namespace sp {

// empty-subtree roots are a pure function of the empty leaf: cached on the host per leaf value
static std::map<std::vector<uint64_t>, std::vector<uint64_t>> g_empty_cache;  // leaf -> 65 felts
// Work buffer of sp_merkle_verify_update[_dev], one per stream like the hash scratch: roots | node indices | child lists
// | hashes | their status bytes.  It grows as a tree's slot table does (RetiringBuffer of context.hpp); keys and roots
// reach it through the stream's page-locked buffer (stage_copy of pedersen.hpp).
using VerifyWork = RetiringBuffer<char>;
static std::map<StreamKey, VerifyWork> g_verify_work;
void release_merkle_state() {
  g_empty_cache.clear();
  for (auto& kv : g_verify_work) kv.second.release();
  g_verify_work.clear();
}

}  // namespace sp

using namespace sp;

// host-side range check of a caller's felt (signature.py:307: hash inputs are in [0, p))
static bool felt_below_p(const uint64_t* v) {
  static const uint64_t P[4] = {1ull, 0ull, 0ull, 0x0800000000000011ull};
  for (int i = 3; i >= 0; --i) {
    if (v[i] != P[i]) return v[i] < P[i];
  }
  return false;
}

// The one key check: every key below 2^height and, where the call walks the keys' induced subtree (`ordered`), the keys
// strictly increasing.  false: the text is in sp_last_error.
static bool keys_ok(unsigned height, const uint64_t* keys, size_t n, bool ordered) {
  for (size_t i = 0; i < n; ++i) {
    if (ordered && i > 0 && keys[i] <= keys[i - 1]) { set_error("keys must be strictly increasing"); return false; }
    if (height < 64 && (keys[i] >> height) != 0) { set_error("key out of range for height"); return false; }
  }
  return true;
}

// empty-subtree roots: empties[k+1] = H(empties[k], empties[k]); 64 sequential hashes on `st` the first
// time a given empty leaf is seen, then served from the host-side cache (65 felts per leaf value).  The caller
// holds the library lock (the cache is shared); `s` is the scratch of `st`.
static int empty_roots(const uint64_t* empty_leaf, const Scratch& s, hipStream_t st, const std::vector<uint64_t>** out) {
  std::vector<uint64_t> key(empty_leaf, empty_leaf + 4);
  auto it = g_empty_cache.find(key);
  if (it == g_empty_cache.end()) {
    uint64_t* d_full = nullptr;
    SP_HIP(hipMalloc(&d_full, 65 * 32));
    SP_HIP(hipMemcpyAsync(d_full, key.data(), 32, hipMemcpyHostToDevice, st));
    for (unsigned k2 = 0; k2 < 64; ++k2) {
      const int rc = enqueue_pedersen(d_full + 4 * k2, 1, d_full + 4 * k2, 1, d_full + 4 * (k2 + 1), 1, nullptr,
                                      s.flag, 1, st, s, nullptr);
      if (rc != SP_OK) { (void)hipFree(d_full); return rc; }
    }
    std::vector<uint64_t> all(65 * 4);
    SP_HIP(hipMemcpyAsync(all.data(), d_full, 65 * 32, hipMemcpyDeviceToHost, st));
    SP_HIP(hipStreamSynchronize(st));
    (void)hipFree(d_full);
    it = g_empty_cache.emplace(key, all).first;
  }
  *out = &it->second;
  return SP_OK;
}

extern "C" int sp_merkle_sparse_root(const uint64_t* keys, const uint64_t* leaves, size_t n,
                                     unsigned height, const uint64_t* empty_leaf, uint64_t* root,
                                     uint8_t* status) {
  LaneScope ls(ctx_current());
  SP_REQUIRE_READY();
  if (height > 64) { set_error("height must be <= 64"); return SP_ERR_BAD_ARGUMENT; }
  if (!felt_below_p(empty_leaf)) { set_error("empty leaf must be a field element (< p)"); return SP_ERR_BAD_ARGUMENT; }
  if (!keys_ok(height, keys, n, true)) return SP_ERR_BAD_ARGUMENT;
  if (ls.open() != SP_OK) return SP_ERR_HIP;
  HostLane& L = *ls.lane;
  hipStream_t st = L.stream;
  // ---- host bookkeeping: induced subtree (merkle_tree.py:18-26) ----
  std::vector<uint64_t> idx(keys, keys + n);
  std::vector<int2> src;                 // all levels, concatenated
  std::vector<size_t> level_off, level_cnt;
  for (unsigned l = 0; l < height && !idx.empty(); ++l) {
    std::vector<uint64_t> nxt;
    nxt.reserve(idx.size());
    level_off.push_back(src.size());
    const size_t m = idx.size();
    for (size_t j = 0; j < m;) {
      int2 s;
      if ((idx[j] & 1) == 0) {
        s.x = (int)j;
        if (j + 1 < m && idx[j + 1] == idx[j] + 1) { s.y = (int)(j + 1); nxt.push_back(idx[j] >> 1); j += 2; }
        else { s.y = -1; nxt.push_back(idx[j] >> 1); j += 1; }
      } else {
        s.x = -1; s.y = (int)j; nxt.push_back(idx[j] >> 1); j += 1;
      }
      src.push_back(s);
    }
    level_cnt.push_back(nxt.size());
    idx.swap(nxt);
  }
  // ---- the stream's scratch and the empty-subtree roots (a copy: the cache is the lock's) ----
  const size_t emp_bytes = ((size_t)height + 1) * 32;
  std::vector<uint64_t> emp;
  Scratch s;
  {
    ctx_lock lk(ctx().mu);
    int rc = get_scratch_public(n ? n : 1, s, st);
    if (rc != SP_OK) return rc;
    SP_HIP(hipMemsetAsync(s.flag, 0, sizeof(unsigned), st));
    const std::vector<uint64_t>* all = nullptr;
    rc = empty_roots(empty_leaf, s, st, &all);
    if (rc != SP_OK) return rc;
    emp.assign(all->begin(), all->begin() + emp_bytes / 8);
  }
  unsigned f = 0;
  if (n == 0) {  // nothing to hash: the root of the empty tree
    std::memcpy(root, &emp[4 * (size_t)height], 32);
  } else {
    // ---- lane buffer: empties[height + 1] | child lists | leaves (= ping) : what goes up, one piece | pong | points ----
    const size_t fb = n * 32, src_used = src.size() * sizeof(int2);
    const size_t src_bytes = (src_used + sizeof(int2) + 63) & ~(size_t)63;
    const size_t cpt_bytes = 2 * ((size_t)height + 1) * sizeof(aff_packed);
    const size_t in_bytes = emp_bytes + src_bytes + fb;
    SP_HIP(L.io.reserve(in_bytes + fb + cpt_bytes + 1024));
    char* b = (char*)L.io.ptr;
    uint64_t* d_emp = (uint64_t*)b;
    int2* d_src = (int2*)(b + emp_bytes);
    uint64_t* d_a = (uint64_t*)(b + emp_bytes + src_bytes);
    uint64_t* d_b = (uint64_t*)(b + in_bytes);
    // the constant points of the levels (SPARSE quad kernel, pedersen.hip), 64-byte aligned behind the values
    aff_packed* d_cpts = (aff_packed*)(((uintptr_t)(b + in_bytes + fb) + 63) & ~(uintptr_t)63);
    StagedTrip trip(L.hio, in_bytes, st);
    SP_HIP(trip.up(d_emp, {{emp.data(), emp_bytes}, {src.data(), src_used}, {nullptr, src_bytes - src_used}, {leaves, fb}}));
    uint64_t *cur = d_a, *nxt = d_b;
    {
      ctx_lock lk(ctx().mu);
      bool have_cpts = false;
      if (height > 0) {
        const int rc = enqueue_partial_points(d_emp, (int)height, d_cpts, st, &have_cpts);
        if (rc != SP_OK) return rc;
      }
      for (size_t l = 0; l < level_cnt.size(); ++l) {
        // gathered mode: operand pointers come from src (children in `cur`, or this level's
        // empty-subtree root) inside the accumulate kernel - no separate gather pass
        const int rc = enqueue_pedersen_sparse(cur, d_emp + 4 * l, nxt, s.flag, level_cnt[l], st, s, d_src + level_off[l],
                                               have_cpts ? d_cpts + 2 * l : nullptr);
        if (rc != SP_OK) return rc;
        std::swap(cur, nxt);
      }
    }
    // the root sits in whichever of ping and pong was written last: two small copies, not a staged piece
    SP_HIP(hipMemcpyAsync(root, cur, 32, hipMemcpyDeviceToHost, st));
    SP_HIP(hipMemcpyAsync(&f, s.flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    SP_HIP(hipStreamSynchronize(st));
  }
  if (status) *status = (uint8_t)f;
  return SP_OK;
}

// =================================================================================================
// Persistent sparse trees: merkle_multi_update on a tree that already holds state.
//
// services/perpetual/cairo/state/state.cairo:155-173 updates the positions tree and the orders
// tree (height 64) once per batch: old root and new root along the union of the touched paths, the
// untouched siblings coming from the previous state (the `merkle_facts` store of main.cairo:61-64).
// sp_merkle_sparse_root only covers the first batch (everything else empty).  A tree handle keeps
// the state IN HBM: an open-addressing hash table (level, index) -> felt of every node that differs
// from the empty-subtree root of its level.  An update ships the sorted keys and the new leaves
// (40 B per leaf) and runs entirely on the device:
//   per level   tree_level_kernel: from the level's sorted node indices builds the parents' indices
//               (merkle_tree.py:18-26: parents = set(index // 2)), the child-index list of every parent
//               and looks the untouched siblings up in the table;
//               the gathered Pedersen launch of csrc/pedersen.hip hashes the level;
//   at the end  one insert kernel writes the new leaves and every new node into the table - only if no
//               input was out of range / unhashable, so a failed update leaves the tree as it was.
// The host only counts the nodes per level (a function of the keys alone) to size the launches, and
// keeps a copy of the current root.  Round 1 kept the node store in host maps: 12 ms per 4096-leaf update
// of a height-64 tree, most of it map lookups / insertions and the 8 MB of values crossing PCIe.
struct TreeSlot {       // 48 bytes
  uint64_t index;
  uint32_t level1;      // level + 1; 0 = never used
  uint32_t state;       // 0 empty, 1 being written, 2 ready
  uint64_t value[4];
};
__device__ __forceinline__ uint64_t tree_mix(uint64_t index, uint32_t level) {
  uint64_t z = index + 0x9E3779B97F4A7C15ull * (uint64_t)(level + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// value of node (level, index) or nullptr when the node is still the empty-subtree root of its level
__device__ __forceinline__ const uint64_t* tree_find(const TreeSlot* __restrict__ tab, uint64_t mask, uint32_t level,
                                                     uint64_t index) {
  for (uint64_t i = tree_mix(index, level) & mask;; i = (i + 1) & mask) {
    const TreeSlot& sl = tab[i];
    // lookups never run beside insertions (different launches of one stream): plain loads
    const uint32_t st = sl.state;
    if (st == 0) return nullptr;
    if (st == 2 && sl.level1 == level + 1 && sl.index == index) return sl.value;
  }
}
// Inserts or overwrites; the keys of one launch are distinct, so two lanes never claim the same key.
__device__ __forceinline__ bool tree_put(TreeSlot* __restrict__ tab, uint64_t mask, uint32_t level, uint64_t index,
                                         const uint64_t* value) {
  for (uint64_t i = tree_mix(index, level) & mask;; i = (i + 1) & mask) {
    TreeSlot& sl = tab[i];
    // relaxed: a slot another lane is filling right now belongs to a different key (the keys of a launch
    // are distinct), so whatever is read from it cannot match
    uint32_t st = __hip_atomic_load(&sl.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (st == 0) {
      uint32_t expected = 0;
      if (__hip_atomic_compare_exchange_strong(&sl.state, &expected, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        sl.index = index;
        sl.level1 = level + 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) sl.value[q] = value[q];
        __hip_atomic_store(&sl.state, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // readers: later launches
        return true;  // a slot that was empty: the table's entry count grows
      }
      st = expected;  // somebody else claimed it: a different key (keys are distinct), keep probing
    }
    if (st == 2 && sl.level1 == level + 1 && sl.index == index) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sl.value[q] = value[q];
      return false;
    }
  }
}

// Layout of one update in the work buffer (host-computed from the level counts, uploaded once).
struct TreeLevels {
  unsigned height;
  unsigned cnt[66];       // nodes per level (level 0 = the new leaves)
  int val_base[66];       // felts: where the values of level l start
  int sib_base[66];       // felts: where the siblings of level l + 1's parents go (one slot per parent)
  unsigned idx_off[66];   // idx: where the node indices of level l start
  unsigned src_off[66];   // src: where the child lists of level l + 1 start
};

// The structure of the whole update is built before any hash runs (it depends on the sorted keys only), level-
// PARALLEL: the nodes of level l are the distinct values of key >> l, in order, so
//   tree_level_nodes_kernel   block l (one workgroup per level) writes the node indices of level l with a
//                             ballot scan over the keys - no level waits for another (round 2 walked the levels
//                             one after the other in ONE workgroup: 370 us of a 3.5 ms update);
//   tree_children_kernel      one thread per node of levels 0 .. height - 1: a node that opens a new parent
//                             (merkle_tree.py:18-26) finds the parent's position by binary search in the next
//                             level's (sorted) node list and writes its child list - absolute positions in
//                             `felts`, TREE_PENDING = the sibling comes from the table (tree_lookup_kernel).
constexpr int TREE_PENDING = INT_MIN;
__global__ void __launch_bounds__(1024)
tree_level_nodes_kernel(TreeLevels lv, const uint64_t* __restrict__ keys, uint64_t* __restrict__ idx_all) {
  __shared__ unsigned wave_tot[16];
  __shared__ unsigned carry;
  const unsigned level = blockIdx.x + 1;  // 1 .. height (level 0 = the keys themselves, already in place)
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned n = lv.cnt[0];
  uint64_t* out = idx_all + lv.idx_off[level];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (unsigned tile = 0; tile < n; tile += 1024) {
    const unsigned i = tile + threadIdx.x;
    const bool live = i < n;
    const uint64_t me = live ? (level < 64 ? keys[i] >> level : 0) : 0;
    const bool head = live && (i == 0 || (level < 64 ? keys[i - 1] >> level : 0) != me);
    const unsigned long long ballot = __ballot(head);
    const unsigned before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(ballot);
    __syncthreads();
    unsigned off = carry;
    for (unsigned w = 0; w < wave; ++w) off += wave_tot[w];
    if (head) out[off + before] = me;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = carry;
      for (unsigned w = 0; w < 16; ++w) tot += wave_tot[w];
      carry = tot;
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256)
tree_children_kernel(TreeLevels lv, const uint64_t* __restrict__ idx_all, int2* __restrict__ src_all, unsigned n_nodes) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;  // node number over levels 0 .. height - 1
  if (g >= n_nodes) return;
  unsigned level = 0;
  while (level + 1 < lv.height && g >= lv.idx_off[level + 1]) ++level;  // idx_off is the running node count
  const unsigned j = g - lv.idx_off[level], cnt = lv.cnt[level];
  const uint64_t* idx = idx_all + lv.idx_off[level];
  const uint64_t me = idx[j];
  // a node opens a new parent unless its left neighbour in the array is its left sibling
  if ((me & 1) && j > 0 && idx[j - 1] == me - 1) return;
  const uint64_t* par = idx_all + lv.idx_off[level + 1];
  unsigned lo = 0, hi = lv.cnt[level + 1];
  while (lo < hi) {  // first parent >= me >> 1 (it is there)
    const unsigned mid = (lo + hi) >> 1;
    if (par[mid] < (me >> 1)) lo = mid + 1; else hi = mid;
  }
  const int val_base = lv.val_base[level];
  int2 s2;
  if ((me & 1) == 0) {
    s2.x = val_base + (int)j;
    s2.y = (j + 1 < cnt && idx[j + 1] == me + 1) ? val_base + (int)j + 1 : TREE_PENDING;
  } else {
    s2.y = val_base + (int)j;
    s2.x = TREE_PENDING;
  }
  src_all[lv.src_off[level] + lo] = s2;
}

// Every parent whose child list has a pending side: the untouched sibling from the table (copied to
// felts[sib_base + q]) or -1 = the level's empty-subtree root.  One thread per parent of the update.
__global__ void __launch_bounds__(256)
tree_lookup_kernel(TreeLevels lv, const uint64_t* __restrict__ idx_all, const TreeSlot* __restrict__ tab, uint64_t mask,
                   uint64_t* __restrict__ felts, int2* __restrict__ src_all, unsigned n_parents) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_parents) return;
  unsigned level = 0;  // children's level: src_off is the running parent count
  while (level + 1 < lv.height && g >= lv.src_off[level + 1]) ++level;
  const unsigned q = g - lv.src_off[level];
  int2 s2 = src_all[g];
  if (s2.x != TREE_PENDING && s2.y != TREE_PENDING) return;
  const uint64_t parent = idx_all[lv.idx_off[level + 1] + q];
  const bool left = s2.x == TREE_PENDING;
  const uint64_t* sib = tree_find(tab, mask, level, 2 * parent + (left ? 0 : 1));
  const int pos = sib ? lv.sib_base[level] + (int)q : -1;
  if (sib) {
#pragma unroll
    for (int w = 0; w < 4; ++w) felts[4 * (size_t)pos + w] = sib[w];
  }
  if (left) s2.x = pos; else s2.y = pos;
  src_all[g] = s2;
}

// table[(level, idx)] = value for every node of the update, all levels in one launch
__global__ void __launch_bounds__(256)
tree_insert_kernel(TreeSlot* __restrict__ tab, uint64_t mask, TreeLevels lv, const uint64_t* __restrict__ idx_all,
                   const uint64_t* __restrict__ felts, unsigned total, unsigned long long* __restrict__ fresh) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  bool claimed = false;
  if (g < total) {
    unsigned level = 0;
    while (level < lv.height && g >= lv.idx_off[level + 1]) ++level;  // idx_off is the running node count
    const unsigned j = g - lv.idx_off[level];
    claimed = tree_put(tab, mask, level, idx_all[g], felts + 4 * (size_t)(lv.val_base[level] + (int)j));
  }
  const unsigned long long b = __ballot(claimed);  // one atomic per wave for the entry counter
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(fresh, (unsigned long long)__popcll(b));
}
// out[j] = leaf (level 0) keys[j] or the empty leaf
__global__ void __launch_bounds__(256)
tree_get_kernel(const TreeSlot* __restrict__ tab, uint64_t mask, const uint64_t* __restrict__ keys, unsigned cnt,
                const uint64_t* __restrict__ empty_leaf, uint64_t* __restrict__ out) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  const uint64_t* v = tree_find(tab, mask, 0, keys[j]);
  if (!v) v = empty_leaf;
#pragma unroll
  for (int w = 0; w < 4; ++w) out[4 * (size_t)j + w] = v[w];
}
// ---- witness export: the tree read back by position, nothing hashed ----
// One thread per record = per inner node of the keys' induced subtree.  idx_all is what tree_level_nodes_kernel wrote
// (TreeLevels of the keys, level 0 = the keys): record u is node idx_all[cnt[0] + u], levels 1 .. height one after the
// other, ascending inside a level - the order of the records.  Three probes: the node and its two children, each its
// level's empty-subtree root (emp[level]) when the table has never seen the position.  A child may well be set where
// the other is not and where neither is on a key's path, so neither can be derived from the other records.
__global__ void __launch_bounds__(256)
tree_witness_kernel(TreeLevels lv, const uint64_t* __restrict__ idx_all, const TreeSlot* __restrict__ tab, uint64_t mask,
                    const uint64_t* __restrict__ emp, uint64_t* __restrict__ node, uint64_t* __restrict__ left,
                    uint64_t* __restrict__ right, unsigned n_records) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_records) return;
  const unsigned g = lv.cnt[0] + u;  // position in idx_all; idx_off is the running node count
  unsigned level = 1;
  while (level < lv.height && g >= lv.idx_off[level + 1]) ++level;
  const uint64_t index = idx_all[g];  // < 2^(64 - level): 2 index + 1 cannot wrap
  const uint64_t* v = tree_find(tab, mask, level, index);
  const uint64_t* l = tree_find(tab, mask, level - 1, 2 * index);
  const uint64_t* r = tree_find(tab, mask, level - 1, 2 * index + 1);
  if (!v) v = emp + 4 * level;
  if (!l) l = emp + 4 * (level - 1);
  if (!r) r = emp + 4 * (level - 1);
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    node[4 * (size_t)u + w] = v[w];
    left[4 * (size_t)u + w] = l[w];
    right[4 * (size_t)u + w] = r[w];
  }
}
// One thread per (key, level): siblings[key j][level] = the node beside the path of keys[j] at `level` (0 .. height - 1,
// so the shift is below 64 and the sibling's index at level 63 is 0 or 1); the level-0 thread also writes the leaf.
__global__ void __launch_bounds__(256)
tree_prove_kernel(const TreeSlot* __restrict__ tab, uint64_t mask, const uint64_t* __restrict__ keys, unsigned height,
                  const uint64_t* __restrict__ emp, uint64_t* __restrict__ leaves, uint64_t* __restrict__ siblings,
                  unsigned n_pairs) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_pairs) return;
  const unsigned j = g / height, level = g - j * height;
  const uint64_t key = keys[j];
  const uint64_t* s = tree_find(tab, mask, level, (key >> level) ^ 1ull);
  if (!s) s = emp + 4 * level;
#pragma unroll
  for (int w = 0; w < 4; ++w) siblings[4 * (size_t)g + w] = s[w];
  if (level == 0) {
    const uint64_t* v = tree_find(tab, mask, 0, key);
    if (!v) v = emp;
#pragma unroll
    for (int w = 0; w < 4; ++w) leaves[4 * (size_t)j + w] = v[w];
  }
}
// ---- verifying a multi-update from its witnesses (sp_merkle_verify_update): nothing is looked up, nothing hashed ----
__device__ __forceinline__ bool felt_same(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b) {
  const u256 x = ld_u256(a), y = ld_u256(b);  // two 16-byte loads each
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= x.w[i] ^ y.w[i];
  return d == 0;
}
// One thread per POSITION u of the keys' induced subtree (the order of the records, see tree_witness_kernel); it takes
// the before record (u) and the after record (n_records + u) of its position together.  src_all is what
// tree_children_kernel wrote for the keys: the parents' running count is the record number, so src_all[u] is the
// child list of position u - per side the place of the child among the values of level - 1 (val_base + j: leaf j at
// level 1, else record idx_off[level - 1] - cnt[0] + j), or TREE_PENDING = that child is on no key's path.  Per half:
// `hashed` (one bulk launch sequence over left, right of all 2 R records) against node where the hash has status 0; a
// child on a path against the node of the child record of the SAME half, or against the half's leaf; a child off
// every path against the same child of the OTHER half; the last position's node against the half's root.  No thread
// reads what another writes.  No key is shifted here, so level 64 needs no care beyond tree_level_nodes_kernel's.
// *verdict was preset to SP_PATH_TRUE on the stream: a wave that raised any bit clears the byte with one atomic on the
// aligned word that holds it.
__global__ void __launch_bounds__(256)
witness_check_kernel(TreeLevels lv, const int2* __restrict__ src_all, const uint64_t* __restrict__ node,
                     const uint64_t* __restrict__ left, const uint64_t* __restrict__ right,
                     const uint64_t* __restrict__ hashed, const uint8_t* __restrict__ hash_status,
                     const uint64_t* __restrict__ prev_leaves, const uint64_t* __restrict__ new_leaves,
                     const uint64_t* __restrict__ roots, uint8_t* __restrict__ status, uint8_t* __restrict__ verdict,
                     unsigned n_records) {
  const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned st[2] = {0, 0};
  if (u < n_records) {
    const unsigned g = lv.cnt[0] + u;  // position in idx_all; idx_off is the running node count
    unsigned level = 1;
    while (level < lv.height && g >= lv.idx_off[level + 1]) ++level;
    const int2 s2 = src_all[u];
    const int child_base = lv.val_base[level - 1];
    const size_t child_rec = level > 1 ? lv.idx_off[level - 1] - lv.cnt[0] : 0;  // record number of the level below's first node
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t half = (size_t)h * n_records, rec = half + u;
      const uint64_t* leaves = h ? new_leaves : prev_leaves;
      unsigned s = hash_status[rec];
      if (s == 0 && !felt_same(hashed + 4 * rec, node + 4 * rec)) s = SP_WITNESS_HASH_MISMATCH;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int at = c ? s2.y : s2.x;
        const uint64_t* child = (c ? right : left) + 4 * rec;
        if (at != TREE_PENDING) {
          const size_t j = (size_t)(at - child_base);
          const uint64_t* want = level == 1 ? leaves + 4 * j : node + 4 * (half + child_rec + j);
          if (!felt_same(child, want)) s |= SP_WITNESS_LINK_MISMATCH;
        } else if (h == 0 && !felt_same(child, child + 4 * (size_t)n_records)) {
          st[1] = SP_WITNESS_SIBLING_CHANGED;  // the after record's byte starts from it
          s |= SP_WITNESS_SIBLING_CHANGED;
        }
      }
      if (u == n_records - 1 && !felt_same(node + 4 * rec, roots + 4 * h)) s |= SP_WITNESS_ROOT_MISMATCH;
      st[h] |= s;
      if (status) status[rec] = (uint8_t)st[h];
    }
  }
  unsigned bits = st[0] | st[1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o);
  if ((threadIdx.x & 63) == 0 && bits) {
    const uintptr_t p = (uintptr_t)verdict;
    atomicAnd(reinterpret_cast<unsigned*>(p & ~(uintptr_t)3), ~(0xffu << (8 * (unsigned)(p & 3))));  // SP_PATH_FALSE
  }
}
// ---- the leaf kernels of sp_state_batch: one thread per item, in front of the update's structure kernels ----
// Status bits raised by any lane go into the stream's status flag with one atomic per wave.
__device__ __forceinline__ void tree_raise(unsigned* __restrict__ flag, unsigned bits) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (unsigned)__shfl_xor((int)bits, o);
  if ((threadIdx.x & 63) == 0 && bits) atomicOr(flag, bits);
}
__device__ __forceinline__ bool tree_leaf_is(const TreeSlot* __restrict__ tab, uint64_t mask, uint64_t key,
                                             const uint64_t* __restrict__ empty_leaf, const uint64_t* value) {
  const uint64_t* v = tree_find(tab, mask, 0, key);
  if (!v) v = empty_leaf;
  bool same = true;
#pragma unroll
  for (int w = 0; w < 4; ++w) same &= v[w] == value[w];
  return same;
}
constexpr uint32_t STATE_UNCHANGED = 0xffffffffu;
// Positions (position/hash.cairo:76-131): hashes = the n previous leaves, then the leaves of the changed positions;
// chain_status likewise; map[j] = number of item j among the changed ones, or STATE_UNCHANGED.  Item j: the tree's
// current leaf at keys[j] against its previous hash (only a previous chain that hashed can mismatch), status[j], and
// level-0 slot j of the update = changed ? new hash : previous hash.
__global__ void __launch_bounds__(256)
state_pos_leaf_kernel(const TreeSlot* __restrict__ tab, uint64_t mask, const uint64_t* __restrict__ keys, unsigned cnt,
                      const uint64_t* __restrict__ empty_leaf, const uint64_t* __restrict__ hashes,
                      const uint8_t* __restrict__ chain_status, const uint32_t* __restrict__ map,
                      uint64_t* __restrict__ level0, uint8_t* __restrict__ status, unsigned* __restrict__ flag) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned st = 0;
  if (j < cnt) {
    const uint64_t* leaf = hashes + 4 * (size_t)j;
    st = chain_status[j];
    if (st == 0 && !tree_leaf_is(tab, mask, keys[j], empty_leaf, leaf)) st = SP_STATE_PREV_MISMATCH;
    const uint32_t m = map[j];
    if (m != STATE_UNCHANGED) {
      st |= chain_status[(size_t)cnt + m];
      leaf = hashes + 4 * ((size_t)cnt + m);
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) level0[4 * (size_t)j + w] = leaf[w];
    status[j] = (uint8_t)st;
  }
  tree_raise(flag, st);
}
// Orders: level 0 already holds ord_new (copied with the update's inputs); item j: range check of the new leaf
// against p, the tree's current leaf at keys[j] against prev[j] (a stored leaf is below p, so a prev >= p never
// matches), status[j].
__global__ void __launch_bounds__(256)
state_ord_leaf_kernel(const TreeSlot* __restrict__ tab, uint64_t mask, const uint64_t* __restrict__ keys, unsigned cnt,
                      const uint64_t* __restrict__ empty_leaf, const uint64_t* __restrict__ prev,
                      const uint64_t* __restrict__ level0, uint8_t* __restrict__ status, unsigned* __restrict__ flag) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned st = 0;
  if (j < cnt) {
    if (!u256_lt(ld_u256(level0 + 4 * (size_t)j), U256_P)) st |= SP_HASH_OUT_OF_RANGE;
    if (!tree_leaf_is(tab, mask, keys[j], empty_leaf, prev + 4 * (size_t)j)) st |= SP_STATE_PREV_MISMATCH;
    status[j] = (uint8_t)st;
  }
  tree_raise(flag, st);
}
// rehash every ready slot of `old` into `tab`
__global__ void __launch_bounds__(256)
tree_rehash_kernel(const TreeSlot* __restrict__ old, uint64_t old_slots, TreeSlot* __restrict__ tab, uint64_t mask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_slots) return;
  const TreeSlot& sl = old[i];
  if (sl.state == 2) (void)tree_put(tab, mask, sl.level1 - 1, sl.index, sl.value);
}

// ---- ordered range scan of the non-empty leaves (sp_tree_scan): a descent from the root, no sweep of the table ----
// The frontier of level l is the ascending list of node indices at level l whose key interval meets [lo, hi] and
// whose value differs from the level's empty-subtree root; one step takes it to level l - 1, the frontier of level 0
// is the answer.  What carries the correctness:
//   1. PRUNING COMPARES VALUES (scan_keeps): a leaf that was written and later set back to the empty leaf leaves its
//      whole path in the table, holding empty-subtree roots.  A node that merely exists may have no live leaf below
//      it; a node whose value differs from its level's empty root has at least one.
//   2. so the CUT IS SAFE, with a margin of two: a kept node has a live leaf below it, and that leaf is in range
//      unless the node's interval sticks out of [lo, hi] - which only the node that holds lo (the first of its
//      frontier) and the node that holds hi (the last) can do.  A frontier above level 0 is therefore cut to its
//      first cap + 2 nodes (scan_limit): a frontier that was cut has lost its last node, so at most one node kept
//      is dead, at least cap + 1 have a leaf in range - the first `cap` leaves lie below them, and a cut at ANY level
//      means `more`.  Level 0 holds keys in range only and is cut to cap.  (A cut to cap alone returns an empty page
//      with `more` set for lo = previous key + 1, cap = 1: the node that holds the previous key takes the place.)
//   3. SHIFTS: only children are probed, so a level that is shifted by is at most 63; scan_meets still guards
//      level < 64 the way tree_level_nodes_kernel does, and the root (level 64: "everything") is never tested.
// Work buffer (sp_tree_scan lays it out): header | frontier 0 = the keys | leaves | frontier 1 | mark bytes 0 / 1 |
// cnt[65] | tot[height + 1][blocks]; frontiers and marks have cap + 2 places.  Level l uses frontier, marks of parity l & 1.  A node's MARK byte says which of
// its two children are kept (bit 0 left, bit 1 right): it is written by the thread that emits the node, which probes
// the node's children then and there - every node is probed once, by the launch that places it - and adds their number
// to tot[l][position >> 8] (integer atomics: the sum does not depend on the order).  cnt and tot are cleared once per
// call.  Launches: tree_scan_top_kernel walks the narrow top in ONE workgroup while the frontier fits its 1024
// threads; below that one tree_scan_step_kernel launch per level, grids sized from cap + 2 (which bounds every
// frontier): a block reads the live length on the device and leaves when it has no node.  No level comes back to the
// host.
struct ScanHeader {          // 16 bytes, copied back in front of the keys
  unsigned long long n;      // keys found, at most cap
  unsigned more;             // a frontier was cut: further keys exist in the range
  unsigned start;            // the level at which the top kernel handed over (0: it finished the descent)
};
constexpr unsigned SCAN_TOP = 1024;   // threads of the top kernel = the widest frontier it steps from
constexpr unsigned SCAN_BLOCK = 256;  // threads of a step block = frontier nodes per tot[] entry
struct ScanWork {
  const TreeSlot* tab;
  uint64_t mask;
  const uint64_t* emp;       // empty-subtree roots of levels 0 .. height
  uint64_t lo, hi;
  unsigned cap, blocks;      // blocks = ceil((cap + 2) / SCAN_BLOCK): entries of tot per level
  ScanHeader* hdr;
  uint64_t* frontier[2];
  uint8_t* marks[2];
  unsigned* cnt;             // live frontier length per level (below the hand-over)
  unsigned* tot;             // kept children per SCAN_BLOCK nodes of a level's frontier
  uint64_t* leaves;
};
// property 2: how many nodes the frontier of `level` keeps
__device__ __forceinline__ unsigned scan_limit(const ScanWork& w, unsigned level) { return level ? w.cap + 2 : w.cap; }
__device__ __forceinline__ bool scan_meets(uint64_t index, unsigned level, uint64_t lo, uint64_t hi) {
  const uint64_t first = level < 64 ? index << level : 0;
  const uint64_t last = level < 64 ? first | ((1ull << level) - 1ull) : ~0ull;
  return first <= hi && last >= lo;
}
// A whole slot in three 16-byte loads whose addresses are known before any of them returns: a probe costs ONE trip to
// memory, and the two children of a node are probed side by side.  (tree_find reads state, then level and index, then
// the value, each behind a branch on the one before.  Measured gain over two tree_find calls: 2.29 -> 2.21 ms per
// 4096-key page while the atomics still dominated, 0.43 -> 0.36 ms per 256-key page)
struct ScanSlot {
  uint4 head;  // x, y: index; z: level + 1; w: state
  uint4 v[2];
};
__device__ __forceinline__ ScanSlot scan_load(const TreeSlot* tab, uint64_t i) {
  const uint4* p = reinterpret_cast<const uint4*>(tab + i);  // 48-byte slots of a 256-byte aligned table
  ScanSlot s;
  s.head = p[0];
  s.v[0] = p[1];
  s.v[1] = p[2];
  return s;
}
// property 1: present AND different from the level's empty root (e0, e1); `s` is the slot at the key's home `i`.
// Lookups never run beside insertions (different launches of one stream), so a slot is empty or ready.
// (Loading runs of four consecutive slots per probe was measured and dropped: DESIGN.md 11.)
__device__ __forceinline__ bool scan_keeps(const ScanWork& w, unsigned level, uint64_t index, uint64_t i, ScanSlot s,
                                           uint4 e0, uint4 e1) {
  for (;;) {
    if (s.head.w == 0) return false;
    if (s.head.w == 2 && s.head.z == level + 1 && s.head.x == (uint32_t)index && s.head.y == (uint32_t)(index >> 32)) {
      const uint32_t d = (s.v[0].x ^ e0.x) | (s.v[0].y ^ e0.y) | (s.v[0].z ^ e0.z) | (s.v[0].w ^ e0.w) |
                         (s.v[1].x ^ e1.x) | (s.v[1].y ^ e1.y) | (s.v[1].z ^ e1.z) | (s.v[1].w ^ e1.w);
      return d != 0;
    }
    i = (i + 1) & w.mask;
    s = scan_load(w.tab, i);
  }
}
// which children of node (level, index), level >= 1, are kept: both home slots and the empty root are loaded at once
__device__ __forceinline__ unsigned scan_mark(const ScanWork& w, unsigned level, uint64_t index) {
  const unsigned below = level - 1;
  const uint64_t il = tree_mix(2 * index, below) & w.mask, ir = tree_mix(2 * index + 1, below) & w.mask;
  const ScanSlot sl = scan_load(w.tab, il), sr = scan_load(w.tab, ir);
  const uint4* e = reinterpret_cast<const uint4*>(w.emp + 4 * below);
  const uint4 e0 = e[0], e1 = e[1];
  unsigned mark = 0;
  if (scan_meets(2 * index, below, w.lo, w.hi) && scan_keeps(w, below, 2 * index, il, sl, e0, e1)) mark |= 1u;
  if (scan_meets(2 * index + 1, below, w.lo, w.hi) && scan_keeps(w, below, 2 * index + 1, ir, sr, e0, e1)) mark |= 2u;
  return mark;
}
// key and leaf of position p of the answer (a kept node of level 0 is in the table)
__device__ __forceinline__ void scan_leaf(const ScanWork& w, uint64_t key, unsigned p) {
  uint64_t i = tree_mix(key, 0) & w.mask;
  ScanSlot s = scan_load(w.tab, i);
  while (s.head.w != 0 &&
         !(s.head.w == 2 && s.head.z == 1 && s.head.x == (uint32_t)key && s.head.y == (uint32_t)(key >> 32))) {
    i = (i + 1) & w.mask;
    s = scan_load(w.tab, i);
  }
  uint64_t* out = w.leaves + 4 * (size_t)p;  // 8-byte aligned only: cap + 2 keys lie in front
  if (s.head.w != 0) {
    out[0] = s.v[0].x | (uint64_t)s.v[0].y << 32;
    out[1] = s.v[0].z | (uint64_t)s.v[0].w << 32;
    out[2] = s.v[1].x | (uint64_t)s.v[1].y << 32;
    out[3] = s.v[1].z | (uint64_t)s.v[1].w << 32;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = w.emp[q];
  }
}
__device__ __forceinline__ unsigned scan_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
  return v;
}
__global__ void __launch_bounds__(SCAN_TOP)
tree_scan_top_kernel(ScanWork w, unsigned height) {
  __shared__ unsigned wave_tot[SCAN_TOP / 64];
  // the frontiers of the top live in LDS (2 x 16 KiB), not in the work buffer: no trip to L2 between two levels
  // (measured: 2 % of a 256-key page)
  __shared__ uint64_t fr[2][2 * SCAN_TOP];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned level = height, cnt = 1, more = 0;
  if (threadIdx.x == 0) fr[height & 1][0] = 0;  // the root; the host has compared it with the empty root
  __syncthreads();
  while (level > 0 && cnt <= SCAN_TOP) {
    const uint64_t* cur = fr[level & 1];
    uint64_t* next = fr[(level - 1) & 1];  // total <= 2 cnt <= 2 SCAN_TOP places are written
    const bool live = threadIdx.x < cnt;
    const uint64_t me = live ? cur[threadIdx.x] : 0;
    const unsigned mark = live ? scan_mark(w, level, me) : 0;
    const unsigned long long bl = __ballot(mark & 1), br = __ballot(mark & 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned before = __popcll(bl & below) + __popcll(br & below);
    if (lane == 0) wave_tot[wave] = __popcll(bl) + __popcll(br);
    __syncthreads();
    unsigned p = before, total = 0;
    for (unsigned v = 0; v < SCAN_TOP / 64; ++v) {
      if (v < wave) p += wave_tot[v];
      total += wave_tot[v];
    }
    const unsigned limit = scan_limit(w, level - 1);
    if ((mark & 1) && p < limit) next[p] = 2 * me;
    p += mark & 1;
    if ((mark & 2) && p < limit) next[p] = 2 * me + 1;
    if (total > limit) more = 1;  // property 2: a cut at any level
    cnt = total < limit ? total : limit;
    --level;
    __syncthreads();  // next[] is read by other threads, wave_tot is written again
    if (cnt == 0) level = 0;  // nothing in range: the answer is empty
  }
  if (level == 0) {  // cnt <= min(cap, 2 SCAN_TOP) keys in frontier 0: their leaves
    for (unsigned i = threadIdx.x; i < cnt; i += SCAN_TOP) {
      const uint64_t key = fr[0][i];
      w.frontier[0][i] = key;
      scan_leaf(w, key, i);
    }
  } else {           // hand over at `level`: marks and totals of its frontier, as a step launch would have left them
    const uint64_t* cur = fr[level & 1];
    for (unsigned base = 0; base < cnt; base += SCAN_TOP) {
      const unsigned i = base + threadIdx.x;  // the 64 nodes of a wave lie in one SCAN_BLOCK: one atomic per wave
      const unsigned mark = i < cnt ? scan_mark(w, level, cur[i]) : 0;
      if (i < cnt) {
        w.frontier[level & 1][i] = cur[i];
        w.marks[level & 1][i] = (uint8_t)mark;
      }
      const unsigned kept = scan_wave_sum((unsigned)__popc(mark));
      if (lane == 0 && kept) atomicAdd(&w.tot[(size_t)level * w.blocks + i / SCAN_BLOCK], kept);
    }
  }
  if (threadIdx.x == 0) {
    w.hdr->n = level == 0 ? cnt : 0;
    w.hdr->more = more;
    w.hdr->start = level;
    if (level) w.cnt[level] = cnt;
  }
}
// One step, level -> level - 1, one thread per frontier node.  A block sums the totals in front of it itself (block b
// reads b entries, strided over its threads): no scan launch and no tile of block totals; block 0 also sums all of
// them and leaves the next level's length and the cut.
__global__ void __launch_bounds__(SCAN_BLOCK)
tree_scan_step_kernel(ScanWork w, unsigned level) {
  __shared__ unsigned wave_tot[SCAN_BLOCK / 64];
  __shared__ unsigned wave_sum[2][SCAN_BLOCK / 64];
  if (level > w.hdr->start) return;  // the top kernel has walked this level
  const unsigned cnt = w.cnt[level];
  const unsigned b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (b * SCAN_BLOCK >= cnt) return;  // surplus block (cnt == 0: cnt[level - 1] keeps the 0 it was cleared to)
  const unsigned live_blocks = (cnt + SCAN_BLOCK - 1) / SCAN_BLOCK;
  const unsigned* tot = w.tot + (size_t)level * w.blocks;
  unsigned front = 0, all = 0;
  for (unsigned j = threadIdx.x; j < (b == 0 ? live_blocks : b); j += SCAN_BLOCK) {
    const unsigned t = tot[j];
    if (j < b) front += t;
    all += t;
  }
  front = scan_wave_sum(front);
  all = scan_wave_sum(all);
  const unsigned i = b * SCAN_BLOCK + threadIdx.x;
  const bool live = i < cnt;
  const uint64_t me = live ? w.frontier[level & 1][i] : 0;
  const unsigned mark = live ? w.marks[level & 1][i] : 0;
  const unsigned long long bl = __ballot(mark & 1), br = __ballot(mark & 2);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned p = __popcll(bl & below) + __popcll(br & below);
  if (lane == 0) {
    wave_tot[wave] = __popcll(bl) + __popcll(br);
    wave_sum[0][wave] = front;
    wave_sum[1][wave] = all;
  }
  __syncthreads();
  front = all = 0;
  for (unsigned v = 0; v < SCAN_BLOCK / 64; ++v) {
    if (v < wave) p += wave_tot[v];
    front += wave_sum[0][v];
    all += wave_sum[1][v];
  }
  unsigned wave_first = front;  // position of the wave's first child: its at most 128 children lie in two SCAN_BLOCKs
  for (unsigned v = 0; v < wave; ++v) wave_first += wave_tot[v];
  const unsigned bucket = wave_first / SCAN_BLOCK;
  p += front;
  const unsigned limit = scan_limit(w, level - 1);
  uint64_t* next = w.frontier[(level - 1) & 1];
  unsigned kept_lo = 0, kept_hi = 0;  // kept grandchildren whose parent lies in `bucket` / in the one behind it
#pragma unroll
  for (unsigned side = 0; side < 2; ++side) {
    if (mark & (1u << side)) {
      if (p < limit) {  // the cut (property 2)
        const uint64_t child = 2 * me + side;
        next[p] = child;
        if (level > 1) {
          const unsigned m = scan_mark(w, level - 1, child);
          w.marks[(level - 1) & 1][p] = (uint8_t)m;
          if (p / SCAN_BLOCK == bucket) kept_lo += (unsigned)__popc(m); else kept_hi += (unsigned)__popc(m);
        } else {
          scan_leaf(w, child, p);
        }
      }
      ++p;
    }
  }
  // one atomic per wave and bucket: with one add per child, the 4096 adds of a level went into the ONE cache line
  // that holds its totals and a 4096-key page took 2.21 ms instead of 0.79
  kept_lo = scan_wave_sum(kept_lo);
  kept_hi = scan_wave_sum(kept_hi);
  if (lane == 0 && level > 1) {
    unsigned* into = w.tot + (size_t)(level - 1) * w.blocks + bucket;
    if (kept_lo) atomicAdd(into, kept_lo);
    if (kept_hi) atomicAdd(into + 1, kept_hi);
  }
  if (b == 0 && threadIdx.x == 0) {
    const unsigned kept = all < limit ? all : limit;
    if (all > limit) w.hdr->more = 1;
    if (level > 1) w.cnt[level - 1] = kept; else w.hdr->n = kept;
  }
}

// ---- ordered list of the keys whose leaves differ between two trees (sp_tree_diff): the scan's descent from TWO roots ----
// The frontier of level l is the ascending list of node indices at level l whose key interval meets [lo, hi] and whose
// value in table A differs from its value in table B; a position absent from a table reads as the empty-subtree root of
// its level (both trees have one empty leaf, so one array of empty roots serves both).  The three properties of the
// scan carry over:
//   1. PRUNING COMPARES VALUES (diff_mark): both tables are consistent hash trees, so equal leaves below a node give
//      equal nodes - a kept node has a differing leaf below it - and equal nodes mean equal subtrees, up to a hash
//      collision - a pruned node has none.  A path that A holds with empty-root values (a leaf written and set back)
//      equals B's missing entry and is pruned.
//   2. THE CUT (diff_limit): the differing leaf below a kept node is in range unless the node's interval sticks out of
//      [lo, hi], which only the first and the last node of a frontier can do; frontiers above level 0 keep cap + 2
//      nodes, level 0 keeps cap, a cut at any level means `more` - the scan's argument word for word.
//   3. SHIFTS: only children are probed (levels <= 63), scan_meets guards level < 64, the root is never tested.
// The scan kernels above stay as they are: the diff has kernels of its own with the scan's launch shape, work-buffer
// layout (one more run of leaves) and position arithmetic, and shares the __device__ helpers (scan_meets, scan_load,
// scan_wave_sum, tree_mix, ScanHeader, SCAN_TOP, SCAN_BLOCK).  What differs is the probe: FOUR home slots per emitted
// node - two children in two tables whose masks differ - twelve 16-byte loads issued before the first use, and linear
// probing that continues in each table on its own.  A tree that was never updated has no table: its probes go to
// `none`, one zeroed slot of the work buffer (mask 0), so "absent" is what every probe of it answers and no load of
// the other table waits behind a branch.
struct DiffWork {
  const TreeSlot* tab[2];    // A, B; nullptr: no table, every probe answers the level's empty root
  uint64_t mask[2];          // 0 beside a null table
  const TreeSlot* none;      // one slot of zeros
  const uint64_t* emp;       // empty-subtree roots of levels 0 .. height
  uint64_t lo, hi;
  unsigned cap, blocks;      // blocks = ceil((cap + 2) / SCAN_BLOCK): entries of tot per level
  ScanHeader* hdr;
  uint64_t* frontier[2];
  uint8_t* marks[2];
  unsigned* cnt;
  unsigned* tot;
  uint64_t* leaves[2];       // of A, of B
};
// property 2: how many nodes the frontier of `level` keeps
__device__ __forceinline__ unsigned diff_limit(const DiffWork& w, unsigned level) { return level ? w.cap + 2 : w.cap; }
struct DiffValue {
  uint4 v[2];
};
__device__ __forceinline__ const TreeSlot* diff_table(const DiffWork& w, unsigned t) { return w.tab[t] ? w.tab[t] : w.none; }
// value of (level, index) in table t; `s` is the slot at the key's home `i`; absent: the level's empty root (e0, e1)
__device__ __forceinline__ DiffValue diff_value(const TreeSlot* tab, uint64_t mask, unsigned level, uint64_t index,
                                                uint64_t i, ScanSlot s, uint4 e0, uint4 e1) {
  DiffValue out;
  for (;;) {
    if (s.head.w == 0) {
      out.v[0] = e0;
      out.v[1] = e1;
      return out;
    }
    if (s.head.w == 2 && s.head.z == level + 1 && s.head.x == (uint32_t)index && s.head.y == (uint32_t)(index >> 32)) {
      out.v[0] = s.v[0];
      out.v[1] = s.v[1];
      return out;
    }
    i = (i + 1) & mask;
    s = scan_load(tab, i);
  }
}
__device__ __forceinline__ bool diff_differs(const DiffValue& a, const DiffValue& b) {
  const uint32_t d = (a.v[0].x ^ b.v[0].x) | (a.v[0].y ^ b.v[0].y) | (a.v[0].z ^ b.v[0].z) | (a.v[0].w ^ b.v[0].w) |
                     (a.v[1].x ^ b.v[1].x) | (a.v[1].y ^ b.v[1].y) | (a.v[1].z ^ b.v[1].z) | (a.v[1].w ^ b.v[1].w);
  return d != 0;
}
// Every word of the slots just loaded is an input of ONE empty statement: all their loads are issued before the first
// use, one trip to memory for the whole probe.  Without it the compiler sinks the loads of one child behind the branch
// on scan_meets and folds the home-slot load of another into its probing loop (seen in the device assembly: nine of
// the twelve loads of diff_mark in flight at the first wait, in two groups).
typedef uint32_t diff_w4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ diff_w4 diff_words(uint4 u) { return diff_w4{u.x, u.y, u.z, u.w}; }
__device__ __forceinline__ void diff_hold(const ScanSlot& a, const ScanSlot& b) {
  asm volatile("" ::"v"(diff_words(a.head)), "v"(diff_words(a.v[0])), "v"(diff_words(a.v[1])), "v"(diff_words(b.head)),
               "v"(diff_words(b.v[0])), "v"(diff_words(b.v[1])));
}
__device__ __forceinline__ void diff_hold(const ScanSlot& a, const ScanSlot& b, const ScanSlot& c, const ScanSlot& d) {
  asm volatile("" ::"v"(diff_words(a.head)), "v"(diff_words(a.v[0])), "v"(diff_words(a.v[1])), "v"(diff_words(b.head)),
               "v"(diff_words(b.v[0])), "v"(diff_words(b.v[1])), "v"(diff_words(c.head)), "v"(diff_words(c.v[0])),
               "v"(diff_words(c.v[1])), "v"(diff_words(d.head)), "v"(diff_words(d.v[0])), "v"(diff_words(d.v[1])));
}
// which children of node (level, index), level >= 1, are kept (property 1): the four home slots - left and right child
// in A and in B - and the empty root are loaded at once, then each table is probed on along its own chain
__device__ __forceinline__ unsigned diff_mark(const DiffWork& w, unsigned level, uint64_t index) {
  const unsigned below = level - 1;
  const TreeSlot* ta = diff_table(w, 0);
  const TreeSlot* tb = diff_table(w, 1);
  const uint64_t hl = tree_mix(2 * index, below), hr = tree_mix(2 * index + 1, below);
  const uint64_t al = hl & w.mask[0], ar = hr & w.mask[0], bl = hl & w.mask[1], br = hr & w.mask[1];
  const ScanSlot sal = scan_load(ta, al), sar = scan_load(ta, ar), sbl = scan_load(tb, bl), sbr = scan_load(tb, br);
  const uint4* e = reinterpret_cast<const uint4*>(w.emp + 4 * below);
  const uint4 e0 = e[0], e1 = e[1];
  diff_hold(sal, sar, sbl, sbr);
  unsigned mark = 0;
  if (scan_meets(2 * index, below, w.lo, w.hi) &&
      diff_differs(diff_value(ta, w.mask[0], below, 2 * index, al, sal, e0, e1),
                   diff_value(tb, w.mask[1], below, 2 * index, bl, sbl, e0, e1)))
    mark |= 1u;
  if (scan_meets(2 * index + 1, below, w.lo, w.hi) &&
      diff_differs(diff_value(ta, w.mask[0], below, 2 * index + 1, ar, sar, e0, e1),
                   diff_value(tb, w.mask[1], below, 2 * index + 1, br, sbr, e0, e1)))
    mark |= 2u;
  return mark;
}
// key and both leaves of position p of the answer
__device__ __forceinline__ void diff_leaf(const DiffWork& w, uint64_t key, unsigned p) {
  const TreeSlot* ta = diff_table(w, 0);
  const TreeSlot* tb = diff_table(w, 1);
  const uint64_t h = tree_mix(key, 0);
  const uint64_t ia = h & w.mask[0], ib = h & w.mask[1];
  const ScanSlot sa = scan_load(ta, ia), sb = scan_load(tb, ib);
  const uint4* e = reinterpret_cast<const uint4*>(w.emp);
  const uint4 e0 = e[0], e1 = e[1];
  diff_hold(sa, sb);
  const DiffValue v[2] = {diff_value(ta, w.mask[0], 0, key, ia, sa, e0, e1), diff_value(tb, w.mask[1], 0, key, ib, sb, e0, e1)};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    uint64_t* out = w.leaves[t] + 4 * (size_t)p;  // 8-byte aligned only: cap + 2 keys lie in front
    out[0] = v[t].v[0].x | (uint64_t)v[t].v[0].y << 32;
    out[1] = v[t].v[0].z | (uint64_t)v[t].v[0].w << 32;
    out[2] = v[t].v[1].x | (uint64_t)v[t].v[1].y << 32;
    out[3] = v[t].v[1].z | (uint64_t)v[t].v[1].w << 32;
  }
}
// The narrow top in one workgroup, frontiers in LDS: tree_scan_top_kernel with diff_mark / diff_leaf.
__global__ void __launch_bounds__(SCAN_TOP)
tree_diff_top_kernel(DiffWork w, unsigned height) {
  __shared__ unsigned wave_tot[SCAN_TOP / 64];
  __shared__ uint64_t fr[2][2 * SCAN_TOP];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned level = height, cnt = 1, more = 0;
  if (threadIdx.x == 0) fr[height & 1][0] = 0;  // the root; the host has compared the two roots (property 3)
  __syncthreads();
  while (level > 0 && cnt <= SCAN_TOP) {
    const uint64_t* cur = fr[level & 1];
    uint64_t* next = fr[(level - 1) & 1];  // total <= 2 cnt <= 2 SCAN_TOP places are written
    const bool live = threadIdx.x < cnt;
    const uint64_t me = live ? cur[threadIdx.x] : 0;
    const unsigned mark = live ? diff_mark(w, level, me) : 0;
    const unsigned long long bl = __ballot(mark & 1), br = __ballot(mark & 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned before = __popcll(bl & below) + __popcll(br & below);
    if (lane == 0) wave_tot[wave] = __popcll(bl) + __popcll(br);
    __syncthreads();
    unsigned p = before, total = 0;
    for (unsigned v = 0; v < SCAN_TOP / 64; ++v) {
      if (v < wave) p += wave_tot[v];
      total += wave_tot[v];
    }
    const unsigned limit = diff_limit(w, level - 1);
    if ((mark & 1) && p < limit) next[p] = 2 * me;
    p += mark & 1;
    if ((mark & 2) && p < limit) next[p] = 2 * me + 1;
    if (total > limit) more = 1;  // property 2: a cut at any level
    cnt = total < limit ? total : limit;
    --level;
    __syncthreads();  // next[] is read by other threads, wave_tot is written again
    if (cnt == 0) level = 0;  // nothing differs in range: the answer is empty
  }
  if (level == 0) {  // cnt <= min(cap, 2 SCAN_TOP) keys in frontier 0: their leaves
    for (unsigned i = threadIdx.x; i < cnt; i += SCAN_TOP) {
      const uint64_t key = fr[0][i];
      w.frontier[0][i] = key;
      diff_leaf(w, key, i);
    }
  } else {           // hand over at `level`: marks and totals of its frontier, as a step launch would have left them
    const uint64_t* cur = fr[level & 1];
    for (unsigned base = 0; base < cnt; base += SCAN_TOP) {
      const unsigned i = base + threadIdx.x;  // the 64 nodes of a wave lie in one SCAN_BLOCK: one atomic per wave
      const unsigned mark = i < cnt ? diff_mark(w, level, cur[i]) : 0;
      if (i < cnt) {
        w.frontier[level & 1][i] = cur[i];
        w.marks[level & 1][i] = (uint8_t)mark;
      }
      const unsigned kept = scan_wave_sum((unsigned)__popc(mark));
      if (lane == 0 && kept) atomicAdd(&w.tot[(size_t)level * w.blocks + i / SCAN_BLOCK], kept);
    }
  }
  if (threadIdx.x == 0) {
    w.hdr->n = level == 0 ? cnt : 0;
    w.hdr->more = more;
    w.hdr->start = level;
    if (level) w.cnt[level] = cnt;
  }
}
// One step, level -> level - 1, one thread per frontier node: tree_scan_step_kernel with diff_mark / diff_leaf (256
// nodes per block, a mark byte per node, one atomic per wave and block for the block totals, each block sums the
// totals in front of it).
__global__ void __launch_bounds__(SCAN_BLOCK)
tree_diff_step_kernel(DiffWork w, unsigned level) {
  __shared__ unsigned wave_tot[SCAN_BLOCK / 64];
  __shared__ unsigned wave_sum[2][SCAN_BLOCK / 64];
  if (level > w.hdr->start) return;  // the top kernel has walked this level
  const unsigned cnt = w.cnt[level];
  const unsigned b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (b * SCAN_BLOCK >= cnt) return;  // surplus block (cnt == 0: cnt[level - 1] keeps the 0 it was cleared to)
  const unsigned live_blocks = (cnt + SCAN_BLOCK - 1) / SCAN_BLOCK;
  const unsigned* tot = w.tot + (size_t)level * w.blocks;
  unsigned front = 0, all = 0;
  for (unsigned j = threadIdx.x; j < (b == 0 ? live_blocks : b); j += SCAN_BLOCK) {
    const unsigned t = tot[j];
    if (j < b) front += t;
    all += t;
  }
  front = scan_wave_sum(front);
  all = scan_wave_sum(all);
  const unsigned i = b * SCAN_BLOCK + threadIdx.x;
  const bool live = i < cnt;
  const uint64_t me = live ? w.frontier[level & 1][i] : 0;
  const unsigned mark = live ? w.marks[level & 1][i] : 0;
  const unsigned long long bl = __ballot(mark & 1), br = __ballot(mark & 2);
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned p = __popcll(bl & below) + __popcll(br & below);
  if (lane == 0) {
    wave_tot[wave] = __popcll(bl) + __popcll(br);
    wave_sum[0][wave] = front;
    wave_sum[1][wave] = all;
  }
  __syncthreads();
  front = all = 0;
  for (unsigned v = 0; v < SCAN_BLOCK / 64; ++v) {
    if (v < wave) p += wave_tot[v];
    front += wave_sum[0][v];
    all += wave_sum[1][v];
  }
  unsigned wave_first = front;  // position of the wave's first child: its at most 128 children lie in two SCAN_BLOCKs
  for (unsigned v = 0; v < wave; ++v) wave_first += wave_tot[v];
  const unsigned bucket = wave_first / SCAN_BLOCK;
  p += front;
  const unsigned limit = diff_limit(w, level - 1);
  uint64_t* next = w.frontier[(level - 1) & 1];
  unsigned kept_lo = 0, kept_hi = 0;  // kept grandchildren whose parent lies in `bucket` / in the one behind it
#pragma unroll
  for (unsigned side = 0; side < 2; ++side) {
    if (mark & (1u << side)) {
      if (p < limit) {  // the cut (property 2)
        const uint64_t child = 2 * me + side;
        next[p] = child;
        if (level > 1) {
          const unsigned m = diff_mark(w, level - 1, child);
          w.marks[(level - 1) & 1][p] = (uint8_t)m;
          if (p / SCAN_BLOCK == bucket) kept_lo += (unsigned)__popc(m); else kept_hi += (unsigned)__popc(m);
        } else {
          diff_leaf(w, child, p);
        }
      }
      ++p;
    }
  }
  kept_lo = scan_wave_sum(kept_lo);
  kept_hi = scan_wave_sum(kept_hi);
  if (lane == 0 && level > 1) {  // one atomic per wave and bucket
    unsigned* into = w.tot + (size_t)(level - 1) * w.blocks + bucket;
    if (kept_lo) atomicAdd(into, kept_lo);
    if (kept_hi) atomicAdd(into + 1, kept_hi);
  }
  if (b == 0 && threadIdx.x == 0) {
    const unsigned kept = all < limit ? all : limit;
    if (all > limit) w.hdr->more = 1;
    if (level > 1) w.cnt[level - 1] = kept; else w.hdr->n = kept;
  }
}

struct SparseTree {
  unsigned height = 0;
  uint64_t empty_leaf[4] = {0, 0, 0, 0};
  int ctx_index = 0;           // the context (device) the tree lives on
  RetiringBuffer<TreeSlot> table;  // HBM; the table before the last growth (tree_reserve) stays until the next one
  uint64_t slots = 0;          // power of two
  uint64_t entries = 0;        // used slots as of the last read of d_entries
  unsigned long long* d_entries = nullptr;  // device counter of claimed slots (insert kernels add to it)
  bool has_root = false;
  uint64_t root[4] = {0, 0, 0, 0};
  // Every tree has its OWN stream and work buffer and its own mutex: an operation holds the tree's mutex from
  // start to end (updates of one tree are ordered anyway) and takes the library lock only to enqueue - the
  // copies and the ~3 ms of level launches of a height-64 update run without it, so hash / verify batches and
  // updates of OTHER trees proceed meanwhile (round 2: null stream, library lock across everything).
  hipStream_t stream = nullptr;
  DeviceBuffer buf;
  PinnedBuffer hbuf;  // host-side staging of an update's inputs (empty roots, leaves, keys): see PinnedBuffer
  // The constant points of the levels (pedersen.hip SPARSE quad kernel): for level l the sum of the table entries
  // that the level's empty-subtree root selects as a left / right operand, [2 l] and [2 l + 1]; computed on the
  // tree's stream by its first update, kept for its lifetime (the window plan cannot change under a live tree).
  DeviceBuffer cpts;
  int cpts_state = 0;  // 0: not computed, 1: ready, -1: the plan has no constant window on one side
  std::mutex mu;
  bool destroyed = false;  // set by sp_tree_destroy under `mu`: a thread that was waiting for the mutex with the
                           // old handle must not revive the freed tree
};

static std::map<int, std::shared_ptr<SparseTree>> g_trees;
static int g_next_tree = 1;

static void tree_free(SparseTree& t) {
  if (t.stream) {
    (void)hipStreamSynchronize(t.stream);
    (void)hipStreamDestroy(t.stream);
  }
  t.table.release();
  if (t.d_entries) (void)hipFree(t.d_entries);
  t.buf.release();
  t.hbuf.release();
  t.cpts.release();
  t.cpts_state = 0;
  t.stream = nullptr;
  t.d_entries = nullptr;
  t.slots = 0;
}

// Looks the handle up, selects the tree's context and device for this host thread and locks the tree.
struct TreeScope {
  std::shared_ptr<SparseTree> t;
  int previous_ctx = -1;
  int previous_dev = -1;
  bool switched_dev = false;
  std::unique_lock<std::mutex> held;
  int open(int handle) {
    {
      ctx_lock lk(global_mu());
      auto it = g_trees.find(handle);
      if (it == g_trees.end()) { set_error("unknown tree handle"); return SP_ERR_BAD_ARGUMENT; }
      t = it->second;
    }
    held = std::unique_lock<std::mutex>(t->mu);
    if (t->destroyed) { set_error("unknown tree handle"); return SP_ERR_BAD_ARGUMENT; }
    previous_ctx = ctx_current();
    ctx_select(t->ctx_index);
    const int dev = ctx().device;
    if (hipGetDevice(&previous_dev) == hipSuccess && previous_dev != dev) switched_dev = hipSetDevice(dev) == hipSuccess;
    if (!t->stream) SP_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    return SP_OK;
  }
  ~TreeScope() {
    if (previous_ctx >= 0) ctx_select(previous_ctx);
    if (switched_dev) (void)hipSetDevice(previous_dev);
  }
};

// Room for `extra` more entries at a load factor of at most 1/2 (tree mutex held).
// Growth policy (round 6): a table that has to grow is sized for FOUR times what is asked of it
// (load factor 1/4 straight after a growth), so that the next updates of the same size fit without another one, and
// the growth itself costs the caller no wait: clear and rehash are enqueued on the tree's stream and the old table is
// retired, not freed (RetiringBuffer of context.hpp: with a hipFree, calls 1 - 2 of a fresh tree cost 2.9 - 3.1 ms
// against 1.97 ms in round 5).  By the next growth its rehash has long finished: the intervening update synchronised
// the stream.  First allocation: 2^16 slots, or STARKPERP_TREE_INITIAL_SLOTS_LOG2.
static uint64_t tree_initial_slots() {
  static const uint64_t v = [] {
    const char* e = getenv("STARKPERP_TREE_INITIAL_SLOTS_LOG2");
    const int lg = e ? atoi(e) : 16;
    return (uint64_t)1 << (lg < 10 ? 10 : (lg > 30 ? 30 : lg));
  }();
  return v;
}
static int tree_reserve(SparseTree& t, uint64_t extra) {
  if (!t.d_entries) {
    SP_HIP(hipMalloc(&t.d_entries, sizeof(unsigned long long)));
    SP_HIP(hipMemsetAsync(t.d_entries, 0, sizeof(unsigned long long), t.stream));
  }
  if (t.slots && 2 * (t.entries + extra) > t.slots) {  // would not fit by the last known count: refresh it
    unsigned long long used = 0;
    SP_HIP(hipMemcpyAsync(&used, t.d_entries, sizeof(used), hipMemcpyDeviceToHost, t.stream));
    SP_HIP(hipStreamSynchronize(t.stream));
    t.entries = used;
  }
  if (t.slots && 2 * (t.entries + extra) <= t.slots) return SP_OK;
  uint64_t want = t.slots ? t.slots : tree_initial_slots();
  while (4 * (t.entries + extra) > want) want <<= 1;
  if (want == t.slots) return SP_OK;
  TreeSlot* old = nullptr;
  SP_HIP(t.table.grow(want * sizeof(TreeSlot), t.stream, &old));
  tl_mark("tree: table allocated");
  SP_HIP(hipMemsetAsync(t.table.ptr, 0, want * sizeof(TreeSlot), t.stream));
  if (old) {
    hipLaunchKernelGGL(tree_rehash_kernel, dim3((unsigned)((t.slots + 255) / 256)), dim3(256), 0, t.stream, old, t.slots,
                       t.table.ptr, want - 1);
    SP_HIP(hipGetLastError());
  }
  t.slots = want;
  return SP_OK;
}

// The empty-subtree roots of the tree's levels, a copy (tree mutex held; the cache and the scratch map are shared).
static int tree_empty_roots(const SparseTree& t, std::vector<uint64_t>& out) {
  ctx_lock lk(global_mu());
  Scratch s;
  int rc = get_scratch_public(1, s, t.stream);
  if (rc != SP_OK) return rc;
  const std::vector<uint64_t>* emp = nullptr;
  rc = empty_roots(t.empty_leaf, s, t.stream, &emp);
  if (rc != SP_OK) return rc;
  out.assign(emp->begin(), emp->begin() + 4 * ((size_t)t.height + 1));
  return SP_OK;
}

static int tree_root_locked(SparseTree& t, uint64_t* root) {
  if (t.has_root) {
    std::memcpy(root, t.root, 32);
    return SP_OK;
  }
  std::vector<uint64_t> emp;
  const int rc = tree_empty_roots(t, emp);
  if (rc != SP_OK) return rc;
  std::memcpy(root, &emp[4 * (size_t)t.height], 32);
  return SP_OK;
}

// ---- the update itself, in two phases (tree mutex held, context selected) ----
//   tree_enqueue   everything up to "levels enqueued" on the tree's stream, and the asynchronous copy-back of the
//                  status flag and the candidate root;
//   tree_wait      the ONE wait of an update; hands back the flag;
//   tree_commit    launches tree_insert_kernel and adopts the candidate root.
// sp_tree_update and sp_order_batch run them back to back (tree_update_locked); sp_state_batch enqueues two trees,
// waits for both, decides once and commits both or neither.
//
// Level 0 is filled in one of two ways: the host's `leaves` are copied into the work buffer, or a PRODUCER already
// enqueued on the tree's stream writes the level-0 values there (sp_state_batch: no hash crosses PCIe).  A producer
// owns `dev_bytes` of the work buffer behind the update's own arrays and `host_bytes` of the tree's page-locked
// staging buffer behind the update's inputs (host == nullptr: the batch is above PINNED_STAGE_MAX, copy directly).
struct LeafProducer {
  size_t dev_bytes = 0, host_bytes = 0;
  // uploads, and hashing that uses the stream's scratch in a layout of its own: runs first, under the library lock
  std::function<int(char* dev, char* host, hipStream_t st)> stage;
  // the leaf kernel and the copy-back of its status bytes: behind tree_reserve's memset / rehash, the copies of keys
  // and empty roots (d_empty: the empty leaf) and the clearing of `flag`, all on the same stream
  std::function<int(char* dev, char* host, const TreeSlot* tab, uint64_t mask, const uint64_t* d_keys,
                    const uint64_t* d_empty, uint64_t* d_level0, unsigned* flag, hipStream_t st)> place;
};
struct TreePending {  // what tree_enqueue leaves for tree_wait / tree_commit
  bool queued = false;  // false: an empty update, nothing is on the stream
  TreeLevels lv;
  size_t total = 0;
  uint64_t* d_felts = nullptr;
  uint64_t* d_idx = nullptr;
  const unsigned* h_flag = nullptr;   // where flag and candidate root land: the tree's page-locked buffer, or ...
  const uint64_t* h_root = nullptr;
  unsigned flag_host = 0;             // ... these, for an update too large for it
  uint64_t root_host[4] = {0, 0, 0, 0};
};

// ---- host: only the node COUNT of every level (merkle_tree.py:18-26 on the keys alone): level l has one node
// per distinct key >> l, i.e. 1 + the adjacent key pairs whose highest differing bit is >= l.  keys sorted, n >= 1;
// cnt[0 .. height].  Shared by an update (tree_enqueue) and a witness (sp_tree_witness_size, sp_tree_witness). ----
static void tree_level_counts(unsigned height, const uint64_t* keys, size_t n, std::vector<size_t>& cnt) {
  cnt.assign(height + 1, 0);
  size_t hist[65] = {0};
  for (size_t i = 1; i < n; ++i) ++hist[63 - __builtin_clzll(keys[i] ^ keys[i - 1])];
  size_t above = 0;
  for (int l = 64; l >= 0; --l) {
    if (l < 64) above += hist[l];
    if ((unsigned)l <= height) cnt[l] = 1 + above;
  }
}
// The TreeLevels of the keys' induced subtree and the sizes of its arrays: `total` nodes over all levels, `felts`
// values, `idxs` node indices, `srcs` child lists.  false: too large for the 32-bit positions of the kernels.
static bool tree_layout(unsigned height, const uint64_t* keys, size_t n, std::vector<size_t>& cnt, TreeLevels& lv,
                        size_t& total, size_t& felts, size_t& idxs, size_t& srcs) {
  tree_level_counts(height, keys, n, cnt);
  total = 0;
  for (unsigned l = 0; l <= height; ++l) total += cnt[l];
  // felts: [level 0 values][siblings for level 1's parents][level 1 values][siblings ...] ...
  std::memset(&lv, 0, sizeof(lv));
  lv.height = height;
  felts = idxs = srcs = 0;
  for (unsigned l = 0; l <= height; ++l) {
    lv.cnt[l] = (unsigned)cnt[l];
    lv.val_base[l] = (int)felts;
    felts += cnt[l];
    lv.idx_off[l] = (unsigned)idxs;
    idxs += cnt[l];
    if (l < height) {
      lv.sib_base[l] = (int)felts;
      felts += cnt[l + 1];
      lv.src_off[l] = (unsigned)srcs;
      srcs += cnt[l + 1];
    }
  }
  return felts < (size_t)INT_MAX && total <= 0x7fffffffull;
}

// `enqueued`, when given, is called once the levels are on the stream and the library lock is free again.
static int tree_enqueue(SparseTree& t, const uint64_t* keys, const uint64_t* leaves, size_t n, uint64_t* old_root,
                        uint8_t* status, const LeafProducer* producer, TreePending& p,
                        const std::function<void()>* enqueued = nullptr) {
  const unsigned height = t.height;
  if (!keys_ok(height, keys, n, true)) return SP_ERR_BAD_ARGUMENT;
  int rc = tree_root_locked(t, old_root);
  if (rc != SP_OK) return rc;
  if (status) *status = 0;
  p.queued = false;
  if (n == 0) return SP_OK;
  std::vector<size_t> cnt;
  TreeLevels& lv = p.lv;
  size_t total = 0, felts = 0, idxs = 0, srcs = 0;
  if (!tree_layout(height, keys, n, cnt, lv, total, felts, idxs, srcs)) { set_error("update too large"); return SP_ERR_BAD_ARGUMENT; }
  tl_mark("tree: level counts");
  rc = tree_reserve(t, total);
  if (rc != SP_OK) return rc;
  tl_mark("tree: table reserved");
  const size_t emp_bytes = ((size_t)height + 1) * 32;
  const size_t felt_bytes = felts * 32, idx_bytes = idxs * 8, src_bytes = srcs * sizeof(int2);
  const size_t own_bytes = emp_bytes + felt_bytes + idx_bytes + src_bytes;
  const size_t prod_off = (own_bytes + 255) & ~(size_t)255;  // the producer's part of the work buffer
  SP_HIP(t.buf.reserve(producer ? prod_off + producer->dev_bytes + 1024 : own_bytes + 1024));
  char* b = (char*)t.buf.ptr;
  uint64_t* d_emp = (uint64_t*)b;
  uint64_t* d_felts = (uint64_t*)(b + emp_bytes);
  uint64_t* d_idx = (uint64_t*)(b + emp_bytes + felt_bytes);
  int2* d_src = (int2*)(b + emp_bytes + felt_bytes + idx_bytes);
  hipStream_t st = t.stream;
  Scratch s;
  unsigned* h_flag = &p.flag_host;
  uint64_t* h_root = p.root_host;
  {
    // ---- enqueue under the library lock: scratch map, empty-root cache, launch bookkeeping ----
    tl_mark("tree: work buffer ready");
    ctx_lock lk(global_mu());
    tl_mark("tree: library lock taken");
    // Small updates go through the tree's page-locked buffer (PinnedBuffer): inputs | landing of flag and
    // candidate root | the producer's part.
    const size_t leaf_bytes = leaves ? n * 32 : 0;
    const size_t land_off = (emp_bytes + leaf_bytes + n * 8 + 31) & ~(size_t)31;
    const size_t in_bytes = land_off + 64 + (producer ? producer->host_bytes : 0);
    char* const stage = StagedTrip(t.hbuf, in_bytes, st).stage;  // the decision only: the copies below are its own
    if (stage) {
      h_flag = (unsigned*)(stage + land_off);
      h_root = (uint64_t*)(stage + land_off + 32);
    }
    char* prod_host = stage ? stage + land_off + 64 : nullptr;
    if (producer && producer->stage) {
      rc = producer->stage(b + prod_off, prod_host, st);
      if (rc != SP_OK) return rc;
      tl_mark("tree: producer staged");
    }
    rc = get_scratch_public(n, s, st);
    if (rc != SP_OK) return rc;
    tl_mark("tree: scratch");
    SP_HIP(hipMemsetAsync(s.flag, 0, sizeof(unsigned), st));
    tl_mark("tree: flag cleared");
    const std::vector<uint64_t>* emp = nullptr;
    rc = empty_roots(t.empty_leaf, s, st, &emp);
    if (rc != SP_OK) return rc;
    tl_mark("tree: empty roots");
    // empty roots + leaves are adjacent in the work buffer (d_emp, then the level-0 values at the start of d_felts):
    // one copy; the keys a second one.
    if (stage) {
      // the previous update's copies out of this buffer are long finished: every update ends with a wait on `st`
      std::memcpy(stage, emp->data(), emp_bytes);
      if (leaves) std::memcpy(stage + emp_bytes, leaves, n * 32);
      std::memcpy(stage + emp_bytes + leaf_bytes, keys, n * 8);
      SP_HIP(hipMemcpyAsync(d_emp, stage, emp_bytes + leaf_bytes, hipMemcpyHostToDevice, st));
      SP_HIP(hipMemcpyAsync(d_idx, stage + emp_bytes + leaf_bytes, n * 8, hipMemcpyHostToDevice, st));
    } else {
      SP_HIP(hipMemcpyAsync(d_emp, emp->data(), emp_bytes, hipMemcpyHostToDevice, st));
      if (leaves) SP_HIP(hipMemcpyAsync(d_felts, leaves, n * 32, hipMemcpyHostToDevice, st));
      SP_HIP(hipMemcpyAsync(d_idx, keys, n * 8, hipMemcpyHostToDevice, st));
    }
    tl_mark("tree: inputs copied");
    if (producer && producer->place) {  // level 0 comes from (or is checked by) a kernel on this stream
      rc = producer->place(b + prod_off, prod_host, t.table.ptr, t.slots - 1, d_idx, d_emp, d_felts, s.flag, st);
      if (rc != SP_OK) return rc;
      tl_mark("tree: leaf kernel enqueued");
    }
    // the structure of every level and the sibling lookups, then the hashes level by level
    hipLaunchKernelGGL(tree_level_nodes_kernel, dim3(height), dim3(1024), 0, st, lv, d_idx, d_idx);
    hipLaunchKernelGGL(tree_children_kernel, dim3((unsigned)((total - cnt[height] + 255) / 256)), dim3(256), 0, st, lv,
                       d_idx, d_src, (unsigned)(total - cnt[height]));
    hipLaunchKernelGGL(tree_lookup_kernel, dim3((unsigned)((srcs + 255) / 256)), dim3(256), 0, st, lv, d_idx, t.table.ptr,
                       t.slots - 1, d_felts, d_src, (unsigned)srcs);
    SP_HIP(hipGetLastError());
    tl_mark("tree: structure kernels enqueued");
    if (t.cpts_state == 0) {  // once per tree: the constant points of its 64 levels (d_emp is on the stream already)
      SP_HIP(t.cpts.reserve(2 * (size_t)height * sizeof(aff_packed)));
      bool usable = false;
      rc = enqueue_partial_points(d_emp, (int)height, (aff_packed*)t.cpts.ptr, st, &usable);
      if (rc != SP_OK) return rc;
      t.cpts_state = usable ? 1 : -1;
    }
    const aff_packed* cpts = t.cpts_state == 1 ? (const aff_packed*)t.cpts.ptr : nullptr;
    for (unsigned l = 0; l < height;) {
      // a run of levels whose paths do not merge (as many parents as children: every node has ONE touched child)
      // goes out as one launch where the size class allows it (ped_path_kernel)
      unsigned l2 = l;
      while (l2 < height && cnt[l2 + 1] == cnt[l]) ++l2;
      if (l2 - l >= 2) {
        PathLevels pl;
        std::memset(&pl, 0, sizeof(pl));
        pl.first = (int)l;
        pl.n_levels = (int)(l2 - l);
        for (unsigned j = 0; j <= height; ++j) { pl.val_base[j] = lv.val_base[j]; pl.src_off[j] = lv.src_off[j]; }
        bool done = false;
        rc = enqueue_pedersen_path(d_felts, d_emp, s.flag, cnt[l], st, d_src, pl, cpts, &done);
        if (rc != SP_OK) return rc;
        if (done) { l = l2; continue; }
      }
      rc = enqueue_pedersen_sparse(d_felts, d_emp + 4 * l, d_felts + 4 * (size_t)lv.val_base[l + 1], s.flag, cnt[l + 1],
                                   st, s, d_src + lv.src_off[l], cpts ? cpts + 2 * l : nullptr);
      if (rc != SP_OK) return rc;
      ++l;
    }
  }
  tl_mark("tree: levels enqueued");
  if (enqueued) (*enqueued)();  // the library lock is free again: sp_order_batch lets its verifier through
  // ---- the device runs; nobody waits on the library lock for it ----
  // The status flag and the candidate root come back together: ONE wait per update (tree_wait).
  p.queued = true;  // from here on the stream holds work that reads the tree's buffers
  p.total = total;
  p.d_felts = d_felts;
  p.d_idx = d_idx;
  p.h_flag = h_flag;
  p.h_root = h_root;
  SP_HIP(hipMemcpyAsync(h_flag, s.flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  SP_HIP(hipMemcpyAsync(h_root, d_felts + 4 * (size_t)lv.val_base[height], 32, hipMemcpyDeviceToHost, st));
  return SP_OK;
}

// Waits for what tree_enqueue put on the stream; *flag = the update's status flag (0 for an empty update).
static int tree_wait(SparseTree& t, const TreePending& p, unsigned* flag) {
  *flag = 0;
  if (!p.queued) return SP_OK;
  SP_HIP(hipStreamSynchronize(t.stream));
  tl_mark("tree: levels hashed");
  *flag = *p.h_flag;
  return SP_OK;
}

// commit: every new node into the table, one launch - and nobody waits for it.  The tree's next
// operation is ordered behind it on the tree's stream (lookups, the next update's copies into the work
// buffer, the rehash of a growing table); a reallocation of the work buffer or sp_tree_destroy synchronise
// (hipFree / tree_free).  ~0.09 ms of 217 k hash-table insertions leave the caller's latency.
static int tree_commit(SparseTree& t, const TreePending& p, uint64_t* new_root) {
  hipLaunchKernelGGL(tree_insert_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, t.stream, t.table.ptr,
                     t.slots - 1, p.lv, p.d_idx, p.d_felts, (unsigned)p.total, t.d_entries);
  SP_HIP(hipGetLastError());
  std::memcpy(t.root, p.h_root, 32);
  t.has_root = true;
  t.entries += p.total;  // upper bound until tree_reserve reads the device counter again
  std::memcpy(new_root, t.root, 32);
  return SP_OK;
}

// One tree, the phases back to back.  `may_commit`, when given, is asked once every new node has been hashed and
// before anything is written to the table: false leaves the tree as it was (*status = SP_TREE_NOT_COMMITTED).
static int tree_update_locked(SparseTree& t, const uint64_t* keys, const uint64_t* leaves, size_t n, uint64_t* old_root,
                              uint64_t* new_root, uint8_t* status, const std::function<bool()>* may_commit,
                              const std::function<void()>* enqueued = nullptr) {
  TreePending p;
  int rc = tree_enqueue(t, keys, leaves, n, old_root, status, nullptr, p, enqueued);
  if (rc != SP_OK) {
    if (p.queued) (void)hipStreamSynchronize(t.stream);  // the copy-back failed: nothing may still run on `p`
    return rc;
  }
  if (!p.queued) {
    std::memcpy(new_root, old_root, 32);
    if (may_commit && !(*may_commit)() && status) *status = SP_TREE_NOT_COMMITTED;
    return SP_OK;
  }
  unsigned f = 0;
  rc = tree_wait(t, p, &f);
  if (rc != SP_OK) return rc;
  if (status) *status = (uint8_t)f;
  if (f != 0) {  // an input out of range or an unhashable pair: nothing was written, the tree is as it was
    std::memcpy(new_root, old_root, 32);
    return SP_OK;
  }
  if (may_commit && !(*may_commit)()) {
    if (status) *status = SP_TREE_NOT_COMMITTED;
    std::memcpy(new_root, old_root, 32);
    return SP_OK;
  }
  return tree_commit(t, p, new_root);
}

namespace sp {
void release_tree_state() {
  for (auto& kv : g_trees) tree_free(*kv.second);
  g_trees.clear();
}
}  // namespace sp

extern "C" {

int sp_tree_create_on(int context, unsigned height, const uint64_t* empty_leaf, int* tree) {
  SP_REQUIRE_READY();
  if (height < 1 || height > 64) { set_error("height must be in 1..64"); return SP_ERR_BAD_ARGUMENT; }
  if (context < 0 || context >= ctx_count() || !ctx_at(context).ready) { set_error("no such context"); return SP_ERR_BAD_ARGUMENT; }
  // an out-of-range empty leaf would poison the cached empty-subtree roots (their chain flags
  // SP_HASH_OUT_OF_RANGE once, later calls hit the cache and never see the flag again)
  if (!felt_below_p(empty_leaf)) { set_error("empty leaf must be a field element (< p)"); return SP_ERR_BAD_ARGUMENT; }
  ctx_lock lk(global_mu());
  auto t = std::make_shared<SparseTree>();
  t->height = height;
  t->ctx_index = context;
  std::memcpy(t->empty_leaf, empty_leaf, 32);
  const int id = g_next_tree++;
  g_trees.emplace(id, t);
  *tree = id;
  return SP_OK;
}

int sp_tree_create(unsigned height, const uint64_t* empty_leaf, int* tree) {
  return sp_tree_create_on(0, height, empty_leaf, tree);
}

int sp_tree_destroy(int tree) {
  SP_REQUIRE_READY();
  std::shared_ptr<SparseTree> keep;
  {
    TreeScope ts;
    int rc = ts.open(tree);
    if (rc != SP_OK) return rc;
    keep = ts.t;
    {
      ctx_lock lk(global_mu());
      g_trees.erase(tree);
    }
    tree_free(*ts.t);  // waits for the tree's stream
    ts.t->destroyed = true;
  }
  return SP_OK;
}

int sp_tree_root(int tree, uint64_t* root) {
  SP_REQUIRE_READY();
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  return tree_root_locked(*ts.t, root);
}

int sp_tree_get(int tree, const uint64_t* keys, size_t n, uint64_t* leaves) {
  SP_REQUIRE_READY();
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& t = *ts.t;
  if (!keys_ok(t.height, keys, n, false)) return SP_ERR_BAD_ARGUMENT;
  if (n == 0) return SP_OK;
  if (!t.table.ptr) {
    for (size_t i = 0; i < n; ++i) std::memcpy(leaves + 4 * i, t.empty_leaf, 32);
    return SP_OK;
  }
  if (n > 0xffffffffull) { set_error("too many keys"); return SP_ERR_BAD_ARGUMENT; }
  SP_HIP(t.buf.reserve(n * 40 + 64));
  uint64_t* d_keys = (uint64_t*)t.buf.ptr;
  uint64_t* d_emp = d_keys + n;
  uint64_t* d_out = d_emp + 4;
  SP_HIP(hipMemcpyAsync(d_keys, keys, n * 8, hipMemcpyHostToDevice, t.stream));
  SP_HIP(hipMemcpyAsync(d_emp, t.empty_leaf, 32, hipMemcpyHostToDevice, t.stream));
  hipLaunchKernelGGL(tree_get_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t.stream, t.table.ptr, t.slots - 1,
                     d_keys, (unsigned)n, d_emp, d_out);
  SP_HIP(hipGetLastError());
  SP_HIP(hipMemcpyAsync(leaves, d_out, n * 32, hipMemcpyDeviceToHost, t.stream));
  SP_HIP(hipStreamSynchronize(t.stream));
  return SP_OK;
}

// ---- witness export (include/starkperp.h): the preimages that main.cairo:39-40,61-64 takes as merkle_facts and that
// the merkle_multi_update calls of state/state.cairo:155-173 walk (merkle_tree.py:4-26), read back by position ----
int sp_tree_witness_size(unsigned height, const uint64_t* keys, size_t n, size_t* n_records) {
  if (!n_records || (n && !keys)) { set_error("sp_tree_witness_size: null argument"); return SP_ERR_BAD_ARGUMENT; }
  if (height < 1 || height > 64) { set_error("height must be in 1..64"); return SP_ERR_BAD_ARGUMENT; }
  if (!keys_ok(height, keys, n, true)) return SP_ERR_BAD_ARGUMENT;
  size_t records = 0;
  if (n) {
    std::vector<size_t> cnt;
    tree_level_counts(height, keys, n, cnt);
    for (unsigned l = 1; l <= height; ++l) records += cnt[l];
  }
  *n_records = records;
  return SP_OK;
}

int sp_tree_witness(int tree, const uint64_t* keys, size_t n, size_t capacity, uint8_t* level, uint64_t* index,
                    uint64_t* node, uint64_t* left, uint64_t* right, size_t* n_records) {
  SP_REQUIRE_READY();
  if (!n_records || (n && !keys)) { set_error("sp_tree_witness: null argument"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_tree_witness");
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& t = *ts.t;
  const unsigned height = t.height;
  if (!keys_ok(height, keys, n, true)) return SP_ERR_BAD_ARGUMENT;
  if (n == 0) { *n_records = 0; return SP_OK; }
  std::vector<size_t> cnt;
  TreeLevels lv;
  size_t total = 0, felts = 0, idxs = 0, srcs = 0;
  if (!tree_layout(height, keys, n, cnt, lv, total, felts, idxs, srcs)) { set_error("witness too large"); return SP_ERR_BAD_ARGUMENT; }
  const size_t records = total - n;  // every node above level 0
  *n_records = records;
  if (capacity < records) { set_error("sp_tree_witness: capacity below the record count"); return SP_ERR_BAD_ARGUMENT; }
  if (!level || !index || !node || !left || !right) { set_error("sp_tree_witness: null output array"); return SP_ERR_BAD_ARGUMENT; }
  std::vector<uint64_t> emp;
  rc = tree_empty_roots(t, emp);
  if (rc != SP_OK) return rc;
  if (!t.table.ptr) {  // never updated: every position is its level's empty-subtree root; the indices as the kernel finds them
    size_t u = 0;
    for (unsigned l = 1; l <= height; ++l) {
      for (size_t i = 0; i < n; ++i) {
        const uint64_t me = l < 64 ? keys[i] >> l : 0;
        if (i > 0 && (l < 64 ? keys[i - 1] >> l : 0) == me) continue;
        level[u] = (uint8_t)l;
        index[u] = me;
        std::memcpy(node + 4 * u, &emp[4 * l], 32);
        std::memcpy(left + 4 * u, &emp[4 * (l - 1)], 32);
        std::memcpy(right + 4 * u, &emp[4 * (l - 1)], 32);
        ++u;
      }
    }
    return SP_OK;
  }
  // work buffer: empty roots | node indices of levels 0 .. height (level 0 = the keys) | node | left | right values.
  // What goes back - the indices of levels 1 .. height and the three value arrays - is one contiguous piece.
  const size_t emp_bytes = ((size_t)height + 1) * 32, in_bytes = emp_bytes + n * 8, out_bytes = records * (8 + 96);
  SP_HIP(t.buf.reserve(in_bytes + out_bytes + 64));
  char* b = (char*)t.buf.ptr;
  uint64_t* d_emp = (uint64_t*)b;
  uint64_t* d_idx = (uint64_t*)(b + emp_bytes);
  uint64_t* d_node = d_idx + total;
  uint64_t* d_left = d_node + 4 * records;
  uint64_t* d_right = d_left + 4 * records;
  hipStream_t st = t.stream;
  tl_mark("witness: work buffer ready");
  // small results through the tree's page-locked buffer (its previous user has finished: every operation ends with a
  // wait on the stream), larger ones directly into the caller's arrays
  StagedTrip trip(t.hbuf, in_bytes + out_bytes, st);
  SP_HIP(trip.up(d_emp, {{emp.data(), emp_bytes}, {keys, n * 8}}));
  hipLaunchKernelGGL(tree_level_nodes_kernel, dim3(height), dim3(1024), 0, st, lv, d_idx, d_idx);
  hipLaunchKernelGGL(tree_witness_kernel, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, st, lv, d_idx, t.table.ptr,
                     t.slots - 1, d_emp, d_node, d_left, d_right, (unsigned)records);
  SP_HIP(hipGetLastError());
  tl_mark("witness: kernels enqueued");
  if (timeline.mine) {  // diagnostics only (STARKPERP_TIMELINE=1): an extra wait that tells the kernels from the copy back
    SP_HIP(hipStreamSynchronize(st));
    tl_mark("witness: kernels done");
  }
  const std::initializer_list<Piece> outs = {{index, records * 8}, {node, records * 32}, {left, records * 32},
                                             {right, records * 32}};
  SP_HIP(trip.down(d_idx + n, outs));
  SP_HIP(hipStreamSynchronize(st));
  tl_mark("witness: results on the host");
  trip.finish(outs);
  // the level of a record is a function of the level counts alone: filled here, it does not cross PCIe
  size_t u = 0;
  for (unsigned l = 1; l <= height; ++l) {
    std::memset(level + u, (int)l, cnt[l]);
    u += cnt[l];
  }
  return SP_OK;
}

int sp_tree_prove(int tree, const uint64_t* keys, size_t n, uint64_t* leaves, uint64_t* siblings) {
  SP_REQUIRE_READY();
  if (n && (!keys || !leaves || !siblings)) { set_error("sp_tree_prove: null argument"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_tree_prove");
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& t = *ts.t;
  const unsigned height = t.height;
  if (!keys_ok(height, keys, n, false)) return SP_ERR_BAD_ARGUMENT;
  if (n == 0) return SP_OK;
  if (n > 0x7fffffffull / height) { set_error("too many keys"); return SP_ERR_BAD_ARGUMENT; }
  const size_t pairs = n * height;
  std::vector<uint64_t> emp;
  rc = tree_empty_roots(t, emp);
  if (rc != SP_OK) return rc;
  if (!t.table.ptr) {  // never updated: the empty leaf under a path of empty-subtree roots
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(leaves + 4 * i, emp.data(), 32);
      std::memcpy(siblings + 4 * i * height, emp.data(), (size_t)height * 32);
    }
    return SP_OK;
  }
  // work buffer: empty roots | keys | leaves | siblings; leaves and siblings go back as one piece
  const size_t emp_bytes = ((size_t)height + 1) * 32, in_bytes = emp_bytes + n * 8, out_bytes = (n + pairs) * 32;
  SP_HIP(t.buf.reserve(in_bytes + out_bytes + 64));
  char* b = (char*)t.buf.ptr;
  uint64_t* d_emp = (uint64_t*)b;
  uint64_t* d_keys = (uint64_t*)(b + emp_bytes);
  uint64_t* d_leaves = d_keys + n;
  uint64_t* d_sib = d_leaves + 4 * n;
  hipStream_t st = t.stream;
  tl_mark("prove: work buffer ready");
  StagedTrip trip(t.hbuf, in_bytes + out_bytes, st);
  SP_HIP(trip.up(d_emp, {{emp.data(), emp_bytes}, {keys, n * 8}}));
  hipLaunchKernelGGL(tree_prove_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, t.table.ptr, t.slots - 1,
                     d_keys, height, d_emp, d_leaves, d_sib, (unsigned)pairs);
  SP_HIP(hipGetLastError());
  tl_mark("prove: kernel enqueued");
  if (timeline.mine) {  // diagnostics only, as in sp_tree_witness
    SP_HIP(hipStreamSynchronize(st));
    tl_mark("prove: kernel done");
  }
  const std::initializer_list<Piece> outs = {{leaves, n * 32}, {siblings, pairs * 32}};
  SP_HIP(trip.down(d_leaves, outs));
  SP_HIP(hipStreamSynchronize(st));
  tl_mark("prove: results on the host");
  trip.finish(outs);
  return SP_OK;
}

// The table's size as it stands: the device counter of claimed slots (read-only) and the slot count.
int sp_tree_table_size(int tree, uint64_t* entries, uint64_t* slots) {
  SP_REQUIRE_READY();
  if (!entries || !slots) { set_error("sp_tree_table_size: null argument"); return SP_ERR_BAD_ARGUMENT; }
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& t = *ts.t;
  unsigned long long used = 0;
  if (t.d_entries) {
    SP_HIP(hipMemcpyAsync(&used, t.d_entries, sizeof(used), hipMemcpyDeviceToHost, t.stream));
    SP_HIP(hipStreamSynchronize(t.stream));
  }
  *entries = used;
  *slots = t.slots;
  return SP_OK;
}

// ---- sp_tree_scan (include/starkperp.h): which keys a tree holds, in order, in pages - the descent of
// tree_scan_top_kernel / tree_scan_step_kernel.  Everything on the tree's stream under the tree's mutex, so a page
// describes a batch boundary; one wait, at the end. ----
int sp_tree_scan(int tree, uint64_t lo, uint64_t hi, size_t capacity, uint64_t* keys, uint64_t* leaves, size_t* n,
                 int* more) {
  SP_REQUIRE_READY();
  if (!keys || !leaves || !n || !more) { set_error("sp_tree_scan: null argument"); return SP_ERR_BAD_ARGUMENT; }
  if (capacity == 0) { set_error("sp_tree_scan: capacity must be at least 1"); return SP_ERR_BAD_ARGUMENT; }
  if (lo > hi) { set_error("sp_tree_scan: lo above hi"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_tree_scan");
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& t = *ts.t;
  const unsigned height = t.height;
  if (height < 64 && (hi >> height) != 0) { set_error("sp_tree_scan: hi out of range for height"); return SP_ERR_BAD_ARGUMENT; }
  if (!t.table.ptr || !t.has_root) {  // never updated: no launch
    *n = 0;
    *more = 0;
    return SP_OK;
  }
  std::vector<uint64_t> emp;
  rc = tree_empty_roots(t, emp);
  if (rc != SP_OK) return rc;
  if (std::memcmp(t.root, &emp[4 * (size_t)height], 32) == 0) {  // the frontier of level `height` is empty
    *n = 0;
    *more = 0;
    return SP_OK;
  }
  const size_t cap = capacity < SP_TREE_SCAN_MAX ? capacity : SP_TREE_SCAN_MAX;
  const size_t wide = cap + 2;  // what a frontier above level 0 keeps (scan_limit)
  const size_t blocks = (wide + SCAN_BLOCK - 1) / SCAN_BLOCK;
  // work buffer: empty roots | header, keys (= frontier 0), leaves: what goes back, one piece | frontier 1 | marks 0 |
  // marks 1 | cnt[65], tot[height + 1][blocks]: cleared once
  const size_t emp_bytes = ((size_t)height + 1) * 32, out_bytes = sizeof(ScanHeader) + wide * 8 + cap * 32;
  const size_t f1_off = emp_bytes + out_bytes, m_off = f1_off + wide * 8, z_off = (m_off + 2 * wide + 15) & ~(size_t)15;
  const size_t z_bytes = (65 + ((size_t)height + 1) * blocks) * sizeof(unsigned);
  SP_HIP(t.buf.reserve(z_off + z_bytes + 64));
  char* b = (char*)t.buf.ptr;
  ScanWork w;
  w.tab = t.table.ptr;
  w.mask = t.slots - 1;
  w.emp = (const uint64_t*)b;
  w.lo = lo;
  w.hi = hi;
  w.cap = (unsigned)cap;
  w.blocks = (unsigned)blocks;
  w.hdr = (ScanHeader*)(b + emp_bytes);
  w.frontier[0] = (uint64_t*)(b + emp_bytes + sizeof(ScanHeader));
  w.leaves = w.frontier[0] + wide;
  w.frontier[1] = (uint64_t*)(b + f1_off);
  w.marks[0] = (uint8_t*)(b + m_off);
  w.marks[1] = w.marks[0] + wide;
  w.cnt = (unsigned*)(b + z_off);
  w.tot = w.cnt + 65;
  hipStream_t st = t.stream;
  tl_mark("scan: work buffer ready");
  // a page up to 4 MiB comes back through the tree's page-locked buffer in one copy; above that the header comes back
  // first and the n keys and leaves go directly into the caller's arrays
  const bool whole = StagedTrip::fits(emp_bytes + out_bytes);
  StagedTrip trip(t.hbuf, whole ? emp_bytes + out_bytes : emp_bytes + sizeof(ScanHeader), st);
  char* const stage = trip.stage;
  SP_HIP(trip.up(b, {{emp.data(), emp_bytes}}));
  SP_HIP(hipMemsetAsync(b + z_off, 0, z_bytes, st));
  hipLaunchKernelGGL(tree_scan_top_kernel, dim3(1), dim3(SCAN_TOP), 0, st, w, height);
  // The frontier of level height - k has at most 2^k nodes, so the top kernel hands over at level height - 11 or
  // below, and never when cap + 2 <= SCAN_TOP: those launches are not made.  The others find on the device whether their
  // level is theirs.
  if (wide > SCAN_TOP) {
    for (unsigned level = height > 11 ? height - 11 : 0; level >= 1; --level) {
      hipLaunchKernelGGL(tree_scan_step_kernel, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, st, w, level);
    }
  }
  SP_HIP(hipGetLastError());
  tl_mark("scan: kernels enqueued");
  if (timeline.mine) {  // diagnostics only, as in sp_tree_witness
    SP_HIP(hipStreamSynchronize(st));
    tl_mark("scan: kernels done");
  }
  ScanHeader h;
  h.n = 0;
  h.more = 0;
  h.start = 0;
  if (stage && whole) {  // the whole page in one copy; what the header counts goes on to the caller
    SP_HIP(trip.down(w.hdr, {{&h, sizeof(h)}, {keys, wide * 8}, {leaves, cap * 32}}));
    SP_HIP(hipStreamSynchronize(st));
    trip.finish({{&h, sizeof(h)}});
    if (h.n > cap) { set_error("sp_tree_scan: inconsistent count"); return SP_ERR_HIP; }
    trip.finish({{nullptr, sizeof(h)}, {keys, h.n * 8}, {nullptr, (wide - h.n) * 8}, {leaves, h.n * 32}});
  } else {
    SP_HIP(hipMemcpyAsync(stage ? (void*)(stage + emp_bytes) : (void*)&h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    SP_HIP(hipStreamSynchronize(st));
    if (stage) std::memcpy(&h, stage + emp_bytes, sizeof(h));
    if (h.n > cap) { set_error("sp_tree_scan: inconsistent count"); return SP_ERR_HIP; }
    if (h.n) {
      SP_HIP(hipMemcpyAsync(keys, w.frontier[0], h.n * 8, hipMemcpyDeviceToHost, st));
      SP_HIP(hipMemcpyAsync(leaves, w.leaves, h.n * 32, hipMemcpyDeviceToHost, st));
      SP_HIP(hipStreamSynchronize(st));
    }
  }
  tl_mark("scan: results on the host");
  *n = (size_t)h.n;
  *more = h.more ? 1 : 0;
  return SP_OK;
}

// ---- sp_tree_clone (include/starkperp.h): a second handle on the same tree - device copies, nothing hashed.  The
// source's mutex is held from start to end.  The copies are enqueued on the SOURCE's stream, behind the insert kernel of
// its last commit (which nobody has waited for), and waited for before the call returns.  Nothing of the clone is
// registered before every allocation and copy has succeeded: a failure leaves no handle and the source as it was. ----
int sp_tree_clone(int tree, int* clone) {
  SP_REQUIRE_READY();
  if (!clone) { set_error("sp_tree_clone: null argument"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_tree_clone");
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  SparseTree& s = *ts.t;
  auto t = std::make_shared<SparseTree>();
  t->height = s.height;
  t->ctx_index = s.ctx_index;
  std::memcpy(t->empty_leaf, s.empty_leaf, 32);
  t->has_root = s.has_root;
  std::memcpy(t->root, s.root, 32);
  // stream, work buffer, staging buffer: the clone's own, made by its first call as a created tree's are; the per-level
  // constant points are recomputed by its first update (cpts_state 0)
  if (s.table.ptr || s.d_entries) {  // a tree that was never updated has neither: its clone is a fresh tree, no device work
    TreeSlot* table = nullptr;
    unsigned long long* counter = nullptr;
    hipError_t e = hipSuccess;
    const char* what = "hipMalloc (the clone's table)";
    if (s.table.ptr) e = hipMalloc(&table, s.slots * sizeof(TreeSlot));
    if (e == hipSuccess && s.d_entries) {
      what = "hipMalloc (the clone's entry counter)";
      e = hipMalloc(&counter, sizeof(unsigned long long));
    }
    if (e == hipSuccess && table) {
      what = "hipMemcpyAsync (table, device to device)";
      e = hipMemcpyAsync(table, s.table.ptr, s.slots * sizeof(TreeSlot), hipMemcpyDeviceToDevice, s.stream);
    }
    if (e == hipSuccess && counter) {
      what = "hipMemcpyAsync (entry counter, device to device)";
      e = hipMemcpyAsync(counter, s.d_entries, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s.stream);
    }
    tl_mark("clone: copies enqueued");
    // also on a failure: a copy that did get onto the stream writes into what is freed below
    const hipError_t waited = hipStreamSynchronize(s.stream);
    if (e == hipSuccess && waited != hipSuccess) {
      what = "hipStreamSynchronize (the source's stream)";
      e = waited;
    }
    if (e != hipSuccess) {
      if (table) (void)hipFree(table);
      if (counter) (void)hipFree(counter);
      return hip_fail(e, what);
    }
    tl_mark("clone: copies done");
    t->table.ptr = table;
    t->table.bytes = table ? s.slots * sizeof(TreeSlot) : 0;
    t->slots = table ? s.slots : 0;
    t->d_entries = counter;
    t->entries = s.entries;
  }
  ctx_lock lk(global_mu());
  const int id = g_next_tree++;
  g_trees.emplace(id, t);
  *clone = id;
  return SP_OK;
}

// ---- sp_tree_diff (include/starkperp.h): where two trees differ, in order, in pages - the descent of
// tree_diff_top_kernel / tree_diff_step_kernel.  Both tree mutexes from start to end, taken in ascending handle order
// (as sp_state_batch takes them: diff(a, b) beside diff(b, a) cannot block); the work runs on the stream and in the work
// buffer of the lower handle, behind a wait for the other tree's stream (the insert kernel of its last commit may
// still be in flight); the library lock only inside tree_empty_roots.  One wait, at the end. ----
int sp_tree_diff(int tree_a, int tree_b, uint64_t lo, uint64_t hi, size_t capacity, uint64_t* keys, uint64_t* leaves_a,
                 uint64_t* leaves_b, size_t* n, int* more) {
  SP_REQUIRE_READY();
  if (!keys || !leaves_a || !leaves_b || !n || !more) { set_error("sp_tree_diff: null argument"); return SP_ERR_BAD_ARGUMENT; }
  if (capacity == 0) { set_error("sp_tree_diff: capacity must be at least 1"); return SP_ERR_BAD_ARGUMENT; }
  if (lo > hi) { set_error("sp_tree_diff: lo above hi"); return SP_ERR_BAD_ARGUMENT; }
  if (tree_a == tree_b) { set_error("sp_tree_diff: the same tree handle twice"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_tree_diff");
  TreeScope first, second;
  const bool a_first = tree_a < tree_b;
  int rc = first.open(a_first ? tree_a : tree_b);
  if (rc != SP_OK) return rc;
  rc = second.open(a_first ? tree_b : tree_a);
  if (rc != SP_OK) return rc;
  SparseTree& A = a_first ? *first.t : *second.t;
  SparseTree& B = a_first ? *second.t : *first.t;
  SparseTree& t = *first.t;      // whose stream, work buffer and staging buffer serve the call
  SparseTree& other = *second.t;
  if (A.ctx_index != B.ctx_index) { set_error("sp_tree_diff: the two trees live on different contexts"); return SP_ERR_BAD_ARGUMENT; }
  if (A.height != B.height) { set_error("sp_tree_diff: the two trees differ in height"); return SP_ERR_BAD_ARGUMENT; }
  if (std::memcmp(A.empty_leaf, B.empty_leaf, 32) != 0) {
    set_error("sp_tree_diff: the two trees differ in their empty leaf");
    return SP_ERR_BAD_ARGUMENT;
  }
  const unsigned height = A.height;
  if (height < 64 && (hi >> height) != 0) { set_error("sp_tree_diff: hi out of range for height"); return SP_ERR_BAD_ARGUMENT; }
  std::vector<uint64_t> emp;
  rc = tree_empty_roots(A, emp);
  if (rc != SP_OK) return rc;
  const uint64_t* empty_root = &emp[4 * (size_t)height];
  // a tree without a committed update stands at the empty root, whether its table exists (a rejected first update) or not
  if (std::memcmp(A.has_root ? A.root : empty_root, B.has_root ? B.root : empty_root, 32) == 0) {
    *n = 0;  // equal roots: the frontier of level `height` is empty, no launch
    *more = 0;
    return SP_OK;
  }
  const size_t cap = capacity < SP_TREE_DIFF_MAX ? capacity : SP_TREE_DIFF_MAX;
  const size_t wide = cap + 2;  // what a frontier above level 0 keeps (diff_limit)
  const size_t blocks = (wide + SCAN_BLOCK - 1) / SCAN_BLOCK;
  // work buffer: empty roots | header, keys (= frontier 0), leaves of A, leaves of B: what goes back, one piece |
  // frontier 1 | marks 0 | marks 1 | the zeroed slot, cnt[65], tot[height + 1][blocks]: cleared once
  const size_t emp_bytes = ((size_t)height + 1) * 32, out_bytes = sizeof(ScanHeader) + wide * 8 + 2 * cap * 32;
  const size_t f1_off = emp_bytes + out_bytes, m_off = f1_off + wide * 8, z_off = (m_off + 2 * wide + 15) & ~(size_t)15;
  const size_t none_bytes = 64;  // one TreeSlot, 16-byte aligned
  const size_t z_bytes = none_bytes + (65 + ((size_t)height + 1) * blocks) * sizeof(unsigned);
  SP_HIP(t.buf.reserve(z_off + z_bytes + 64));
  char* b = (char*)t.buf.ptr;
  DiffWork w;
  w.tab[0] = A.has_root ? A.table.ptr : nullptr;  // (a table without a root holds nothing)
  w.tab[1] = B.has_root ? B.table.ptr : nullptr;
  w.mask[0] = w.tab[0] ? A.slots - 1 : 0;
  w.mask[1] = w.tab[1] ? B.slots - 1 : 0;
  w.none = (const TreeSlot*)(b + z_off);
  w.emp = (const uint64_t*)b;
  w.lo = lo;
  w.hi = hi;
  w.cap = (unsigned)cap;
  w.blocks = (unsigned)blocks;
  w.hdr = (ScanHeader*)(b + emp_bytes);
  w.frontier[0] = (uint64_t*)(b + emp_bytes + sizeof(ScanHeader));
  w.leaves[0] = w.frontier[0] + wide;
  w.leaves[1] = w.leaves[0] + 4 * cap;
  w.frontier[1] = (uint64_t*)(b + f1_off);
  w.marks[0] = (uint8_t*)(b + m_off);
  w.marks[1] = w.marks[0] + wide;
  w.cnt = (unsigned*)(b + z_off + none_bytes);
  w.tot = w.cnt + 65;
  hipStream_t st = t.stream;
  // the other tree's last commit (its insert kernel, the rehash of a growth) may still be in flight on ITS stream; the
  // call is synchronous and holds both mutexes, so nothing of either tree starts before the reads below are done
  SP_HIP(hipStreamSynchronize(other.stream));
  tl_mark("diff: work buffer ready");
  const bool whole = StagedTrip::fits(emp_bytes + out_bytes);
  StagedTrip trip(t.hbuf, whole ? emp_bytes + out_bytes : emp_bytes + sizeof(ScanHeader), st);
  char* const stage = trip.stage;
  SP_HIP(trip.up(b, {{emp.data(), emp_bytes}}));
  SP_HIP(hipMemsetAsync(b + z_off, 0, z_bytes, st));
  hipLaunchKernelGGL(tree_diff_top_kernel, dim3(1), dim3(SCAN_TOP), 0, st, w, height);
  // as in sp_tree_scan: the top kernel hands over at level height - 11 or below, and never when cap + 2 <= SCAN_TOP
  if (wide > SCAN_TOP) {
    for (unsigned level = height > 11 ? height - 11 : 0; level >= 1; --level) {
      hipLaunchKernelGGL(tree_diff_step_kernel, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, st, w, level);
    }
  }
  SP_HIP(hipGetLastError());
  tl_mark("diff: kernels enqueued");
  if (timeline.mine) {  // diagnostics only, as in sp_tree_witness
    SP_HIP(hipStreamSynchronize(st));
    tl_mark("diff: kernels done");
  }
  ScanHeader h;
  h.n = 0;
  h.more = 0;
  h.start = 0;
  if (stage && whole) {  // the whole page in one copy; what the header counts goes on to the caller
    SP_HIP(trip.down(w.hdr, {{&h, sizeof(h)}, {keys, wide * 8}, {leaves_a, cap * 32}, {leaves_b, cap * 32}}));
    SP_HIP(hipStreamSynchronize(st));
    trip.finish({{&h, sizeof(h)}});
    if (h.n > cap) { set_error("sp_tree_diff: inconsistent count"); return SP_ERR_HIP; }
    trip.finish({{nullptr, sizeof(h)}, {keys, h.n * 8}, {nullptr, (wide - h.n) * 8}, {leaves_a, h.n * 32},
                 {nullptr, (cap - h.n) * 32}, {leaves_b, h.n * 32}});
  } else {  // the header first, then exactly n keys and two runs of n leaves
    SP_HIP(hipMemcpyAsync(stage ? (void*)(stage + emp_bytes) : (void*)&h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, st));
    SP_HIP(hipStreamSynchronize(st));
    if (stage) std::memcpy(&h, stage + emp_bytes, sizeof(h));
    if (h.n > cap) { set_error("sp_tree_diff: inconsistent count"); return SP_ERR_HIP; }
    if (h.n) {
      SP_HIP(hipMemcpyAsync(keys, w.frontier[0], h.n * 8, hipMemcpyDeviceToHost, st));
      SP_HIP(hipMemcpyAsync(leaves_a, w.leaves[0], h.n * 32, hipMemcpyDeviceToHost, st));
      SP_HIP(hipMemcpyAsync(leaves_b, w.leaves[1], h.n * 32, hipMemcpyDeviceToHost, st));
      SP_HIP(hipStreamSynchronize(st));
    }
  }
  tl_mark("diff: results on the host");
  *n = (size_t)h.n;
  *more = h.more ? 1 : 0;
  return SP_OK;
}

// ---- sp_merkle_verify_update[_dev] (include/starkperp.h): merkle_multi_update's statement (state/state.cairo:155-173)
// checked against two witnesses, stateless.  The position structure is the update's own - tree_layout, then
// tree_level_nodes_kernel and tree_children_kernel on the keys - one enqueue_pedersen hashes all 2 R records (both
// halves are one contiguous array), witness_check_kernel compares. ----
struct VerifyShape {
  TreeLevels lv;
  size_t total = 0, idxs = 0, records = 0;
  unsigned top = 0;  // nodes of level `height` (1)
};
// The arguments both calls share; false: a bad argument, the text is in sp_last_error.  n == 0 leaves `vs` unset.
static bool verify_update_args(unsigned height, const uint64_t* keys, size_t n, const void* prev_leaves,
                               const void* new_leaves, const void* prev_root, const void* new_root, const void* node,
                               const void* left, const void* right, size_t n_records, const void* verdict, VerifyShape& vs) {
  if (height < 1 || height > 64) { set_error("height must be in 1..64"); return false; }
  if (!prev_root || !new_root || !verdict) { set_error("sp_merkle_verify_update: null argument"); return false; }
  if (n == 0) {
    if (n_records != 0) { set_error("sp_merkle_verify_update: n_records is not the witness size of the keys"); return false; }
    return true;
  }
  if (!keys || !prev_leaves || !new_leaves || !node || !left || !right) {
    set_error("sp_merkle_verify_update: null argument");
    return false;
  }
  if (!keys_ok(height, keys, n, true)) return false;
  std::vector<size_t> cnt;
  size_t felts = 0, srcs = 0;
  if (!tree_layout(height, keys, n, cnt, vs.lv, vs.total, felts, vs.idxs, srcs) || 2 * (vs.total - n) >= 0x80000000ull) {
    set_error("sp_merkle_verify_update: witness too large");
    return false;
  }
  vs.records = vs.total - n;  // = srcs: one child list per record
  vs.top = (unsigned)cnt[height];
  if (n_records != vs.records) { set_error("sp_merkle_verify_update: n_records is not the witness size of the keys"); return false; }
  return true;
}
static bool roots_equal(const uint64_t* a, const uint64_t* b) { return std::memcmp(a, b, 32) == 0; }

// Everything on the device but keys and roots (host); enqueues on `st` and returns once both are in the stream's
// page-locked buffer.  The caller holds the library lock (scratch map, work-buffer map, launch bookkeeping).
static int enqueue_verify_update(const VerifyShape& vs, const uint64_t* keys, size_t n, const uint64_t* prev_leaves,
                                 const uint64_t* new_leaves, const uint64_t* prev_root, const uint64_t* new_root,
                                 const uint64_t* node, const uint64_t* left, const uint64_t* right, uint8_t* verdict,
                                 uint8_t* status, hipStream_t st) {
  const size_t R = vs.records;
  // work buffer: roots (2 felts) | node indices, level 0 = the keys | child lists | hashes of the 2 R records | status
  const size_t idx_off = 64, src_off = idx_off + vs.idxs * 8;
  const size_t hash_off = (src_off + R * sizeof(int2) + 31) & ~(size_t)31, hst_off = hash_off + 2 * R * 32;
  const size_t need = hst_off + 2 * R + 64;
  VerifyWork& w = g_verify_work[stream_key(st)];
  if (need > w.bytes) SP_HIP(w.grow(need + need / 4, st));
  char* b = w.ptr;
  uint64_t* d_roots = (uint64_t*)b;
  uint64_t* d_idx = (uint64_t*)(b + idx_off);
  int2* d_src = (int2*)(b + src_off);
  uint64_t* d_hashed = (uint64_t*)(b + hash_off);
  uint8_t* d_hst = (uint8_t*)(b + hst_off);
  // roots and keys are adjacent on the device: one copy out of the page-locked buffer
  int rc = stage_copy({{prev_root, 32}, {new_root, 32}, {keys, n * 8}}, d_roots, st);
  if (rc != SP_OK) return rc;
  SP_HIP(hipMemsetAsync(verdict, SP_PATH_TRUE, 1, st));
  hipLaunchKernelGGL(tree_level_nodes_kernel, dim3(vs.lv.height), dim3(1024), 0, st, vs.lv, d_idx, d_idx);
  hipLaunchKernelGGL(tree_children_kernel, dim3((unsigned)((vs.total - vs.top + 255) / 256)), dim3(256), 0, st, vs.lv,
                     d_idx, d_src, (unsigned)(vs.total - vs.top));
  SP_HIP(hipGetLastError());
  Scratch s;
  rc = get_scratch_public(2 * R, s, st);
  if (rc != SP_OK) return rc;
  rc = enqueue_pedersen(left, 1, right, 1, d_hashed, 1, d_hst, nullptr, 2 * R, st, s, nullptr);
  if (rc != SP_OK) return rc;
  hipLaunchKernelGGL(witness_check_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, vs.lv, d_src, node, left,
                     right, d_hashed, d_hst, prev_leaves, new_leaves, d_roots, status, verdict, (unsigned)R);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

int sp_merkle_verify_update_dev(unsigned height, const uint64_t* keys, size_t n, const uint64_t* prev_leaves,
                                const uint64_t* new_leaves, const uint64_t* prev_root, const uint64_t* new_root,
                                const uint64_t* node, const uint64_t* left, const uint64_t* right, size_t n_records,
                                uint8_t* verdict, uint8_t* status, void* stream) {
  CtxByPointer sp_ctx_sel__(verdict);  // the context of the device these pointers live on
  SP_REQUIRE_READY();
  VerifyShape vs;
  if (!verify_update_args(height, keys, n, prev_leaves, new_leaves, prev_root, new_root, node, left, right, n_records,
                          verdict, vs)) return SP_ERR_BAD_ARGUMENT;
  if (n == 0) {
    SP_HIP(hipMemsetAsync(verdict, roots_equal(prev_root, new_root) ? SP_PATH_TRUE : SP_PATH_FALSE, 1, (hipStream_t)stream));
    return SP_OK;
  }
  ctx_lock lk(ctx().mu);
  return enqueue_verify_update(vs, keys, n, prev_leaves, new_leaves, prev_root, new_root, node, left, right, verdict,
                               status, (hipStream_t)stream);
}

// Host-pointer variant on a host lane: the three record arrays and the leaves up (one staged copy up to
// PINNED_STAGE_MAX, five direct ones above it, as sp_tree_witness's results come down), one enqueue under the library
// lock, the verdict byte - and the status bytes when asked for - down.
int sp_merkle_verify_update(unsigned height, const uint64_t* keys, size_t n, const uint64_t* prev_leaves,
                            const uint64_t* new_leaves, const uint64_t* prev_root, const uint64_t* new_root,
                            const uint64_t* node, const uint64_t* left, const uint64_t* right, size_t n_records,
                            uint8_t* verdict, uint8_t* status) {
  LaneScope ls(0);  // the primary context, as sp_merkle_verify_paths
  SP_REQUIRE_READY();
  VerifyShape vs;
  if (!verify_update_args(height, keys, n, prev_leaves, new_leaves, prev_root, new_root, node, left, right, n_records,
                          verdict, vs)) return SP_ERR_BAD_ARGUMENT;
  if (n == 0) {
    *verdict = roots_equal(prev_root, new_root) ? SP_PATH_TRUE : SP_PATH_FALSE;
    return SP_OK;
  }
  if (ls.open() != SP_OK) return SP_ERR_HIP;
  HostLane& L = *ls.lane;
  const size_t R = vs.records;
  // device: node | left | right (2 R felts each) | previous leaves | new leaves | verdict (one word) | status bytes
  const size_t rec_bytes = 2 * R * 32, leaf_bytes = n * 32, in_bytes = 3 * rec_bytes + 2 * leaf_bytes;
  const size_t out_bytes = 4 + (status ? 2 * R : 0);
  SP_HIP(L.io.reserve(in_bytes + 4 + 2 * R + 64));
  char* b = (char*)L.io.ptr;
  uint64_t* d_node = (uint64_t*)b;
  uint64_t* d_left = d_node + 8 * R;
  uint64_t* d_right = d_left + 8 * R;
  uint64_t* d_prev = d_right + 8 * R;
  uint64_t* d_new = d_prev + 4 * n;
  uint8_t* d_verdict = (uint8_t*)(b + in_bytes);
  uint8_t* d_status = d_verdict + 4;
  StagedTrip trip(L.hio, in_bytes + out_bytes, L.stream);
  SP_HIP(trip.up(d_node, {{node, rec_bytes}, {left, rec_bytes}, {right, rec_bytes}, {prev_leaves, leaf_bytes},
                          {new_leaves, leaf_bytes}}));
  int rc;
  {
    ctx_lock lk(ctx().mu);
    rc = enqueue_verify_update(vs, keys, n, d_prev, d_new, prev_root, new_root, d_node, d_left, d_right, d_verdict,
                               d_status, L.stream);
  }
  if (rc != SP_OK) return rc;
  uint8_t v = SP_PATH_FALSE;  // written by the stream, read after the synchronisation below
  // the verdict byte, the rest of its word, the status bytes when asked for
  const std::initializer_list<Piece> outs = {{&v, 1}, {nullptr, 3}, {status, out_bytes - 4}};
  SP_HIP(trip.down(d_verdict, outs));
  SP_HIP(hipStreamSynchronize(L.stream));
  trip.finish(outs);
  *verdict = v;
  return SP_OK;
}

int sp_tree_update(int tree, const uint64_t* keys, const uint64_t* leaves, size_t n, uint64_t* old_root,
                   uint64_t* new_root, uint8_t* status) {
  SP_REQUIRE_READY();
  TreeScope ts;
  int rc = ts.open(tree);
  if (rc != SP_OK) return rc;
  return tree_update_locked(*ts.t, keys, leaves, n, old_root, new_root, status, nullptr);
}

// BASELINE.json configs[2] in ONE call: message-hash chains -> keyed signature verification -> order ids ->
// orders-tree update, without returning to the caller between the stages (services/perpetual/cairo/order:
// limit_order.cairo:24-52 hashes the order, order.cairo:23-31 takes the order id from the top 64 bits of the
// message hash, :122-124 writes the fulfilled amount at that id, verify_ecdsa_signature checks the signature).
//   words      depth x n felts, word-major (word k of order i at words + 4 (k n + i)): the chain
//              h = H(...H(H(w0, w1), w2)..., w_{depth-1}) is the message hash z_i (written to z_out)
//   r, s, qx, qy   the signatures and public keys (qy == NULL: x-only keys), verified against z_i through the
//              key tables; verdicts[i] as sp_ecdsa_verify_batch (z_i >= 2^251: SP_VERIFY_ASSERT_MSG, nothing committed)
//   leaves     the new orders-tree leaf of order i; its key is bits [id_shift, id_shift + 64) of z_i
// The verification runs on a host lane WHILE the tree update's levels are hashed on the tree's stream; the new
// nodes are committed only if every signature verified (the batch is all-or-nothing in the Cairo program),
// otherwise *tree_status = SP_TREE_NOT_COMMITTED and the tree is unchanged.  Two orders with the same id are an
// error (the caller squashes them first, state/state.cairo:67-96).
int sp_order_batch(const uint64_t* words, size_t depth, size_t n, const uint64_t* r, const uint64_t* s,
                   const uint64_t* qx, const uint64_t* qy, int tree, const uint64_t* leaves, unsigned id_shift,
                   uint64_t* z_out, uint8_t* verdicts, uint64_t* old_root, uint64_t* new_root, uint8_t* tree_status) {
  SP_REQUIRE_READY();
  if (depth < 1 || id_shift > 192) { set_error("sp_order_batch: bad chain depth or id shift"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_order_batch");
  uint8_t chain_status = 0;
  int rc = sp_pedersen_chains(words, n, depth, z_out, &chain_status);
  if (rc != SP_OK) return rc;
  tl_mark("chains done");
  if (chain_status != 0) {  // a word out of range / an unhashable pair: nothing else runs
    if (tree_status) *tree_status = chain_status;
    for (size_t i = 0; i < n; ++i) verdicts[i] = 0;
    rc = sp_tree_root(tree, old_root);  // its own code and error text (a bad handle is not a HIP failure and v.v.)
    if (rc != SP_OK) return rc;
    std::memcpy(new_root, old_root, 32);
    return SP_OK;
  }
  // A message hash of 2^251 or more is not a signed message (constants.cairo:57 SIGNED_MESSAGE_BOUND,
  // order.cairo:22; signature.py:227 asserts the same bound): its order id would not fit the 64-bit field, so
  // the batch cannot be committed - the verdicts say which orders (SP_VERIFY_ASSERT_MSG) and the tree stays.
  bool unsigned_message = false;
  for (size_t i = 0; i < n; ++i) unsigned_message |= (z_out[4 * i + 3] >> 59) != 0;
  if (unsigned_message) {
    rc = sp_ecdsa_verify_batch_keyed(z_out, r, s, qx, qy, verdicts, n);
    if (rc != SP_OK) return rc;
    if (tree_status) *tree_status = SP_TREE_NOT_COMMITTED;
    rc = sp_tree_root(tree, old_root);
    if (rc != SP_OK) return rc;
    std::memcpy(new_root, old_root, 32);
    return SP_OK;
  }
  // The verification needs nothing but z: it starts NOW, on a thread of its own, so that its host work (lane, staging
  // copies, key lookup) runs beside the sort below and its launch beside the tree's levels.  (Round 5 spawned it after
  // the sort: 150 us later, and it then queued for the library lock behind the tree's enqueue.)
  // The verifier does its lock-free part at once (lane, staging copies) and then waits at a gate until the tree
  // update has enqueued its levels: the tree is the critical path and both need the library lock.
  struct Gate {
    std::mutex m;
    std::condition_variable cv;
    bool open = false;
    void release() {
      { std::lock_guard<std::mutex> lk(m); open = true; }
      cv.notify_all();
    }
    void wait() {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return open; });
    }
  } gate;
  const std::function<void()> open_gate = [&] { gate.release(); };
  int vrc = SP_OK;
  std::thread verifier([&] {
    tl_mark("verifier thread runs");
    vrc = verify_batch_keyed_gated(z_out, r, s, qx, qy, verdicts, n, [&] { gate.wait(); });
    tl_mark("verifier done");
  });
  tl_mark("verifier spawned");
  struct Joiner {  // every return below opens the gate and joins the verifier first: it reads the caller's arrays
    std::thread& t;
    Gate& g;
    ~Joiner() { g.release(); if (t.joinable()) t.join(); }
  } joiner{verifier, gate};
  // order ids, sorted, with the leaves in the same order.  The ids are bits of hash outputs - uniform - so one
  // counting pass over their top bits leaves buckets of about one id each and a tiny std::sort inside every bucket
  // (any input is still sorted correctly: a skewed one only makes a bucket's sort longer).  120 us -> ~25 us for
  // 4096 orders against std::sort of (id, index) pairs.
  std::vector<std::pair<uint64_t, size_t>> ids(n);
  {
    const unsigned w = id_shift >> 6, sh = id_shift & 63;
    unsigned lg = 4;
    while (lg < 16 && ((size_t)1 << lg) < n) ++lg;
    const size_t nb = (size_t)1 << lg;
    const unsigned id_bits = 64;  // (ids of a tree lower than 64 all fall into bucket 0: one std::sort, still correct)
    std::vector<uint32_t> start(nb + 1, 0);
    std::vector<uint64_t> raw(n);
    for (size_t i = 0; i < n; ++i) {
      const uint64_t* z = z_out + 4 * i;
      uint64_t v = z[w] >> sh;
      if (sh && w + 1 < 4) v |= z[w + 1] << (64 - sh);
      raw[i] = v;
      ++start[(v >> (id_bits - lg)) + 1];
    }
    for (size_t b = 0; b < nb; ++b) start[b + 1] += start[b];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) ids[fill[raw[i] >> (id_bits - lg)]++] = {raw[i], i};
    for (size_t b = 0; b < nb; ++b)
      if (start[b + 1] - start[b] > 1) std::sort(ids.begin() + start[b], ids.begin() + start[b + 1]);
  }
  std::vector<uint64_t> keys(n), sorted_leaves(4 * n);
  for (size_t j = 0; j < n; ++j) {
    if (j > 0 && ids[j].first == ids[j - 1].first) { set_error("sp_order_batch: two orders share an order id"); return SP_ERR_BAD_ARGUMENT; }
    keys[j] = ids[j].first;
    std::memcpy(&sorted_leaves[4 * j], leaves + 4 * ids[j].second, 32);
  }
  tl_mark("ids sorted");
  bool joined = false;
  const std::function<bool()> all_verified = [&]() {
    gate.release();  // (an empty update asks before anything was enqueued)
    verifier.join();
    joined = true;
    if (vrc != SP_OK) return false;
    for (size_t i = 0; i < n; ++i)
      if (verdicts[i] != 1) return false;
    return true;
  };
  {
    TreeScope ts;
    rc = ts.open(tree);
    if (rc == SP_OK)
      rc = tree_update_locked(*ts.t, keys.data(), sorted_leaves.data(), n, old_root, new_root, tree_status, &all_verified,
                              &open_gate);
  }
  gate.release();  // (the tree failed before it enqueued anything)
  if (!joined && verifier.joinable()) verifier.join();
  // the error text is process-wide (set_error), so what the verifier thread reported is what sp_last_error says;
  // when both legs failed the tree's code wins and the text is whichever leg failed last
  if (rc != SP_OK) return rc;
  return vrc;
}


// shared_state_apply_state_updates (services/perpetual/cairo/state/state.cairo:135-186) in ONE call: the previous and
// the new leaf of every touched position (position/hash.cairo:76-131), merkle_multi_update of the positions tree
// (:155-161) and of the orders tree (:167-173), all or nothing across both.  Stages:
//   positions tree's stream   words of all previous chains and of the changed new chains -> work buffer; ONE
//                             enqueue_pedersen_chain_ragged over both halves (it slices above its launch cap);
//                             state_pos_leaf_kernel: current leaf against previous hash, status byte, level 0;
//                             then the update's structure kernels and level launches (tree_enqueue)
//   orders tree's stream      ord_new into level 0, ord_prev beside it; state_ord_leaf_kernel; structure, levels
//   host                      waits for both streams, decides ONCE, launches both insert kernels or neither
// Nothing returns to the host between the stages and no hash crosses PCIe.  Both tree mutexes are held from start to
// end, taken in ascending handle order; the library lock only inside tree_enqueue; no host lane, no thread.
int sp_state_batch(int positions_tree, int orders_tree, const uint64_t* pos_keys, size_t n_pos,
                   const uint64_t* prev_words, const uint32_t* prev_off, const uint64_t* new_words,
                   const uint32_t* new_off, const uint64_t* ord_keys, const uint64_t* ord_prev,
                   const uint64_t* ord_new, size_t n_ord, uint64_t* pos_old_root, uint64_t* pos_new_root,
                   uint64_t* ord_old_root, uint64_t* ord_new_root, uint8_t* pos_status, uint8_t* ord_status,
                   uint8_t* batch_status) {
  SP_REQUIRE_READY();
  if (!batch_status || !pos_old_root || !pos_new_root || !ord_old_root || !ord_new_root) {
    set_error("sp_state_batch: the four roots and batch_status are required");
    return SP_ERR_BAD_ARGUMENT;
  }
  if ((n_pos && (!pos_keys || !prev_words || !prev_off || !new_off)) || (n_ord && (!ord_keys || !ord_prev || !ord_new))) {
    set_error("sp_state_batch: null input array");
    return SP_ERR_BAD_ARGUMENT;
  }
  if (positions_tree == orders_tree) { set_error("sp_state_batch: the same tree handle twice"); return SP_ERR_BAD_ARGUMENT; }
  TimelineScope timeline("sp_state_batch");
  // ---- offsets: the previous chains as sp_pedersen_chains_ragged wants them, the new ones may be empty ----
  size_t n_changed = 0;
  if (n_pos) {
    if (n_pos >= 0x7fffffffull) { set_error("sp_state_batch: too many positions"); return SP_ERR_BAD_ARGUMENT; }
    if (prev_off[0] != 0 || new_off[0] != 0) { set_error("sp_state_batch: off[0] must be 0"); return SP_ERR_BAD_ARGUMENT; }
    for (size_t i = 0; i < n_pos; ++i) {
      if (prev_off[i + 1] <= prev_off[i]) {
        set_error("sp_state_batch: every previous chain needs at least one element");
        return SP_ERR_BAD_ARGUMENT;
      }
      if (new_off[i + 1] < new_off[i]) { set_error("sp_state_batch: decreasing offset"); return SP_ERR_BAD_ARGUMENT; }
      n_changed += new_off[i + 1] != new_off[i];
    }
    if ((uint64_t)prev_off[n_pos] + new_off[n_pos] > 0xffffffffull) {
      set_error("sp_state_batch: more than 2^32 words");
      return SP_ERR_BAD_ARGUMENT;
    }
    if (new_off[n_pos] && !new_words) { set_error("sp_state_batch: null input array"); return SP_ERR_BAD_ARGUMENT; }
  }
  if (n_ord >= 0x7fffffffull) { set_error("sp_state_batch: too many orders"); return SP_ERR_BAD_ARGUMENT; }
  // ---- both trees, locked in ascending handle order whichever role they play ----
  TreeScope first, second;
  const bool pos_first = positions_tree < orders_tree;
  int rc = first.open(pos_first ? positions_tree : orders_tree);
  if (rc != SP_OK) return rc;
  rc = second.open(pos_first ? orders_tree : positions_tree);
  if (rc != SP_OK) return rc;
  SparseTree& P = pos_first ? *first.t : *second.t;
  SparseTree& O = pos_first ? *second.t : *first.t;
  if (P.ctx_index != O.ctx_index) {
    set_error("sp_state_batch: the two trees live on different contexts");
    return SP_ERR_BAD_ARGUMENT;
  }
  if (!keys_ok(P.height, pos_keys, n_pos, true) || !keys_ok(O.height, ord_keys, n_ord, true)) return SP_ERR_BAD_ARGUMENT;
  tl_mark("trees locked, arguments checked");

  // ---- positions: previous chains, then the changed new ones, as one ragged batch ----
  const size_t n_chains = n_pos + n_changed;
  const size_t prev_total = n_pos ? prev_off[n_pos] : 0, new_total = n_pos ? new_off[n_pos] : 0;
  std::vector<uint32_t> chain_off(n_chains + 1, 0), map(n_pos);
  for (size_t i = 0, k = 0; i < n_pos; ++i) {
    chain_off[i + 1] = prev_off[i + 1];
    const bool changed = new_off[i + 1] != new_off[i];
    map[i] = changed ? (uint32_t)k : STATE_UNCHANGED;
    if (changed) chain_off[n_pos + ++k] = (uint32_t)(prev_total + new_off[i + 1]);
  }
  auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
  std::vector<uint8_t> pos_land, ord_land;  // landing of the status bytes when the page-locked buffer is not used
  LeafProducer pp;
  const size_t p_words = (prev_total + new_total) * 32;
  const size_t pd_hash = pad(p_words), pd_map = pd_hash + pad(n_chains * 32), pd_cst = pd_map + pad(n_pos * 4),
               pd_st = pd_cst + pad(n_chains);
  const size_t ph_map = p_words, ph_st = p_words + pad(n_pos * 4);
  pp.dev_bytes = pd_st + pad(n_pos);
  pp.host_bytes = ph_st + n_pos;
  const uint8_t* pos_bytes = nullptr;
  pp.stage = [&](char* dev, char* host, hipStream_t st) -> int {
    if (host) {
      std::memcpy(host, prev_words, prev_total * 32);
      if (new_total) std::memcpy(host + prev_total * 32, new_words, new_total * 32);
      std::memcpy(host + ph_map, map.data(), n_pos * 4);
      SP_HIP(hipMemcpyAsync(dev, host, p_words, hipMemcpyHostToDevice, st));
      SP_HIP(hipMemcpyAsync(dev + pd_map, host + ph_map, n_pos * 4, hipMemcpyHostToDevice, st));
    } else {
      SP_HIP(hipMemcpyAsync(dev, prev_words, prev_total * 32, hipMemcpyHostToDevice, st));
      if (new_total) SP_HIP(hipMemcpyAsync(dev + prev_total * 32, new_words, new_total * 32, hipMemcpyHostToDevice, st));
      SP_HIP(hipMemcpyAsync(dev + pd_map, map.data(), n_pos * 4, hipMemcpyHostToDevice, st));
    }
    return enqueue_pedersen_chain_ragged((const uint64_t*)dev, chain_off.data(), n_chains, (uint64_t*)(dev + pd_hash),
                                         (uint8_t*)(dev + pd_cst), st);
  };
  pp.place = [&](char* dev, char* host, const TreeSlot* tab, uint64_t mask, const uint64_t* d_keys, const uint64_t* d_empty,
                 uint64_t* d_level0, unsigned* flag, hipStream_t st) -> int {
    hipLaunchKernelGGL(state_pos_leaf_kernel, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, st, tab, mask, d_keys,
                       (unsigned)n_pos, d_empty, (const uint64_t*)(dev + pd_hash), (const uint8_t*)(dev + pd_cst),
                       (const uint32_t*)(dev + pd_map), d_level0, (uint8_t*)(dev + pd_st), flag);
    SP_HIP(hipGetLastError());
    uint8_t* land = host ? (uint8_t*)(host + ph_st) : (pos_land.resize(n_pos), pos_land.data());
    pos_bytes = land;
    SP_HIP(hipMemcpyAsync(land, dev + pd_st, n_pos, hipMemcpyDeviceToHost, st));
    return SP_OK;
  };
  // ---- orders: the new leaves go to level 0 with the update's inputs, the previous ones beside them ----
  LeafProducer op;
  const size_t od_st = pad(n_ord * 32);
  op.dev_bytes = od_st + pad(n_ord);
  op.host_bytes = n_ord * 32 + n_ord;
  const uint8_t* ord_bytes = nullptr;
  op.stage = [&](char* dev, char* host, hipStream_t st) -> int {
    if (host) std::memcpy(host, ord_prev, n_ord * 32);
    SP_HIP(hipMemcpyAsync(dev, host ? (const void*)host : (const void*)ord_prev, n_ord * 32, hipMemcpyHostToDevice, st));
    return SP_OK;
  };
  op.place = [&](char* dev, char* host, const TreeSlot* tab, uint64_t mask, const uint64_t* d_keys, const uint64_t* d_empty,
                 uint64_t* d_level0, unsigned* flag, hipStream_t st) -> int {
    hipLaunchKernelGGL(state_ord_leaf_kernel, dim3((unsigned)((n_ord + 255) / 256)), dim3(256), 0, st, tab, mask, d_keys,
                       (unsigned)n_ord, d_empty, (const uint64_t*)dev, d_level0, (uint8_t*)(dev + od_st), flag);
    SP_HIP(hipGetLastError());
    uint8_t* land = host ? (uint8_t*)(host + n_ord * 32) : (ord_land.resize(n_ord), ord_land.data());
    ord_bytes = land;
    SP_HIP(hipMemcpyAsync(land, dev + od_st, n_ord, hipMemcpyDeviceToHost, st));
    return SP_OK;
  };

  // ---- enqueue both (each tree on its own stream: the two level sequences run side by side), wait for both ----
  TreePending pend_p, pend_o;
  uint64_t p_old[4], o_old[4];
  rc = tree_enqueue(P, pos_keys, nullptr, n_pos, p_old, nullptr, &pp, pend_p);
  tl_mark("positions enqueued");
  int rc2 = SP_OK;
  if (rc == SP_OK) {
    rc2 = tree_enqueue(O, ord_keys, ord_new, n_ord, o_old, nullptr, &op, pend_o);
    tl_mark("orders enqueued");
  }
  if (rc != SP_OK || rc2 != SP_OK) {  // whatever did get onto a stream reads this call's buffers: drain it
    if (P.stream) (void)hipStreamSynchronize(P.stream);
    if (O.stream) (void)hipStreamSynchronize(O.stream);
    return rc != SP_OK ? rc : rc2;
  }
  unsigned flag_p = 0, flag_o = 0;
  rc = tree_wait(P, pend_p, &flag_p);
  rc2 = tree_wait(O, pend_o, &flag_o);
  if (rc != SP_OK || rc2 != SP_OK) {
    if (O.stream) (void)hipStreamSynchronize(O.stream);
    return rc != SP_OK ? rc : rc2;
  }
  tl_mark("both trees hashed");
  // ---- decide once: the item status bytes are in the flags already (the leaf kernels raise what they write) ----
  const unsigned bad = flag_p | flag_o;
  uint64_t p_new[4], o_new[4];
  std::memcpy(p_new, p_old, 32);
  std::memcpy(o_new, o_old, 32);
  if (bad == 0) {
    if (pend_p.queued) rc = tree_commit(P, pend_p, p_new);
    if (rc == SP_OK && pend_o.queued) rc = tree_commit(O, pend_o, o_new);
    if (rc != SP_OK) return rc;
    tl_mark("both trees committed");
  }
  if (pos_status && n_pos) std::memcpy(pos_status, pos_bytes, n_pos);
  if (ord_status && n_ord) std::memcpy(ord_status, ord_bytes, n_ord);
  std::memcpy(pos_old_root, p_old, 32);
  std::memcpy(pos_new_root, p_new, 32);
  std::memcpy(ord_old_root, o_old, 32);
  std::memcpy(ord_new_root, o_new, 32);
  *batch_status = bad ? (uint8_t)(SP_TREE_NOT_COMMITTED | (bad & 0x7f)) : 0;
  return SP_OK;
}

}  // extern "C"
