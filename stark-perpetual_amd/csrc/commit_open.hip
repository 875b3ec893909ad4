// Opening committed tables: every opened row and every Merkle sibling of a proof's query phase read out of the
// tables sp_commit_rows_dev committed, by ONE launch (include/starkperp.h "Opening committed tables").
//
// The index arithmetic, the validation and the slice plan are csrc/commit_open.hpp, shared with the host tests.  The
// kernel is a gather: one wave per opening, lane j copies slot j (a value, the leaf or a sibling - 32 bytes as two
// 128-bit loads and two 128-bit stores) from an address it computes from (table, row, j) alone, so no load waits for
// another and a launch lasts about one trip to HBM.  The wave's opening number is made wave-uniform, so the table
// descriptor, the row and the two offsets come through the scalar cache.
#include <map>
#include <vector>

#include "context.hpp"
#include "pedersen.hpp"
#include "commit_open.hpp"

namespace sp {

__global__ void __launch_bounds__(OPEN_TPB)
commit_open_kernel(const OpenTable* __restrict__ tables, const uint32_t* __restrict__ table_of,
                   const uint64_t* __restrict__ rows, const uint32_t* __restrict__ val_off,
                   const uint32_t* __restrict__ off, size_t first, size_t count, uint64_t* __restrict__ values,
                   uint64_t* __restrict__ leaves, uint64_t* __restrict__ siblings) {
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x / OPEN_LANES);
  const size_t k = (size_t)blockIdx.x * OPEN_PER_BLOCK + wave;
  if (k >= count) return;
  open_gather(tables, table_of, rows, val_off, off, first + k, threadIdx.x % OPEN_LANES, OPEN_LANES, values, leaves,
              siblings);
}

// The call's metadata on the device, per stream: table descriptors | rows | table_of | val_off | off.  Grown on demand
// (a growth frees the old allocation, which waits for the device), released by sp_shutdown.
static std::map<StreamKey, DeviceBuffer> g_open_meta;
void release_commit_open_state() {
  for (auto& kv : g_open_meta) kv.second.release();
  g_open_meta.clear();
}

struct OpenArgs {
  size_t n_tables;
  const void* const* cols;
  const size_t* col_stride;
  const size_t* n_rows;
  const size_t* n_cols;
  const void* const* levels;
  size_t n_open;
  const uint32_t* table_of;
  const uint64_t* rows;
};

// Everything that can be wrong with a call, before anything is written; the felt totals on the way.
static int open_validate(const char* who, const OpenArgs& a, const void* values, const uint32_t* val_off,
                         const void* siblings, const uint32_t* off, uint64_t* n_values, uint64_t* n_siblings) {
  const char* bad = open_check_shapes(a.n_tables, a.n_rows, a.n_cols, a.n_open, a.table_of, n_values, n_siblings);
  if (!bad) bad = open_check_tables(a.n_tables, a.cols, a.col_stride, a.n_rows, a.n_cols, a.levels, a.n_open, a.table_of, a.rows);
  if (!bad) bad = open_check_outputs(values, val_off, siblings, off, *n_values, *n_siblings);
  if (bad) {
    set_error(std::string(who) + ": " + bad);
    return SP_ERR_BAD_ARGUMENT;
  }
  return SP_OK;
}

// Validated arguments, filled offsets, device outputs: the metadata goes over in one staged copy, then one launch
// per slice.  The caller holds the context lock.
static int enqueue_open(const OpenArgs& a, const uint32_t* val_off, const uint32_t* off, uint64_t* values,
                        uint64_t* leaves, uint64_t* siblings, hipStream_t st) {
  const size_t n = a.n_open;
  std::vector<OpenTable> tabs(a.n_tables);
  for (size_t t = 0; t < a.n_tables; ++t) {
    tabs[t] = OpenTable{(const uint64_t*)a.cols[t], (const uint64_t*)a.levels[t], a.col_stride[t], a.n_rows[t],
                        a.n_cols[t], open_height(a.n_rows[t]), 0};
  }
  const size_t tab_bytes = a.n_tables * sizeof(OpenTable), row_bytes = n * sizeof(uint64_t);
  const size_t tof_bytes = n * sizeof(uint32_t), off_bytes = (n + 1) * sizeof(uint32_t);
  DeviceBuffer& meta = g_open_meta[stream_key(st)];
  SP_HIP(meta.reserve(tab_bytes + row_bytes + tof_bytes + 2 * off_bytes));
  char* m = (char*)meta.ptr;
  const OpenTable* d_tabs = (const OpenTable*)m;
  const uint64_t* d_rows = (const uint64_t*)(m + tab_bytes);
  const uint32_t* d_tof = (const uint32_t*)(m + tab_bytes + row_bytes);
  const uint32_t* d_voff = (const uint32_t*)(m + tab_bytes + row_bytes + tof_bytes);
  const uint32_t* d_off = (const uint32_t*)(m + tab_bytes + row_bytes + tof_bytes + off_bytes);
  const int rc = stage_copy({{tabs.data(), tab_bytes}, {a.rows, row_bytes}, {a.table_of, tof_bytes}, {val_off, off_bytes},
                             {off, off_bytes}}, m, st);
  if (rc != SP_OK) return rc;
  for (size_t k = 0; k < open_slice_count(n); ++k) {
    size_t first, count;
    open_slice(n, k, &first, &count);
    const bool prof = profile_launch_begin(st);
    hipLaunchKernelGGL(commit_open_kernel, dim3(open_blocks(count)), dim3(OPEN_TPB), 0, st, d_tabs, d_tof, d_rows, d_voff,
                       d_off, first, count, values, leaves, siblings);
    if (prof) profile_launch_end(st, count);
    SP_HIP(hipGetLastError());
  }
  return SP_OK;
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_commit_open_size(size_t n_tables, const size_t* n_rows, const size_t* n_cols, size_t n_open,
                        const uint32_t* table_of, size_t* n_values, size_t* n_siblings) {
  uint64_t nv = 0, ns = 0;
  const char* bad = open_check_shapes(n_tables, n_rows, n_cols, n_open, table_of, &nv, &ns);
  if (!bad && (n_values == nullptr || n_siblings == nullptr)) bad = "n_values and n_siblings must not be NULL";
  if (bad) {
    set_error(std::string("sp_commit_open_size: ") + bad);
    return SP_ERR_BAD_ARGUMENT;
  }
  *n_values = (size_t)nv;
  *n_siblings = (size_t)ns;
  return SP_OK;
}

int sp_commit_open_dev(size_t n_tables, const void* const* cols, const size_t* col_stride, const size_t* n_rows,
                       const size_t* n_cols, const void* const* levels, size_t n_open, const uint32_t* table_of,
                       const uint64_t* rows, uint64_t* values, uint32_t* val_off, uint64_t* leaves, uint64_t* siblings,
                       uint32_t* off, void* stream) {
  CtxByPointer sp_ctx_sel__(n_tables && cols ? cols[0] : nullptr);  // the context of the device the tables live on
  SP_REQUIRE_READY();
  const OpenArgs a{n_tables, cols, col_stride, n_rows, n_cols, levels, n_open, table_of, rows};
  uint64_t nv = 0, ns = 0;
  const int rc = open_validate("sp_commit_open_dev", a, values, val_off, siblings, off, &nv, &ns);
  if (rc != SP_OK) return rc;
  open_offsets(n_rows, n_cols, n_open, table_of, val_off, off);
  if (n_open == 0) return SP_OK;
  ctx_lock lk(ctx().mu);
  return enqueue_open(a, val_off, off, values, leaves, siblings, (hipStream_t)stream);
}

// Host outputs, on a host lane of the tables' context: values | leaves | siblings are written side by side on the
// device and come back in one copy (context.hpp StagedTrip; above PINNED_STAGE_MAX one direct copy per array).
int sp_commit_open(size_t n_tables, const void* const* cols, const size_t* col_stride, const size_t* n_rows,
                   const size_t* n_cols, const void* const* levels, size_t n_open, const uint32_t* table_of,
                   const uint64_t* rows, uint64_t* values, uint32_t* val_off, uint64_t* leaves, uint64_t* siblings,
                   uint32_t* off) {
  CtxByPointer sp_ctx_sel__(n_tables && cols ? cols[0] : nullptr);
  LaneScope ls(ctx_current());
  SP_REQUIRE_READY();
  const OpenArgs a{n_tables, cols, col_stride, n_rows, n_cols, levels, n_open, table_of, rows};
  uint64_t nv = 0, ns = 0;
  int rc = open_validate("sp_commit_open", a, values, val_off, siblings, off, &nv, &ns);
  if (rc != SP_OK) return rc;
  open_offsets(n_rows, n_cols, n_open, table_of, val_off, off);
  if (n_open == 0) return SP_OK;
  if (ls.open() != SP_OK) return SP_ERR_HIP;
  HostLane& L = *ls.lane;
  const size_t val_bytes = nv * 32, leaf_bytes = n_open * 32, sib_bytes = ns * 32;
  SP_HIP(L.io.reserve(val_bytes + leaf_bytes + sib_bytes + 64));
  uint64_t* d_values = (uint64_t*)L.io.ptr;
  uint64_t* d_leaves = d_values + 4 * nv;
  uint64_t* d_sib = d_leaves + 4 * n_open;
  StagedTrip trip(L.hio, val_bytes + leaf_bytes + sib_bytes, L.stream);
  {
    ctx_lock lk(ctx().mu);
    rc = enqueue_open(a, val_off, off, d_values, leaves ? d_leaves : nullptr, d_sib, L.stream);
  }
  if (rc != SP_OK) return rc;
  const std::initializer_list<Piece> outs = {Piece(values, val_bytes), Piece(leaves, leaf_bytes), Piece(siblings, sib_bytes)};
  SP_HIP(trip.down(d_values, outs));
  SP_HIP(hipStreamSynchronize(L.stream));
  trip.finish(outs);
  return SP_OK;
}

}  // extern "C"
