// Opening committed tables (sp_commit_open[_dev], sp_commit_open_size): the index and plan logic that the kernel of
// commit_open.hip and the host share - argument validation, the offset of level l in a leaves-first levels buffer,
// the sibling index, the two offset arrays, the slice plan and the gather of one opening.  Nothing here needs HIP: a
// plain C++ compiler builds it for the CPU tests (tests/host/commit_open_shim.cpp), which run the same gather over
// host arrays.
//
// A table is what sp_commit_rows_dev committed: n_rows (a power of two) x n_cols felts stored column-major, column c
// starting c * col_stride felts in, and the 2 n_rows - 1 felts of its levels buffer, leaves first and root last.
// Opening (t, r) copies 1 + n_cols + log2(n_rows) felts, its SLOTS, each from an address that follows from (t, r) and
// the slot number alone - no slot waits for another:
//   slot c < n_cols          value of row r in column c      cols[c col_stride + r]           -> values + 4 (val_off[i] + c)
//   slot n_cols              the row's leaf                  levels[r]                        -> leaves + 4 i (if wanted)
//   slot n_cols + 1 + l      sibling at level l < height     levels[base_l + ((r >> l) ^ 1)]  -> siblings + 4 (off[i] + l)
// with base_l = 2 n_rows - (2 n_rows >> l): levels 0 .. l - 1 hold n_rows + n_rows / 2 + ... = 2 n_rows (1 - 2^-l)
// felts.  All of it is 64-bit arithmetic: n_rows may be 2^32 (a levels buffer of 2^33 felts).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef SP_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SP_HD __host__ __device__ __forceinline__
#else
#define SP_HD inline
#endif
#endif

namespace sp {

// ---- the launch plan ----
// One wave per opening (its lanes take the slots 64 at a time), four openings per block of 256 threads.  One launch
// takes up to OPEN_SLICE_MAX openings - the largest class; a call above it goes out as consecutive slices.
constexpr unsigned OPEN_TPB = 256;
constexpr unsigned OPEN_LANES = 64;
constexpr unsigned OPEN_PER_BLOCK = OPEN_TPB / OPEN_LANES;
constexpr size_t OPEN_SLICE_MAX = (size_t)1 << 16;
constexpr uint64_t OPEN_MAX_ROWS = (uint64_t)1 << 32;
constexpr uint64_t OPEN_MAX_FELTS = 0xffffffffull;  // of values and of siblings: the offsets are 32-bit

SP_HD size_t open_slice_count(size_t n_open) { return (n_open + OPEN_SLICE_MAX - 1) / OPEN_SLICE_MAX; }
// slice k of a call: openings first .. first + count
SP_HD void open_slice(size_t n_open, size_t k, size_t* first, size_t* count) {
  *first = k * OPEN_SLICE_MAX;
  *count = n_open - *first < OPEN_SLICE_MAX ? n_open - *first : OPEN_SLICE_MAX;
}
SP_HD unsigned open_blocks(size_t count) { return (unsigned)((count + OPEN_PER_BLOCK - 1) / OPEN_PER_BLOCK); }

// ---- one table, as the kernel reads it ----
struct OpenTable {
  const uint64_t* cols;
  const uint64_t* levels;
  uint64_t col_stride, n_rows, n_cols;
  uint32_t height, pad;
};

SP_HD unsigned open_height(uint64_t n_rows) {  // n_rows a power of two
  unsigned h = 0;
  while (((uint64_t)1 << h) < n_rows) ++h;
  return h;
}
SP_HD uint64_t open_level_base(uint64_t n_rows, unsigned l) { return 2 * n_rows - ((2 * n_rows) >> l); }
SP_HD uint64_t open_sibling_index(uint64_t n_rows, uint64_t r, unsigned l) {
  return open_level_base(n_rows, l) + ((r >> l) ^ 1);
}
SP_HD uint64_t open_value_index(uint64_t col_stride, uint64_t r, uint64_t c) { return c * col_stride + r; }
SP_HD uint64_t open_slots(const OpenTable& t) { return t.n_cols + 1 + t.height; }

// ---- validation: nullptr, or the text for sp_last_error (it names the argument) ----
// The shapes, which is all sp_commit_open_size has: every table's n_rows and n_cols, every table_of[i]; the felt
// totals of the values and the siblings, each at most 2^32 - 1.
SP_HD const char* open_check_shapes(size_t n_tables, const size_t* n_rows, const size_t* n_cols, size_t n_open,
                                    const uint32_t* table_of, uint64_t* n_values, uint64_t* n_siblings) {
  if (n_tables == 0 && n_open > 0) return "n_tables is 0 with openings to answer";
  if (n_tables > 0 && (n_rows == nullptr || n_cols == nullptr)) return "n_rows and n_cols must not be NULL";
  if (n_open > 0 && table_of == nullptr) return "table_of must not be NULL";
  for (size_t t = 0; t < n_tables; ++t) {
    const uint64_t n = n_rows[t];
    if (n == 0 || (n & (n - 1)) != 0 || n > OPEN_MAX_ROWS) return "n_rows must be a power of two, 1 .. 2^32";
    if (n_cols[t] == 0) return "n_cols must be at least 1";
  }
  uint64_t nv = 0, ns = 0;
  for (size_t i = 0; i < n_open; ++i) {
    const uint32_t t = table_of[i];
    if (t >= n_tables) return "table_of names a table >= n_tables";
    if ((uint64_t)n_cols[t] > OPEN_MAX_FELTS - nv) return "more than 2^32 - 1 value felts (n_cols over table_of)";
    nv += n_cols[t];
    ns += open_height(n_rows[t]);
    if (ns > OPEN_MAX_FELTS) return "more than 2^32 - 1 sibling felts (n_rows over table_of)";
  }
  if (n_values) *n_values = nv;
  if (n_siblings) *n_siblings = ns;
  return nullptr;
}
// The rest of a call's inputs, after the shapes: table pointers, strides, rows.
SP_HD const char* open_check_tables(size_t n_tables, const void* const* cols, const size_t* col_stride,
                                    const size_t* n_rows, const size_t* n_cols, const void* const* levels, size_t n_open,
                                    const uint32_t* table_of, const uint64_t* rows) {
  if (n_tables > 0 && (cols == nullptr || levels == nullptr || col_stride == nullptr)) {
    return "cols, col_stride and levels must not be NULL";
  }
  if (n_open > 0 && rows == nullptr) return "rows must not be NULL";
  for (size_t t = 0; t < n_tables; ++t) {
    if (cols[t] == nullptr) return "cols holds a NULL table pointer";
    if (levels[t] == nullptr) return "levels holds a NULL table pointer";
    if (col_stride[t] < n_rows[t]) return "col_stride is below n_rows";
    // the last felt of the table must have a 64-bit byte address
    if ((uint64_t)col_stride[t] > ((~(uint64_t)0 >> 6) / (uint64_t)n_cols[t])) return "col_stride times n_cols overflows";
  }
  for (size_t i = 0; i < n_open; ++i) {
    if (rows[i] >= (uint64_t)n_rows[table_of[i]]) return "rows holds a row >= n_rows of its table";
  }
  return nullptr;
}

// The outputs a call of these totals needs: both offset arrays always, values and siblings when they receive a felt.
SP_HD const char* open_check_outputs(const void* values, const void* val_off, const void* siblings, const void* off,
                                     uint64_t n_values, uint64_t n_siblings) {
  if (val_off == nullptr || off == nullptr) return "val_off and off must not be NULL";
  if (n_values > 0 && values == nullptr) return "values must not be NULL";
  if (n_siblings > 0 && siblings == nullptr) return "siblings must not be NULL";
  return nullptr;
}

// The two offset arrays of validated shapes, n_open + 1 entries each, in felts.
SP_HD void open_offsets(const size_t* n_rows, const size_t* n_cols, size_t n_open, const uint32_t* table_of,
                        uint32_t* val_off, uint32_t* off) {
  val_off[0] = off[0] = 0;
  for (size_t i = 0; i < n_open; ++i) {
    val_off[i + 1] = val_off[i] + (uint32_t)n_cols[table_of[i]];
    off[i + 1] = off[i] + open_height(n_rows[table_of[i]]);
  }
}

// ---- the gather ----
// A felt moves as two 128-bit words.
SP_HD void open_copy_felt(uint64_t* dst, const uint64_t* src) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4 a = s[0], b = s[1];
  d[0] = a;
  d[1] = b;
#else
  memcpy(dst, src, 32);
#endif
}
// The slots lane, lane + lanes, ... of opening i (the kernel: lane of 64; the host: 0 of 1).  val_off and off are the
// call's offset arrays (absolute, also for a slice); leaves may be null.
SP_HD void open_gather(const OpenTable* tables, const uint32_t* table_of, const uint64_t* rows, const uint32_t* val_off,
                       const uint32_t* off, size_t i, unsigned lane, unsigned lanes, uint64_t* values, uint64_t* leaves,
                       uint64_t* siblings) {
  const OpenTable t = tables[table_of[i]];
  const uint64_t r = rows[i];
  const uint64_t slots = open_slots(t);
  for (uint64_t s = lane; s < slots; s += lanes) {
    const uint64_t* src;
    uint64_t* dst;
    if (s < t.n_cols) {
      src = t.cols + 4 * open_value_index(t.col_stride, r, s);
      dst = values + 4 * ((uint64_t)val_off[i] + s);
    } else if (s == t.n_cols) {
      if (leaves == nullptr) continue;
      src = t.levels + 4 * r;
      dst = leaves + 4 * (uint64_t)i;
    } else {
      const unsigned l = (unsigned)(s - t.n_cols - 1);
      src = t.levels + 4 * open_sibling_index(t.n_rows, r, l);
      dst = siblings + 4 * ((uint64_t)off[i] + l);
    }
    open_copy_felt(dst, src);
  }
}

}  // namespace sp
