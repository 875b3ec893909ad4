// What pedersen.hip offers the other translation units of the library (merkle.hip): the per-stream scratch and
// page-locked staging copy, the level and walk launchers.  One definition of every struct that crosses the boundary - PathLevels is passed BY VALUE into a
// kernel, so two hand-kept copies of it would be an ODR hazard nothing checks.
#pragma once
#include "context.hpp"

namespace sp {

struct Scratch {
  int32_t *X, *ZZ, *Pre;
  unsigned* flag;
};
// The stream's scratch planes for n hashes (grown on demand) and its status flag.
int get_scratch_public(size_t n, Scratch& s, hipStream_t st);

// The host `pieces`, one behind the other -> dev: memcpy into the stream's page-locked buffer, then one asynchronous
// copy.  The buffer is guarded by an event that marks the last copy out of it, so the pieces are consumed when this
// returns; calls on one stream share buffer and event.  The caller holds the context lock.
int stage_copy(std::initializer_list<Piece> pieces, void* dev, hipStream_t st);

// Enqueue n hashes; x/y/out strides in felts.  `flag` (device, may be null) ORs item status.
int enqueue_pedersen(const uint64_t* x, size_t xs, const uint64_t* y, size_t ys, uint64_t* out,
                     size_t os, uint8_t* status, unsigned* flag, size_t n, hipStream_t st,
                     const Scratch& s, const int2* src);
// A level of a sparse multi-update (gathered mode, src != null): `cpts` = the level's two constant points
// (enqueue_partial_points) or null.  Levels that fit the quad kernels take the SPARSE variant.
int enqueue_pedersen_sparse(const uint64_t* x, const uint64_t* y, uint64_t* out, unsigned* flag, size_t n,
                            hipStream_t st, const Scratch& s, const int2* src, const aff_packed* cpts);
// The constant points of a sparse tree's levels (ped_partial_kernel): out[2 l], out[2 l + 1] for felts[l].
// Returns SP_OK with *usable = false when the plan leaves no constant window on one of the sides.
int enqueue_partial_points(const uint64_t* felts, int count, aff_packed* out, hipStream_t st, bool* usable);

// ped_path_kernel's levels: val_base / src_off are merkle.hip's TreeLevels fields; level `first` is the children's
// level of the first hash.
struct PathLevels {
  int first, n_levels;
  int val_base[66];
  unsigned src_off[66];
};
// pl.n_levels consecutive levels of a sparse multi-update with n nodes each and no merging paths, as one launch
// (ped_path_kernel).  *done = false when the levels are not of a size class the quad kernels serve (or the switch is
// off): the caller then enqueues them one by one.  cpts_tree: the tree's constant points ([2 l], [2 l + 1]) or null.
int enqueue_pedersen_path(uint64_t* felts, const uint64_t* emp, unsigned* flag, size_t n, hipStream_t st,
                          const int2* src_all, const PathLevels& pl, const aff_packed* cpts_tree, bool* done);

// n ragged walks (ped_fold_ragged_kernel), chains and Merkle paths alike; `off` (n + 1) and `keys` (n, or null) are
// validated HOST arrays, everything else lives on the device.  Enqueues on `st` and returns; the caller holds the
// context lock.
//   keys == null  chains: chain i = felts off[i] .. off[i + 1) of `words`, folded from the left (at least one word
//                 each); `leaves`, `expect` and `verdict` are null
//   keys != null  paths: path i starts from leaves + 4 i and takes the siblings off[i] .. off[i + 1) of `words`, bit j
//                 of keys[i] = the side at step j; expect (+ 4 i estride, estride 0 or 1) and verdict (n bytes): both
//                 or neither
// out = n felts, status = n bytes or null.
int enqueue_pedersen_fold_ragged(const uint64_t* leaves, const uint64_t* words, const uint32_t* off, const uint64_t* keys,
                                 size_t n, uint64_t* out, uint8_t* status, const uint64_t* expect, size_t estride,
                                 uint8_t* verdict, hipStream_t st);
inline int enqueue_pedersen_chain_ragged(const uint64_t* elems, const uint32_t* off, size_t n, uint64_t* out,
                                         uint8_t* status, hipStream_t st) {
  return enqueue_pedersen_fold_ragged(nullptr, elems, off, nullptr, n, out, status, nullptr, 0, nullptr, st);
}

}  // namespace sp
