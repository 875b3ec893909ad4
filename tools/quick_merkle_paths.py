#!/usr/bin/env python3
"""Verifying inclusion proofs beside the API that had to do it before: 4096 proofs of height 64 from sp_tree_prove, on
a tree that holds those 4096 leaves; on the same inputs, in one process,
  (a) sp_merkle_verify_paths, host-inclusive (8.5 MB of leaves and siblings up, 4096 verdict and 4096 status bytes
      back): median and p90 of the calls after a warm-up;
  (b) the device part alone: sp_merkle_fold_paths_dev on resident tensors, between a pair of events;
  (c) the yardstick: the same fold through sp_pedersen_batch_dev, one launch per level (64), the side chosen by a
      tensor `where` - what a caller could do before this call existed - between a pair of events.
Every root of (a), (b) and (c) is checked against sp_tree_root before anything is timed.
    python tools/quick_merkle_paths.py [calls=24] [output file]"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-perpetual_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import workloads as wl  # noqa: E402
from starkperp import _lib, batch_np, state  # noqa: E402
from evidence_stamp import lib_hash  # noqa: E402

CALLS = max(8, int(sys.argv[1])) if len(sys.argv) > 1 else 24
WARMUP = 4
N, HEIGHT = 4096, 64


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def stats(ms):
    ms = np.array(ms[WARMUP:])
    return float(np.median(ms)), float(np.percentile(ms, 90))


def main():
    import torch
    rng = np.random.default_rng(17)
    keys = np.unique(rng.integers(0, 2**64, size=N + 64, dtype=np.uint64))[:N]  # sorted, distinct
    assert keys.shape == (N,)
    lib = _lib.ensure_init()
    tree = state.LibrarySparseTree(HEIGHT, 0)
    tree.update_arrays(keys, batch_np.felts_from_ints(wl.leaves(N, seed=700)))
    leaves, siblings = batch_np.tree_prove(tree, keys)
    root = batch_np.felts_from_ints([tree.root])
    verdict, status = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    rounds = WARMUP + CALLS

    def verify():
        _lib.check(lib.sp_merkle_verify_paths(ptr(leaves), ptr(siblings), None, HEIGHT, ptr(keys), N, ptr(root), 1,
                                              ptr(verdict), ptr(status)), "sp_merkle_verify_paths")

    verify()
    assert (verdict == 1).all() and not status.any(), "a proof of sp_tree_prove does not verify"

    # resident tensors for (b) and (c)
    stream = torch.cuda.current_stream().cuda_stream
    d_leaves = torch.from_numpy(leaves.view(np.int64)).cuda()
    d_sib = torch.from_numpy(siblings.view(np.int64)).cuda()  # [N, 64, 4]
    d_roots = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    d_root = torch.from_numpy(root.view(np.int64)).cuda()

    def fold_dev():
        _lib.check(lib.sp_merkle_fold_paths_dev(d_leaves.data_ptr(), d_sib.data_ptr(), None, HEIGHT, ptr(keys), N,
                                                d_roots.data_ptr(), None, stream), "sp_merkle_fold_paths_dev")

    d_level = [d_sib[:, l, :].contiguous() for l in range(HEIGHT)]  # level-major copies, outside the timing
    bits = torch.from_numpy(((keys[:, None] >> np.arange(HEIGHT, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)).cuda()
    d_bit = [bits[:, l:l + 1].contiguous() for l in range(HEIGHT)]
    d_node = torch.zeros((N, 4), dtype=torch.int64, device="cuda")

    def per_level():
        node = d_leaves
        for l in range(HEIGHT):
            left = torch.where(d_bit[l], d_level[l], node)
            right = torch.where(d_bit[l], node, d_level[l])
            _lib.check(lib.sp_pedersen_batch_dev(left.data_ptr(), right.data_ptr(), d_node.data_ptr(), None, N, stream),
                       "sp_pedersen_batch_dev")
            node = d_node
        return node

    fold_dev()
    torch.cuda.synchronize()
    assert (d_roots == d_root).all().item(), "sp_merkle_fold_paths_dev does not fold to the root"
    assert (per_level() == d_root).all().item(), "the per-level fold does not reach the root"

    def event_timed(fn):
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return stats(ms)

    a = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        verify()
        a.append(1e3 * (time.perf_counter() - t0))
    a = stats(a)
    b = event_timed(fold_dev)
    c = event_timed(per_level)
    up_bytes = (N + N * HEIGHT) * 32
    lines = [
        "tools/quick_merkle_paths.py: %d proofs of height %d from sp_tree_prove; median / p90 of %d calls after %d, "
        "window bits %d" % (N, HEIGHT, CALLS, WARMUP, lib.sp_window_bits()),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "(a) sp_merkle_verify_paths, host-inclusive (%.1f MB up, %d verdict + %d status bytes back)  %8.3f ms   p90 %8.3f ms" % (
            (up_bytes / 1e6, N, N) + a),
        "(b) sp_merkle_fold_paths_dev on resident tensors, event pair               %8.3f ms   p90 %8.3f ms" % b,
        "    per dependent hash: %.2f us over %d levels" % (1e3 * b[0] / HEIGHT, HEIGHT),
        "(c) %d x sp_pedersen_batch_dev, side chosen by a tensor where, event pair  %8.3f ms   p90 %8.3f ms" % (
            (HEIGHT,) + c),
        "    per level: %.2f us" % (1e3 * c[0] / HEIGHT),
        "b / c = %.3f    (a) - (b) = %.3f ms of upload, copy back and host work" % (b[0] / c[0], a[0] - b[0]),
    ]
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "merkle_paths.txt")
    with open(out, "w") as f:
        f.write(text + "\n")
    assert b[0] < c[0], "the fused fold is not faster than one launch per level"


if __name__ == "__main__":
    main()
