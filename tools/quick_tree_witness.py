#!/usr/bin/env python3
"""Witness export beside the update it describes, host-inclusive, NumPy inputs prepacked outside the timing: a
height-64 tree that already holds 4096 leaves; per round, on the same 4096 keys,
  (a) one sp_tree_update (new leaves every round);
  (b) one sp_tree_witness (about 2 x 10^5 records of 105 bytes back to the host);
  (c) one sp_tree_prove (4096 x 64 siblings);
  (d) the host arithmetic alone: sp_tree_witness_size.
Median and p90 of the calls after a warm-up.  The device part of (b) and (c) - upload of the keys and the kernels,
without the copy back - comes from a child process that runs three calls of each with STARKPERP_TIMELINE=1 (the library
then waits once more, between the kernels and the copy back, and prints its host-side marks).
The first witness is checked before anything is timed: its last record is the root, and a sample of its records hashes
(starkperp.batch_np.pedersen_hash_many).
    python tools/quick_tree_witness.py [calls=24] [output file]"""
import ctypes
import os
import re
import subprocess
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

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--timeline"
CALLS = 3 if CHILD else (max(8, int(sys.argv[1])) if len(sys.argv) > 1 else 24)
WARMUP = 0 if CHILD else 4
N = 4096


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def tree_update(tree, keys, leaves):
    roots, st = np.zeros((2, 4), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.load().sp_tree_update(tree._handle, ptr(keys), ptr(leaves), keys.shape[0], ptr(roots[0:1]),
                                          ptr(roots[1:2]), ptr(st)), "sp_tree_update")
    assert st[0] == 0
    return roots


def timed(fn, rounds):
    t = []
    for r in range(rounds):
        t0 = time.perf_counter()
        fn(r)
        t.append(time.perf_counter() - t0)
    t = 1e3 * np.array(t[WARMUP:])
    return float(np.median(t)), float(np.percentile(t, 90))


def device_parts():
    """Child run: {call: median us between 'work buffer ready' and 'kernels done'} from the timeline lines."""
    env = dict(os.environ, STARKPERP_TIMELINE="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--timeline"], env=env, capture_output=True,
                         text=True, timeout=300)
    if out.returncode != 0:
        raise RuntimeError("timeline child failed: %s" % out.stderr[-2000:])
    spans = {"sp_tree_witness": [], "sp_tree_prove": []}
    for line in out.stderr.splitlines():
        m = re.match(r"libstarkperp timeline (sp_tree_witness|sp_tree_prove):(.*)", line)
        if not m:
            continue
        marks = {name.split(" [")[0].strip(): float(us) for us, name in re.findall(r"([\d.]+) us ([^;]+);", m.group(2))}
        start = [v for k, v in marks.items() if k.endswith("work buffer ready")]
        done = [v for k, v in marks.items() if k.endswith("done")]
        if start and done:
            spans[m.group(1)].append(done[0] - start[0])
    return {k: float(np.median(v)) if v else None for k, v in spans.items()}


def main():
    rng = np.random.default_rng(17)
    keys = np.unique(rng.integers(0, 2**64, size=N + 64, dtype=np.uint64))[:N]  # sorted, distinct
    assert keys.shape == (N,)
    rounds = WARMUP + CALLS
    leaves = [batch_np.felts_from_ints(wl.leaves(N, seed=700 + g)) for g in range(rounds + 1)]
    parts = None if CHILD else device_parts()  # before this process opens the device: one process at a time on it
    _lib.ensure_init()
    tree = state.LibrarySparseTree(64, 0)
    tree_update(tree, keys, leaves[0])
    records = batch_np.tree_witness_size(64, keys)
    level, index = np.zeros(records, dtype=np.uint8), np.zeros(records, dtype=np.uint64)
    node, left, right = (np.zeros((records, 4), dtype=np.uint64) for _ in range(3))
    proof_leaves, siblings = np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 64, 4), dtype=np.uint64)
    count = ctypes.c_size_t()
    lib = _lib.load()

    def witness(_):
        _lib.check(lib.sp_tree_witness(tree._handle, ptr(keys), N, records, ptr(level), ptr(index), ptr(node), ptr(left),
                                       ptr(right), ctypes.byref(count)), "sp_tree_witness")

    def prove(_):
        _lib.check(lib.sp_tree_prove(tree._handle, ptr(keys), N, ptr(proof_leaves), ptr(siblings)), "sp_tree_prove")

    def size(_):
        _lib.check(lib.sp_tree_witness_size(64, ptr(keys), N, ctypes.byref(count)), "sp_tree_witness_size")

    # the first witness is a witness: root on top, a sample of records hashes, the proofs' leaves are the leaves
    witness(0)
    assert count.value == records and level[-1] == 64 and index[-1] == 0
    assert batch_np.ints_from_felts(node[-1:])[0] == tree.root
    sample = np.sort(rng.choice(records, size=2048, replace=False))
    hashed = batch_np.pedersen_hash_many(left[sample], right[sample])
    assert (hashed == node[sample]).all(), "a witness record does not hash to its node"
    prove(0)
    assert (proof_leaves == leaves[0]).all()
    if CHILD:
        for r in range(CALLS):
            witness(r), prove(r)
        return
    a = timed(lambda r: tree_update(tree, keys, leaves[r + 1]), rounds)
    b = timed(witness, rounds)
    c = timed(prove, rounds)
    d = timed(size, rounds)
    w_bytes, p_bytes = records * 105, (N + N * 64) * 32
    fmt = lambda us: "not measured" if us is None else "%8.3f ms" % (us / 1e3)
    lines = [
        "tools/quick_tree_witness.py: %d keys on a height-64 tree holding as many; median / p90 of %d host-inclusive "
        "calls after %d, window bits %d" % (N, CALLS, WARMUP, lib.sp_window_bits()),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "(a) sp_tree_update of the %d keys                              %8.3f ms   p90 %8.3f ms" % ((N,) + a),
        "(b) sp_tree_witness: %d records, %.1f MB to the host       %8.3f ms   p90 %8.3f ms" % (
            (records, w_bytes / 1e6) + b),
        "    of which upload + kernels (timeline child, one extra wait)   %s" % fmt(parts["sp_tree_witness"]),
        "(c) sp_tree_prove: %d x 64 siblings, %.1f MB to the host        %8.3f ms   p90 %8.3f ms" % (
            (N, p_bytes / 1e6) + c),
        "    of which upload + kernel (timeline child, one extra wait)    %s" % fmt(parts["sp_tree_prove"]),
        "(d) sp_tree_witness_size (host arithmetic only)                  %8.3f ms   p90 %8.3f ms" % d,
        "b / a = %.3f    c / a = %.3f    copy-back rate of (b): %.1f GB/s over the whole call" % (
            b[0] / a[0], c[0] / a[0], w_bytes / b[0] / 1e6),
    ]
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tree_witness.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
