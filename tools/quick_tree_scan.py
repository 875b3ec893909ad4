#!/usr/bin/env python3
"""Ordered range scan (sp_tree_scan) beside the calls that read a tree by key, host-inclusive, NumPy buffers allocated
outside the timing; median and p90 of the calls after a warm-up, as tools/quick_tree_witness.py takes its own.
  (a) a height-64 tree holding 4096 random keys: sp_tree_scan(0, 2^64 - 1, 4096) against sp_tree_get and sp_tree_prove of
      the same 4096 keys, re-measured here; the device part of the scan (upload of the empty roots, clear, kernels,
      without the copy back) from a child process under STARKPERP_TIMELINE=1; the same answer in 16 pages of 256 through
      LibrarySparseTree.items;
  (b) one 4096-key page of a height-64 tree that holds 2^18 keys against the same page of the 4096-key tree: does the
      cost follow the answer or the table;
  (c) snapshot, restore and compacted() of the 2^18-key tree, and the table's slot count before and after.
No threshold is set: the numbers are recorded.  The first scan of each tree is checked against the keys written before
anything is timed.
    python tools/quick_tree_scan.py [calls=24] [output file]"""
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
from starkperp import _lib, batch_np, state  # noqa: E402
from evidence_stamp import lib_hash  # noqa: E402

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--timeline"
CALLS = 3 if CHILD else (max(8, int(sys.argv[1])) if len(sys.argv) > 1 else 24)
WARMUP = 0 if CHILD else 4
N, BIG = 4096, 1 << 18
TOP = 2**64 - 1


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def timed(fn, rounds=None):
    t = []
    for r in range(WARMUP + CALLS if rounds is None else rounds):
        t0 = time.perf_counter()
        fn(r)
        t.append(time.perf_counter() - t0)
    t = 1e3 * np.array(t[WARMUP if rounds is None else 0:])
    return float(np.median(t)), float(np.percentile(t, 90))


def device_part():
    """Child run: median us between 'work buffer ready' and 'kernels done' of sp_tree_scan."""
    env = dict(os.environ, STARKPERP_TIMELINE="1")
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--timeline"], env=env,
                         capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("timeline child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
    spans = []
    for line in out.stderr.splitlines():
        m = re.match(r"libstarkperp timeline sp_tree_scan:(.*)", line)
        if not m:
            continue
        marks = {name.split(" [")[0].strip(): float(us) for us, name in re.findall(r"([\d.]+) us ([^;]+);", m.group(1))}
        start = [v for k, v in marks.items() if k.endswith("work buffer ready")]
        done = [v for k, v in marks.items() if k.endswith("kernels done")]
        if start and done:
            spans.append(done[0] - start[0])
    return float(np.median(spans)) if spans else None


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 2**64, size=n + 64, dtype=np.uint64))[:n]  # sorted, distinct
    assert keys.shape == (n,)
    leaves = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    leaves[:, 3] >>= np.uint64(8)  # below p
    tree = state.LibrarySparseTree(64, 0)
    for at in range(0, n, 1 << 16):
        tree.update_arrays(keys[at:at + (1 << 16)], leaves[at:at + (1 << 16)])
    return tree, keys, leaves


def main():
    parts = None if CHILD else device_part()  # before this process opens the device: one process at a time on it
    lib = _lib.ensure_init()
    tree, keys, leaves = random_tree(N, 17)
    out_k, out_v = np.zeros(N, dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)
    sib = np.zeros((N, 64, 4), dtype=np.uint64)
    count, more = ctypes.c_size_t(), ctypes.c_int()

    def scan_of(t, cap):
        def call(_):
            _lib.check(lib.sp_tree_scan(t._handle, 0, TOP, cap, ptr(out_k), ptr(out_v), ctypes.byref(count),
                                        ctypes.byref(more)), "sp_tree_scan")
        return call

    def get(_):
        _lib.check(lib.sp_tree_get(tree._handle, ptr(keys), N, ptr(out_v)), "sp_tree_get")

    def prove(_):
        _lib.check(lib.sp_tree_prove(tree._handle, ptr(keys), N, ptr(out_v), ptr(sib)), "sp_tree_prove")

    scan_of(tree, N)(0)
    assert count.value == N and more.value == 0 and (out_k == keys).all() and (out_v == leaves).all()
    if CHILD:
        for r in range(CALLS):
            scan_of(tree, N)(r)
        return
    a_scan, a_get, a_prove = timed(scan_of(tree, N)), timed(get), timed(prove)
    assert [k for k, _ in tree.items(page=256)] == keys.tolist()
    a_pages = timed(lambda _: sum(1 for _ in tree.items(page=256)))
    raw_pages = timed(lambda _: [scan_of(tree, 256)(0) for _ in range(16)])  # 16 calls of 256 without the Python lists

    big, big_keys, big_leaves = random_tree(BIG, 18)
    scan_of(big, N)(0)
    assert count.value == N and more.value == 1 and (out_k == big_keys[:N]).all() and (out_v == big_leaves[:N]).all()
    b_big, b_small = timed(scan_of(big, N)), timed(scan_of(tree, N))

    entries, slots = batch_np.tree_table_size(big)
    t0 = time.perf_counter()
    snap = big.snapshot()
    t_snap = time.perf_counter() - t0
    assert (snap["keys"] == big_keys).all() and (snap["leaves"] == big_leaves).all()
    t0 = time.perf_counter()
    again = state.LibrarySparseTree.restore(snap)
    t_restore = time.perf_counter() - t0
    again.close()
    # slots that hold nothing live: every key of the upper half is set back to the empty leaf, then compacted()
    half = BIG // 2
    for at in range(half, BIG, 1 << 16):
        big.update_arrays(big_keys[at:at + (1 << 16)], np.zeros((min(1 << 16, BIG - at), 4), dtype=np.uint64))
    e_reset, s_reset = batch_np.tree_table_size(big)
    t0 = time.perf_counter()
    small = big.compacted()
    t_compact = time.perf_counter() - t0
    e_small, s_small = batch_np.tree_table_size(small)
    assert small.root == big.root

    fmt = lambda us: "not measured" if us is None else "%8.3f ms" % (us / 1e3)
    lines = [
        "tools/quick_tree_scan.py: height-64 trees; median / p90 of %d host-inclusive calls after %d, window bits %d" % (
            CALLS, WARMUP, lib.sp_window_bits()),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "launch decomposition: one workgroup for the top while the frontier fits 1024 threads, then one launch per level"
        " (the only decomposition built; kernel variants measured and dropped: DESIGN 11 row 18)",
        "(a) tree holding %d keys" % N,
        "    sp_tree_scan(0, 2^64 - 1, %d): %d keys, %.2f MB back          %8.3f ms   p90 %8.3f ms" % (
            (N, N, (16 + (N + 2) * 8 + N * 32) / 1e6) + a_scan),
        "      of which upload, clear and kernels (timeline child, one extra wait)  %s" % fmt(parts),
        "    sp_tree_get of the %d keys                                    %8.3f ms   p90 %8.3f ms" % ((N,) + a_get),
        "    sp_tree_prove of the %d keys                                  %8.3f ms   p90 %8.3f ms" % ((N,) + a_prove),
        "    16 pages of 256 through LibrarySparseTree.items (Python lists)  %8.3f ms   p90 %8.3f ms" % a_pages,
        "    16 sp_tree_scan calls of capacity 256 (one launch each)         %8.3f ms   p90 %8.3f ms" % raw_pages,
        "(b) one %d-key page (more = 1) of a tree holding %d keys            %8.3f ms   p90 %8.3f ms" % ((N, BIG) + b_big),
        "    the %d-key page of the tree holding %d keys, measured beside it %8.3f ms   p90 %8.3f ms" % ((N, N) + b_small),
        "    page of the large tree / page of the small tree = %.3f; table: %d entries in %d slots (%.2f GB)" % (
            b_big[0] / b_small[0], entries, slots, slots * 48 / 1e9),
        "(c) snapshot of the %d keys (pages of 2^18)                        %8.1f ms" % (BIG, 1e3 * t_snap),
        "    restore of the snapshot (sp_tree_update in chunks of 2^18)       %8.1f ms" % (1e3 * t_restore),
        "    after setting %d keys back to the empty leaf: %d entries in %d slots" % (BIG - half, e_reset, s_reset),
        "    compacted() (snapshot + restore of %d keys)                      %8.1f ms: %d entries in %d slots" % (
            half, 1e3 * t_compact, e_small, s_small),
    ]
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tree_scan.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
