#!/usr/bin/env python3
"""Clone and ordered diff of persistent trees (sp_tree_clone, sp_tree_diff) beside the routes they replace, host-inclusive,
NumPy buffers allocated outside the timing; median and p90 of the calls after a warm-up, as tools/quick_tree_scan.py
takes its own.  All trees are height 64.
  (a) two trees of 4096 keys that differ in all of them: sp_tree_diff(0, 2^64 - 1, 4096) against sp_tree_scan of the
      4096-key page of one of them, measured beside it; the device part of the diff (upload of the empty roots, clear,
      kernels, without the copy back) from a step under STARKPERP_TIMELINE=1; the same answer in 16 sp_tree_diff calls
      of capacity 256;
  (b) two trees of 2^18 keys that differ in 4096: the 4096-key diff page against the route without sp_tree_diff - a full
      snapshot() of both trees and a NumPy compare - and against the page of (a): does the cost follow the answer or the
      trees;
  (c) sp_tree_clone of the 2^18-key tree against restore of its snapshot.
No threshold is set: the numbers are recorded.  Every answer is checked against the arrays written before anything is
timed.  Each GPU step is a process of its own under its own `timeout` (one process at a time on the device); the script
stops at the first step that fails.
    python tools/quick_tree_diff.py [calls=24] [output file]"""
import ctypes
import json
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

STEP = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--step" else None
CALLS = int(sys.argv[3]) if STEP else (max(8, int(sys.argv[1])) if len(sys.argv) > 1 else 24)
WARMUP = 0 if STEP == "timeline" else 4
N, BIG = 4096, 1 << 18
TOP = 2**64 - 1
STEP_LIMIT = {"timeline": 120, "small": 180, "big": 300}  # seconds, per step


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def timed(fn, calls=None):
    t = []
    for r in range(WARMUP + (CALLS if calls is None else calls)):
        t0 = time.perf_counter()
        fn(r)
        t.append(time.perf_counter() - t0)
    t = 1e3 * np.array(t[WARMUP:])
    return float(np.median(t)), float(np.percentile(t, 90))


def random_leaves(rng, n):
    leaves = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    leaves[:, 3] >>= np.uint64(8)  # below p
    return leaves


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 2**64, size=n + 64, dtype=np.uint64))[:n]  # sorted, distinct
    assert keys.shape == (n,)
    leaves = random_leaves(rng, n)
    tree = state.LibrarySparseTree(64, 0)
    for at in range(0, n, 1 << 16):
        tree.update_arrays(keys[at:at + (1 << 16)], leaves[at:at + (1 << 16)])
    return tree, keys, leaves


class Buffers:
    def __init__(self, lib):
        self.lib = lib
        self.k = np.zeros(N, dtype=np.uint64)
        self.a, self.b = np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)
        self.count, self.more = ctypes.c_size_t(), ctypes.c_int()

    def diff(self, x, y, cap, lo=0):
        _lib.check(self.lib.sp_tree_diff(x._handle, y._handle, lo, TOP, cap, ptr(self.k), ptr(self.a), ptr(self.b),
                                         ctypes.byref(self.count), ctypes.byref(self.more)), "sp_tree_diff")

    def scan(self, x, cap):
        _lib.check(self.lib.sp_tree_scan(x._handle, 0, TOP, cap, ptr(self.k), ptr(self.a), ctypes.byref(self.count),
                                         ctypes.byref(self.more)), "sp_tree_scan")

    def pages(self, x, y, cap):
        lo, calls = 0, 0
        while True:
            self.diff(x, y, cap, lo)
            calls += 1
            if not self.more.value:
                return calls
            lo = int(self.k[self.count.value - 1]) + 1


def small_pair():
    """Two trees of N keys, the same keys, every leaf different."""
    a, keys, leaves_a = random_tree(N, 17)
    leaves_b = random_leaves(np.random.default_rng(170), N)
    b = state.LibrarySparseTree(64, 0)
    b.update_arrays(keys, leaves_b)
    assert (leaves_a != leaves_b).any(axis=1).all()
    return a, b, keys, leaves_a, leaves_b


def step_small(timeline=False):
    lib = _lib.ensure_init()
    buf = Buffers(lib)
    a, b, keys, leaves_a, leaves_b = small_pair()
    buf.diff(a, b, N)
    assert buf.count.value == N and buf.more.value == 0
    assert (buf.k == keys).all() and (buf.a == leaves_a).all() and (buf.b == leaves_b).all()
    if timeline:
        for _ in range(CALLS):
            buf.diff(a, b, N)
        return {}
    out = {"diff": timed(lambda _: buf.diff(a, b, N)), "scan": timed(lambda _: buf.scan(a, N))}
    assert buf.pages(a, b, 256) == 16
    out["pages"] = timed(lambda _: buf.pages(a, b, 256))
    out["window_bits"] = lib.sp_window_bits()
    return out


def step_big():
    lib = _lib.ensure_init()
    buf = Buffers(lib)
    big, keys, leaves = random_tree(BIG, 18)
    entries, slots = batch_np.tree_table_size(big)
    # (c) first: the clone that (b) diffs against is one of the timed ones
    clones = []

    def clone(_):
        clones.append(big.clone())

    t_clone = timed(clone, calls=4)
    for c in clones[:-1]:
        c.close()
    other = clones[-1]
    assert other.root == big.root and batch_np.tree_table_size(other) == (entries, slots)
    t0 = time.perf_counter()
    snap = big.snapshot()
    t_snap = time.perf_counter() - t0
    assert (snap["keys"] == keys).all() and (snap["leaves"] == leaves).all()
    t0 = time.perf_counter()
    again = state.LibrarySparseTree.restore(snap)
    t_restore = time.perf_counter() - t0
    again.close()
    # (b) the clone receives other leaves at N of the keys
    rng = np.random.default_rng(180)
    where = np.sort(rng.choice(BIG, size=N, replace=False))
    changed = random_leaves(rng, N)
    other.update_arrays(keys[where], changed)
    buf.diff(big, other, N)
    assert buf.count.value == N and buf.more.value == 0
    assert (buf.k == keys[where]).all() and (buf.a == leaves[where]).all() and (buf.b == changed).all()

    def by_snapshots(_):
        s, t = big.snapshot(), other.snapshot()
        assert (s["keys"] == t["keys"]).all()  # (this pair holds the same keys; a general compare merges two key lists)
        rows = np.nonzero((s["leaves"] != t["leaves"]).any(axis=1))[0]
        assert rows.shape[0] == N

    out = {"diff": timed(lambda _: buf.diff(big, other, N)), "snapshots": timed(by_snapshots, calls=3),
           "clone": t_clone, "snapshot_ms": 1e3 * t_snap, "restore_ms": 1e3 * t_restore, "entries": entries, "slots": slots}
    a, b, _, _, _ = small_pair()
    out["small"] = timed(lambda _: buf.diff(a, b, N))
    return out


def run_step(name, env=None):
    """One GPU step in a process of its own, under its own time limit; raises at the first failure."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT[name]), sys.executable, os.path.abspath(__file__), "--step", name, str(CALLS)]
    out = subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (name, out.returncode, out.stderr[-2000:]))
    print("step %s done" % name, flush=True)
    return out


def device_part():
    """Median us between 'work buffer ready' and 'kernels done' of sp_tree_diff, from the timeline step."""
    out = run_step("timeline", {"STARKPERP_TIMELINE": "1"})
    spans = []
    for line in out.stderr.splitlines():
        m = re.match(r"libstarkperp timeline sp_tree_diff:(.*)", line)
        if not m:
            continue
        marks = {name.split(" [")[0].strip(): float(us) for us, name in re.findall(r"([\d.]+) us ([^;]+);", m.group(1))}
        start = [v for k, v in marks.items() if k.endswith("work buffer ready")]
        done = [v for k, v in marks.items() if k.endswith("kernels done")]
        if start and done:
            spans.append(done[0] - start[0])
    return float(np.median(spans)) if spans else None


def main():
    if STEP:
        result = step_small(timeline=True) if STEP == "timeline" else step_small() if STEP == "small" else step_big()
        print("RESULT " + json.dumps(result))
        return
    parts = device_part()
    results = {}
    for name in ("small", "big"):
        out = run_step(name)
        results[name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    s, b = results["small"], results["big"]
    fmt = lambda us: "not measured" if us is None else "%8.3f ms" % (us / 1e3)
    page_mb = (16 + (N + 2) * 8 + 2 * N * 32) / 1e6
    lines = [
        "tools/quick_tree_diff.py: height-64 trees; median / p90 of %d host-inclusive calls after %d, window bits %d" % (
            CALLS, 4, s["window_bits"]),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "launch decomposition: one workgroup for the top while the frontier fits 1024 threads, then one launch per level;"
        " four table probes per node kept (the only decomposition built)",
        "(a) two trees holding the same %d keys, every leaf different" % N,
        "    sp_tree_diff(0, 2^64 - 1, %d): %d keys, %.2f MB back                 %8.3f ms   p90 %8.3f ms" % (
            (N, N, page_mb) + tuple(s["diff"])),
        "      of which upload, clear and kernels (timeline step, one extra wait)   %s" % fmt(parts),
        "    sp_tree_scan of the %d-key page of one of them, measured beside it    %8.3f ms   p90 %8.3f ms" % (
            (N,) + tuple(s["scan"])),
        "    diff page / scan page = %.3f" % (s["diff"][0] / s["scan"][0]),
        "    16 sp_tree_diff calls of capacity 256 (one launch each)                 %8.3f ms   p90 %8.3f ms" % tuple(s["pages"]),
        "(b) two trees holding the same %d keys that differ in %d: table of %d entries in %d slots (%.2f GB) each" % (
            BIG, N, b["entries"], b["slots"], b["slots"] * 48 / 1e9),
        "    sp_tree_diff page of %d                                               %8.3f ms   p90 %8.3f ms" % (
            (N,) + tuple(b["diff"])),
        "    the page of (a), measured beside it                                     %8.3f ms   p90 %8.3f ms" % tuple(b["small"]),
        "    page of the large trees / page of the small trees = %.3f" % (b["diff"][0] / b["small"][0]),
        "    without sp_tree_diff: snapshot() of both trees + NumPy compare (3 calls) %8.1f ms   p90 %8.1f ms" % tuple(
            b["snapshots"]),
        "(c) sp_tree_clone of the %d-key tree (4 calls after 4, each a new %.2f GB table) %8.3f ms   p90 %8.3f ms" % (
            (BIG, b["slots"] * 48 / 1e9) + tuple(b["clone"])),
        "    snapshot of the %d keys (pages of 2^18)                                %8.1f ms" % (BIG, b["snapshot_ms"]),
        "    restore of the snapshot (sp_tree_update in chunks of 2^18)               %8.1f ms" % b["restore_ms"],
    ]
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tree_diff.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
