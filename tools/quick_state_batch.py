#!/usr/bin/env python3
"""The whole state update of a batch (state/state.cairo:135-186), host-inclusive, three ways in one process, NumPy
inputs prepacked outside the timing: height-64 trees that already hold 2048 positions and 4096 orders; every timed
call changes all 2048 positions (asset counts as tests/workloads.positions) and all 4096 orders.
  (a) one sp_state_batch call (batch_np.state_batch);
  (b) the best route before it, on the same arrays: one pedersen_chains_ragged call over previous and new chains,
      two sp_tree_get, two sp_tree_update, one after the other;
  (c) the floor: one sp_tree_update of the 4096 orders alone.
(a) and (b) run on two pairs of trees that are fed the same batches: their roots are asserted equal before anything
is timed.  Median and p90 of the calls after a warm-up; prints a / b and a / c.
    python tools/quick_state_batch.py [calls=24] [output file]"""
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
N_POS, N_ORD = 2048, 4096
EMPTY = (0, 0, ())


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def tree_get(tree, keys):
    out = np.empty((keys.shape[0], 4), dtype=np.uint64)
    _lib.check(_lib.load().sp_tree_get(tree._handle, ptr(keys), keys.shape[0], ptr(out)), "sp_tree_get")
    return out


def tree_update(tree, keys, leaves):
    roots, st = np.zeros((2, 4), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.load().sp_tree_update(tree._handle, ptr(keys), ptr(leaves), keys.shape[0], ptr(roots[0:1]),
                                          ptr(roots[1:2]), ptr(st)), "sp_tree_update")
    assert st[0] == 0
    return roots


def separate_calls(ptree, otree, arrays):
    """Route (b): what SharedState did before sp_state_batch, minus the Python-int packing."""
    pos_keys, prev_words, prev_off, new_words, new_off, ord_keys, ord_prev, ord_new = arrays
    n = pos_keys.shape[0]
    lengths = np.diff(new_off)
    changed = np.flatnonzero(lengths)
    off = np.concatenate([prev_off, prev_off[-1] + new_off[1:][changed]]).astype(np.uint32)
    hashes, st = batch_np.pedersen_chains_ragged(np.concatenate([prev_words, new_words]), off)
    assert not st.any()
    prev_h, new_h = hashes[:n], hashes[:n].copy()
    new_h[changed] = hashes[n:]
    assert (tree_get(ptree, pos_keys) == prev_h).all(), "previous position does not match the tree"
    assert (tree_get(otree, ord_keys) == ord_prev).all(), "previous order state does not match the tree"
    p_roots = tree_update(ptree, pos_keys, new_h)
    o_roots = tree_update(otree, ord_keys, ord_new)
    return p_roots, o_roots


def timed(fn, batches):
    """One call per prepared batch; the first WARMUP are not counted."""
    t = []
    for arrays in batches:
        t0 = time.perf_counter()
        fn(arrays)
        t.append(time.perf_counter() - t0)
    t = 1e3 * np.array(t[WARMUP:])
    return float(np.median(t)), float(np.percentile(t, 90))


def main():
    rng = np.random.default_rng(11)
    pos_keys = np.unique(rng.integers(0, 2**64, size=N_POS + 64, dtype=np.uint64))[:N_POS]  # sorted, distinct
    ord_keys = np.unique(rng.integers(0, 2**64, size=N_ORD + 64, dtype=np.uint64))[:N_ORD]
    assert pos_keys.shape == (N_POS,) and ord_keys.shape == (N_ORD,)
    n_batches = 1 + WARMUP + CALLS
    # generation g of the 2048 positions / 4096 order leaves; batch g takes the state from generation g to g + 1
    gens = [[(p[0], p[1], tuple(p[2])) for p in wl.positions(N_POS, seed=100 + g)] for g in range(n_batches + 1)]
    leaves = [batch_np.felts_from_ints(wl.leaves(N_ORD, seed=500 + g)) for g in range(n_batches + 1)]
    batches = []
    for g in range(n_batches):
        prev = [EMPTY] * N_POS if g == 0 else gens[g]
        packed = state.pack_state_batch([(int(k), p, q) for k, p, q in zip(pos_keys, prev, gens[g + 1])], [])
        ord_prev = np.zeros((N_ORD, 4), dtype=np.uint64) if g == 0 else leaves[g]
        batches.append(packed[:5] + (ord_keys, ord_prev, leaves[g + 1]))
    _lib.ensure_init()
    one, two, floor = state.SharedState(64, 64), state.SharedState(64, 64), state.LibrarySparseTree(64, 0)
    # the first batch fills the trees; (a) and (b) must agree on it and on every later one
    got = batch_np.state_batch(one.positions, one.orders, *batches[0])
    assert got[4] == 0, "the filling batch did not commit"
    want = separate_calls(two.positions, two.orders, batches[0])
    same = [got[0], got[1]] == [tuple(batch_np.ints_from_felts(r)) for r in want]
    assert same and one.positions_root == two.positions_root and one.orders_root == two.orders_root, \
        "sp_state_batch and the separate calls disagree"
    tree_update(floor, ord_keys, leaves[0])
    status = []

    def one_call(arrays):
        status.append(batch_np.state_batch(one.positions, one.orders, *arrays)[4])

    a = timed(one_call, batches[1:])
    b = timed(lambda arrays: separate_calls(two.positions, two.orders, arrays), batches[1:])
    c = timed(lambda arrays: tree_update(floor, ord_keys, arrays[7]), batches[1:])
    assert not any(status), "a timed batch did not commit"
    assert one.positions_root == two.positions_root and one.orders_root == two.orders_root, \
        "sp_state_batch and the separate calls disagree after the timed batches"
    words = int(batches[1][2][-1]) + int(batches[1][4][-1])
    lines = [
        "tools/quick_state_batch.py: %d positions (%d chain words, all changed) + %d orders per call, height-64 trees "
        "holding as many; median / p90 of %d host-inclusive calls after %d, window bits %d"
        % (N_POS, words, N_ORD, CALLS, WARMUP, _lib.load().sp_window_bits()),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "(a) one sp_state_batch call                                   %8.3f ms   p90 %8.3f ms" % a,
        "(b) ragged chains, 2 x sp_tree_get, 2 x sp_tree_update        %8.3f ms   p90 %8.3f ms" % b,
        "(c) floor: sp_tree_update of the %d orders alone            %8.3f ms   p90 %8.3f ms" % ((N_ORD,) + c),
        "a / b = %.3f    a / c = %.3f" % (a[0] / b[0], a[0] / c[0]),
    ]
    if a[0] >= b[0]:
        lines.append("NOTE: the single call is NOT faster than the separate calls on this run")
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "state_batch.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
