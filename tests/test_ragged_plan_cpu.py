"""The fallback plan of the ragged walks (csrc/ragged_plan.hpp: chains of unequal length and Merkle paths, hashed step
by step when no fused kernel serves the call) on the host, no GPU: g++ builds tests/host/ragged_plan_shim.cpp, and the
plan is replayed on Python integers with a non-commutative toy hash - gather by the index pairs of each step, write
the running values of the prefix, scatter by the permutation - against the direct left fold (chains) and the sided
fold of merkle_path_cases.oracle_roots' rule (paths: at level l the sibling is the left operand if bit l of the key is
set).  Also: the order is the stable sort by falling step count, running[s] counts the items of more than s steps, and
the sizes are the ones enqueue_pedersen_fold_ragged reserves from."""
import ctypes
import os
import subprocess

import pytest

from test_chains_ragged_cpu import spy

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "host", "ragged_plan_shim.cpp")
    so = os.path.join(HERE, "host", "ragged_plan_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.rp_sizes.restype = lib.rp_fill.restype = None
    lib.rp_sizes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.rp_fill.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def plan(shim, lens, keys):
    """The plan of items of `lens` words (keys = None: chains) as Python lists."""
    n = len(lens)
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    c_off = (ctypes.c_uint32 * (n + 1))(*off)
    c_keys = (ctypes.c_uint64 * n)(*keys) if keys is not None else None
    info = (ctypes.c_uint64 * 5)()
    shim.rp_sizes(c_off, c_keys, n, info)
    meta_len, max_steps, n_pairs, pairs_at, work_felts = list(info)
    meta = (ctypes.c_uint32 * max(meta_len, 1))()
    running = (ctypes.c_uint64 * max(max_steps, 1))()
    shim.rp_fill(c_off, c_keys, n, meta, running)
    return dict(off=off, meta=list(meta)[:meta_len], running=list(running)[:max_steps], max_steps=max_steps,
                n_pairs=n_pairs, pairs_at=pairs_at, work_felts=work_felts)


def check(shim, lens, keys):
    n, sided = len(lens), keys is not None
    lone = 0 if sided else 1
    steps = [k - lone for k in lens]
    p = plan(shim, lens, keys)
    off, meta = p["off"], p["meta"]
    words = [1000 + 7 * i for i in range(off[-1])]
    leaves = [900000 + 11 * i for i in range(n)]
    # ---- layout and sizes: off | perm | step_off | pad to 8 bytes | pairs ----
    assert meta[:n + 1] == off
    perm = meta[n + 1:2 * n + 1]
    assert perm == sorted(range(n), key=lambda c: -steps[c])  # sorted() is stable: ties keep the caller's order
    assert p["max_steps"] == max(steps)
    assert p["running"] == [sum(1 for s in steps if s > j) for j in range(p["max_steps"])]
    assert p["n_pairs"] == sum(steps) == sum(p["running"])
    assert p["pairs_at"] % 2 == 0 and 0 <= p["pairs_at"] - (2 * n + 1 + p["max_steps"]) <= 1
    assert len(meta) == p["pairs_at"] + 2 * p["n_pairs"]
    assert p["work_felts"] == (2 * n if sided else n) + off[-1]
    step_off = meta[2 * n + 1:2 * n + 1 + p["max_steps"]]
    assert step_off == [sum(p["running"][:j]) for j in range(p["max_steps"])]
    # ---- replay: the work buffer as the enqueue fills it ----
    work = [None] * n + (leaves if sided else []) + words
    assert len(work) == p["work_felts"]
    pairs = meta[p["pairs_at"]:]
    for j in range(p["max_steps"]):
        m = p["running"][j]
        got = []
        for k in range(m):
            a, b = pairs[2 * (step_off[j] + k)], pairs[2 * (step_off[j] + k) + 1]
            assert a < len(work) and b < len(work) and work[a] is not None and work[b] is not None
            got.append(spy(work[a], work[b]))
        work[:m] = got  # a launch reads all its operands' positions before the next one runs
    have = [None] * n
    for k, c in enumerate(perm):
        have[c] = work[k] if steps[c] else (leaves[c] if sided else words[off[c]])
    # ---- the direct folds ----
    want = []
    for c in range(n):
        item = words[off[c]:off[c + 1]]
        if sided:
            node = leaves[c]
            for level, sib in enumerate(item):
                node = spy(sib, node) if (keys[c] >> level) & 1 else spy(node, sib)
        else:
            node = item[0]
            for w in item[1:]:
                node = spy(node, w)
        want.append(node)
    assert have == want
    return p


def test_single_item_of_no_steps(shim):
    assert check(shim, [1], None)["max_steps"] == 0
    assert check(shim, [0], [0])["max_steps"] == 0


def test_equal_lengths(shim):
    check(shim, [4] * 6, None)
    check(shim, [5] * 6, [0, 31, 21, 10, 1, 16])


def test_mixed_unsorted_lengths_with_ties(shim):
    check(shim, [2, 64, 1, 2, 1, 64, 3, 2], None)
    lens = [1, 64, 0, 2, 1, 0, 64, 2]
    check(shim, lens, [0] * 8)
    check(shim, lens, [(1 << k) - 1 for k in lens])  # all ones
    alt = 0x5555555555555555
    check(shim, lens, [alt & ((1 << k) - 1) for k in lens])
    check(shim, lens, [0, 1 << 63, 0, 0, 0, 0, 1 << 63, 0])  # only the last step of a 64-step path swaps
    check(shim, [64], [ALL_ONES])


def test_pairs_offset_with_and_without_the_alignment_pad(shim):
    # 2 n + 1 + max_steps: odd -> one word of padding, even -> none
    a = check(shim, [3, 1], None)     # n = 2, max_steps = 2: 7 -> 8
    assert a["pairs_at"] == 8
    b = check(shim, [4, 1], None)     # n = 2, max_steps = 3: 8
    assert b["pairs_at"] == 8
    c = check(shim, [2, 0, 1], [2, 0, 1])  # n = 3, max_steps = 2: 9 -> 10
    assert c["pairs_at"] == 10
    d = check(shim, [3, 0, 1], [5, 0, 1])  # n = 3, max_steps = 3: 10
    assert d["pairs_at"] == 10
