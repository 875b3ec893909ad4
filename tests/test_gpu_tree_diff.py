"""Clone and ordered diff of the library's persistent trees (sp_tree_clone, sp_tree_diff; include/starkperp.h) and the
deltas built on them.  Ground truth: the two plain dictionaries of what the test wrote into A and into B
(tree_diff_cases.differing / expected), and, where the twin is cheap enough, starkperp.state.SparseMerkleTree.diff on the
C oracle hash (checked against the dictionaries in tests/test_tree_diff_cpu.py).  Every comparison is exact.

Launch decomposition under test (csrc/merkle.hip): tree_diff_top_kernel walks the levels in one workgroup while the
frontier fits its 1024 threads and finishes the descent alone when capacity + 2 <= 1024; below the hand-over one
tree_diff_step_kernel launch per level with 256 nodes per block.  Every emitted node probes two children in TWO tables,
whose slot counts may differ and one of which may not exist."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import tree_diff_cases as D
from witness_replay import oracle_hash_many

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = D.P
BAD_ARGUMENT = -3
TOP64 = 2**64 - 1


def lib_tree(height, empty_leaf=0):
    from starkperp import state
    return state.LibrarySparseTree(height, empty_leaf)


def write(tree, mods):
    """Writes {key: int leaf} through the NumPy route."""
    from starkperp import batch_np
    keys = sorted(mods)
    tree.update_arrays(np.array(keys, dtype=np.uint64), batch_np.felts_from_ints([mods[k] for k in keys]))


def random_felts(rng, n):
    leaves = rng.integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    leaves[:, 3] >>= np.uint64(8)  # below p
    return leaves


# ---- 1. library against twin and dictionaries ---------------------------------------------------------------------------
def compare(a, b, twin_a, twin_b, in_a, in_b, what):
    triples = D.differing(in_a, in_b)
    assert (a.root, b.root) == (twin_a.root, twin_b.root), what
    for name, lo, hi, cap in D.queries(a.height, triples):
        got = a.diff(b, lo, hi, cap)
        assert got == D.expected(triples, lo, hi, cap), (what, name, lo, hi, cap)
        assert got == twin_a.diff(twin_b, lo, hi, cap), (what, name, lo, hi, cap)
    assert b.diff(a) == (D.swapped(triples), False), what
    assert list(a.diff_items(b, page=3)) == triples, what


@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_library_diff_equals_the_twin_and_the_dictionaries_over_a_sequence_of_batches(height):
    from starkperp import state
    start, rounds = D.pair_batches(height, sizes=(40, 7, 40))
    a, b = lib_tree(height), lib_tree(height)
    twin_a = state.SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    twin_b = state.SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    in_a, in_b = {}, {}
    compare(a, b, twin_a, twin_b, in_a, in_b, "two trees never updated")
    assert a.update(start) == twin_a.update(start)
    in_a.update(start)
    compare(a, b, twin_a, twin_b, in_a, in_b, "one tree never updated")
    assert b.update(start) == twin_b.update(start)
    in_b.update(start)
    compare(a, b, twin_a, twin_b, in_a, in_b, "equal trees")
    bad_leaf = np.array([[P & TOP64, 0, 0, P >> 192]], dtype=np.uint64)
    for r, (mods_a, mods_b) in enumerate(rounds):
        assert a.update(mods_a) == twin_a.update(mods_a)
        assert b.update(mods_b) == twin_b.update(mods_b)
        in_a.update(mods_a)
        in_b.update(mods_b)
        compare(a, b, twin_a, twin_b, in_a, in_b, "after batch %d" % r)
        if r == 1:  # a rejected update in between (a leaf >= p): the diff shows the old state
            with pytest.raises(AssertionError):
                b.update_arrays(np.array([sorted(in_b)[0]], dtype=np.uint64), bad_leaf)
            compare(a, b, twin_a, twin_b, in_a, in_b, "after a rejected update")
    a.close(), b.close()


# ---- 2. frontier sizes where the kernel path changes ----------------------------------------------------------------------
@pytest.mark.parametrize("height", [16, 64])
def test_frontier_sizes_at_the_wave_block_and_workgroup_edges(height):
    """63 / 64 / 65 differing keys (wave edge), 255 / 256 / 257 (a step block), 1023 / 1024 / 1025 (the top kernel's
    width: at 1025 it hands over to the step launches).  Per size: a page that holds everything and makes the step
    launches (capacity 4096: capacity + 2 > 1024), a page of exactly n, and n - 1 (cut at level 0 only); one sub-range.
    Even keys of the order differ by value, odd ones exist in A only; 50 further keys are equal in both."""
    rng = random.Random(1900 + height)
    order = D.distinct_keys(rng, height, 1075, (0, (1 << height) - 1))
    rng.shuffle(order)
    shared = D.leaves_for(rng, order[1025:])
    a, b = lib_tree(height), lib_tree(height)
    write(a, shared)
    write(b, shared)
    in_a, in_b, done = dict(shared), dict(shared), 0
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        fresh = order[done:n]
        done = n
        mods_a = D.leaves_for(rng, fresh)
        mods_b = D.leaves_for(rng, fresh[::2])
        write(a, mods_a)
        write(b, mods_b)
        in_a.update(mods_a)
        in_b.update(mods_b)
        triples = D.differing(in_a, in_b)
        assert len(triples) == n
        for cap in (4096, n, n - 1):
            assert a.diff(b, capacity=cap) == D.expected(triples, capacity=cap), (n, cap)
        lo, hi = triples[n // 3][0], triples[2 * n // 3][0]
        assert a.diff(b, lo + 1, hi, 4096) == D.expected(triples, lo + 1, hi, 4096), n
        assert b.diff(a, lo + 1, hi, n) == D.expected(D.swapped(triples), lo + 1, hi, n), n
    a.close(), b.close()


# ---- 3. the cut above level 0 ---------------------------------------------------------------------------------------------
def test_the_cut_above_level_0():
    """700 differing keys, 600 of them under one level-12 node, and 200 keys that are equal in both trees and must not
    appear.  The frontiers below level 12 overflow any page smaller than the answer, so the cut happens above level 0.
    The pages concatenate to the dictionaries' answer and `more` is False exactly on the last call."""
    rng = random.Random(44)
    keys = D.clustered_keys(600, 100)
    in_a = D.leaves_for(rng, keys)
    in_b = D.leaves_for(rng, keys[::3])  # a third differs by value, the rest exists in A only
    base = rng.randrange(1 << 52) << 12
    beside = ({base | low for low in rng.sample(range(1 << 12), 150)} | {k ^ 1 for k in keys[::4]}) - set(keys)
    shared = D.leaves_for(rng, sorted(beside)[:200])
    assert len(shared) == 200 and not set(shared) & set(keys)
    in_a.update(shared)
    in_b.update(shared)
    a, b = lib_tree(64), lib_tree(64)
    write(a, in_a)
    write(b, in_b)
    triples = D.differing(in_a, in_b)
    assert len(triples) == 700 and [t[0] for t in triples] == keys
    diff = lambda lo, hi, cap: a.diff(b, lo, hi, cap)
    for cap in (1, 255, 256, 257, 699, 700, 701):
        got, mores = D.pages(diff, 0, TOP64, cap)
        assert got == triples, cap
        assert mores == [True] * (-(-700 // cap) - 1) + [False], cap
    lo, hi = triples[350][0] + 1, triples[600][0]  # starts just behind a key of the cluster and ends inside it
    for cap in (1, 100, 1100):
        got, _ = D.pages(diff, lo, hi, cap)
        assert got == D.expected(triples, lo, hi)[0], cap
    a.close(), b.close()


# ---- 4. many blocks -------------------------------------------------------------------------------------------------------
def test_many_blocks():
    """20 000 differing keys on height 20 are 79 step blocks of 256 nodes: one page holds them all, pages of 5000 cut
    frontiers of 20 blocks above level 0.  Even positions differ by value, odd ones exist in A only."""
    from starkperp import batch_np
    rng = np.random.default_rng(21)
    keys = np.sort(rng.choice(1 << 20, size=20000, replace=False).astype(np.uint64))
    leaves_a, leaves_b = random_felts(rng, 20000), random_felts(rng, 20000)
    leaves_b[1::2] = 0
    a, b = lib_tree(20), lib_tree(20)
    a.update_arrays(keys, leaves_a)
    b.update_arrays(keys[::2], leaves_b[::2])
    assert (leaves_a != leaves_b).any(axis=1).all()
    k, va, vb, more = batch_np.tree_diff(a, b, 0, (1 << 20) - 1, 32768)
    assert not more and (k == keys).all() and (va == leaves_a).all() and (vb == leaves_b).all()
    lo, parts, mores = 0, [], []
    while True:
        k, va, vb, more = batch_np.tree_diff(a, b, lo, (1 << 20) - 1, 5000)
        parts.append((k, va, vb))
        mores.append(more)
        if not more:
            break
        lo = int(k[-1]) + 1
    assert mores == [True, True, True, False]
    for i, want in enumerate((keys, leaves_a, leaves_b)):
        assert (np.concatenate([p[i] for p in parts]) == want).all(), i
    lo, hi = int(keys[3000]), int(keys[17000])
    k, va, vb, more = batch_np.tree_diff(b, a, lo + 1, hi, 16000)
    assert not more and (k == keys[3001:17001]).all() and (va == leaves_b[3001:17001]).all() \
        and (vb == leaves_a[3001:17001]).all()
    a.close(), b.close()


# ---- 5. tables of different size ------------------------------------------------------------------------------------------
def test_tables_of_different_size():
    """A holds 40 keys in the initial table, B the same 40 and 2000 more in a table that has grown: every home slot is
    computed with its own table's mask."""
    from starkperp import batch_np
    rng = random.Random(55)
    keys = D.distinct_keys(rng, 64, 2040, (0, TOP64))
    rng.shuffle(keys)
    shared, extra = D.leaves_for(rng, keys[:40]), D.leaves_for(rng, keys[40:])
    a, b = lib_tree(64), lib_tree(64)
    write(a, shared)
    write(b, shared)
    write(b, extra)
    slots_a, slots_b = batch_np.tree_table_size(a)[1], batch_np.tree_table_size(b)[1]
    assert slots_a == 1 << 16 < slots_b, (slots_a, slots_b)
    want = [(k, 0, v) for k, v in sorted(extra.items())]
    assert a.diff(b) == (want, False)
    assert b.diff(a) == (D.swapped(want), False)
    assert a.diff(b, capacity=1999) == (want[:1999], True)
    a.close(), b.close()


# ---- 6. no table; equal roots ---------------------------------------------------------------------------------------------
def test_a_tree_without_a_table_and_equal_roots():
    from starkperp import _lib
    lib = _lib.ensure_init()
    rng = random.Random(6)
    written = D.leaves_for(rng, D.distinct_keys(rng, 64, 100, (0, TOP64)))
    fresh, other, full = lib_tree(64), lib_tree(64), lib_tree(64)
    write(full, written)
    want = [(k, 0, v) for k, v in sorted(written.items())]
    assert fresh.diff(full) == (want, False)
    assert full.diff(fresh) == (D.swapped(want), False)
    assert fresh.diff(full, capacity=7) == (want[:7], True)
    assert fresh.diff(other) == ([], False) and other.diff(fresh, 5, 9, 1) == ([], False)
    # equal roots by different histories: in two batches in another order, with a detour over a key set back to empty
    again = lib_tree(64)
    keys = sorted(written)
    write(again, {k: written[k] for k in keys[50:]})
    write(again, {**{k: written[k] for k in keys[:50]}, keys[3] ^ 1: 99})
    assert again.diff(full) == ([(keys[3] ^ 1, 99, 0)], False)
    write(again, {keys[3] ^ 1: 0})
    assert again.root == full.root
    total, launches, units = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(lib.sp_profile_begin(64), "sp_profile_begin")
    try:
        assert again.diff(full) == ([], False) and full.diff(again, 0, keys[10], 3) == ([], False)
    finally:
        _lib.check(lib.sp_profile_end(ctypes.byref(total), ctypes.byref(launches), ctypes.byref(units)), "sp_profile_end")
    assert launches.value == 0
    for tree in (fresh, other, full, again):
        tree.close()


# ---- 7. clone -------------------------------------------------------------------------------------------------------------
def test_clone_is_equal_and_independent():
    from starkperp import batch_np
    rng = random.Random(7)
    written = D.leaves_for(rng, D.distinct_keys(rng, 64, 300, (0, TOP64)))
    source = lib_tree(64)
    write(source, written)
    write(source, {sorted(written)[0]: 0})  # a path that holds empty roots is copied as it stands
    written[sorted(written)[0]] = 0
    pairs = sorted((k, v) for k, v in written.items() if v)
    copy = source.clone()
    probe = [k for k, _ in pairs[:18]] + [pairs[5][0] ^ 1, rng.randrange(2**64)]
    assert copy.root == source.root and copy.scan() == source.scan() == (pairs, False)
    assert copy.witness(probe) == source.witness(probe) and copy.prove(probe) == source.prove(probe)
    assert batch_np.tree_table_size(copy) == batch_np.tree_table_size(source) and copy.entries == source.entries
    assert (copy.height, copy.empty_leaf, copy.context) == (64, 0, 0)
    assert source.diff(copy) == ([], False)
    # updating the clone leaves the source as it was, and the reverse
    root = source.root
    k1, k2, k3 = pairs[7][0], pairs[8][0] ^ 1, pairs[9][0]
    mods = {k1: 111, k2: 222}
    write(copy, mods)
    assert source.root == root and source.scan() == (pairs, False) and copy.root != root
    want = D.differing(written, {**written, **mods})
    assert source.diff(copy) == (want, False) and [t[0] for t in want] == sorted(mods)
    copy_root, copy_scan = copy.root, copy.scan()
    write(source, {k3: 333})
    assert copy.root == copy_root and copy.scan() == copy_scan
    assert source.diff(copy) == (D.differing({**written, k3: 333}, {**written, **mods}), False)
    # a clone of a clone; closing the source, then updating and scanning the clone
    third = copy.clone()
    source.close()
    write(copy, {k1: 0})
    assert copy.get(k1) == 0 and third.get(k1) == 111 and third.root == copy_root
    assert copy.scan() == (sorted((k, v) for k, v in {**written, k1: 0, k2: 222}.items() if v), False)
    assert copy.diff(third) == ([(k1, 0, 111)], False)
    copy.close()
    assert third.scan() == copy_scan
    third.close()


def test_clone_of_a_fresh_tree_and_of_a_tree_with_another_empty_leaf():
    from starkperp import batch_np
    fresh = lib_tree(16)
    copy = fresh.clone()
    assert copy.root == fresh.root and copy.scan() == ([], False) and batch_np.tree_table_size(copy) == (0, 0)
    write(copy, {5: 6})
    assert fresh.scan() == ([], False) and fresh.diff(copy) == ([(5, 0, 6)], False)
    fresh.close(), copy.close()
    seven = lib_tree(16, 7)
    write(seven, {1: 2, 3: 7, 9: 4})
    copy = seven.clone()
    assert copy.empty_leaf == 7 and copy.root == seven.root
    assert copy.get_many([1, 2, 3, 9]) == [2, 7, 7, 4] and copy.scan() == ([(1, 2), (9, 4)], False)
    write(copy, {9: 7, 2: 8})
    assert seven.diff(copy) == ([(2, 7, 8), (9, 4, 7)], False)
    seven.close(), copy.close()


# ---- 8. a page above the staging limit --------------------------------------------------------------------------------------
def test_a_page_above_the_staging_limit_equals_a_staged_one():
    """(h + 1) 32 + 16 + (cap + 2) 8 + 2 cap 32 bytes come back through the page-locked buffer in one copy up to 4 MiB;
    above, the header comes back first and n keys and two runs of n leaves follow directly.  Capacity 4096 is
    0.3 MiB, capacity 2^17 is 9 MiB: the same 100 differing keys both ways."""
    from starkperp import batch_np
    size = lambda cap: 65 * 32 + 16 + (cap + 2) * 8 + 2 * cap * 32
    assert size(4096) <= 4 << 20 < size(1 << 17)
    rng = random.Random(18)
    keys = D.distinct_keys(rng, 64, 100, (0, TOP64))
    in_a, in_b = D.leaves_for(rng, keys), D.leaves_for(rng, keys[::2])
    a, b = lib_tree(64), lib_tree(64)
    write(a, in_a)
    write(b, in_b)
    small, large = (batch_np.tree_diff(a, b, 0, TOP64, cap) for cap in (4096, 1 << 17))
    triples = D.differing(in_a, in_b)
    assert large[0].tolist() == keys and not large[3]
    assert batch_np.ints_from_felts(large[1]) == [t[1] for t in triples]
    assert batch_np.ints_from_felts(large[2]) == [t[2] for t in triples]
    assert all((s == l).all() for s, l in zip(small[:3], large[:3])) and small[3] == large[3]
    lo, hi = keys[10] + 1, keys[60]
    small, large = (batch_np.tree_diff(a, b, lo, hi, cap) for cap in (4096, 1 << 17))
    assert len(large[0]) == 50 and all((s == l).all() for s, l in zip(small[:3], large[:3]))
    a.close(), b.close()


# ---- 9. bad arguments -----------------------------------------------------------------------------------------------------
PAT = 0xA5A5A5A5A5A5A5A5


def test_bad_arguments_leave_the_outputs_untouched():
    from starkperp import _lib
    lib = _lib.ensure_init()
    a, b, low, seven = lib_tree(16), lib_tree(16), lib_tree(15), lib_tree(16, 7)
    write(a, {3: 4, 9: 5})
    write(b, {3: 4, 9: 6, 11: 1})
    keys = np.full(4, PAT, dtype=np.uint64)
    leaves_a, leaves_b = np.full((4, 4), PAT, dtype=np.uint64), np.full((4, 4), PAT, dtype=np.uint64)
    count, more = ctypes.c_size_t(12345), ctypes.c_int(77)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None

    def call(ha, hb, lo, hi, cap, k=keys, va=leaves_a, vb=leaves_b, n=ctypes.byref(count), m=ctypes.byref(more)):
        return lib.sp_tree_diff(ha, hb, lo, hi, cap, ptr(k), ptr(va), ptr(vb), n, m)

    dead = lib_tree(16)
    dead_handle = dead._handle
    dead.close()
    ha, hb = a._handle, b._handle
    for name, rc in {
        "different heights": call(ha, low._handle, 0, 10, 4),
        "different empty leaves": call(ha, seven._handle, 0, 10, 4),
        "the same handle twice": call(ha, ha, 0, 10, 4),
        "a destroyed handle, first": call(dead_handle, hb, 0, 10, 4),
        "a destroyed handle, second": call(ha, dead_handle, 0, 10, 4),
        "an unknown handle, first": call(ha + 100000, hb, 0, 10, 4),
        "an unknown handle, second": call(ha, hb + 100000, 0, 10, 4),
        "lo > hi": call(ha, hb, 5, 4, 4),
        "hi = 2^16 on height 16": call(ha, hb, 0, 1 << 16, 4),
        "capacity = 0": call(ha, hb, 0, 10, 0),
        "null keys": call(ha, hb, 0, 10, 4, k=None),
        "null leaves_a": call(ha, hb, 0, 10, 4, va=None),
        "null leaves_b": call(ha, hb, 0, 10, 4, vb=None),
        "null count": call(ha, hb, 0, 10, 4, n=None),
        "null more": call(ha, hb, 0, 10, 4, m=None),
    }.items():
        assert rc == BAD_ARGUMENT, name
        assert lib.sp_last_error(), name
        assert (keys == PAT).all() and (leaves_a == PAT).all() and (leaves_b == PAT).all(), name
        assert count.value == 12345 and more.value == 77, name
    # sp_tree_clone: a null `clone`, a destroyed handle
    handle = ctypes.c_int(4711)
    assert lib.sp_tree_clone(ha, None) == BAD_ARGUMENT and lib.sp_last_error()
    assert lib.sp_tree_clone(dead_handle, ctypes.byref(handle)) == BAD_ARGUMENT and handle.value == 4711
    assert lib.sp_tree_clone(ha + 100000, ctypes.byref(handle)) == BAD_ARGUMENT and handle.value == 4711
    # after all of them, a good call writes nothing behind its answer
    assert call(ha, hb, 0, (1 << 16) - 1, 4) == 0
    assert (count.value, more.value, keys[:2].tolist()) == (2, 0, [9, 11])
    assert leaves_a[:2].tolist() == [[5, 0, 0, 0], [0, 0, 0, 0]] and leaves_b[:2].tolist() == [[6, 0, 0, 0], [1, 0, 0, 0]]
    assert keys[2] == PAT and (leaves_a[2:] == PAT).all() and (leaves_b[2:] == PAT).all()
    assert call(ha, hb, 0, (1 << 16) - 1, 1) == 0 and (count.value, more.value, int(keys[0])) == (1, 1, 9)
    assert keys[1] == 11 and (leaves_a[1] == 0).all()  # what the call before left: a page of 1 writes one place
    for tree in (a, b, low, seven):
        tree.close()


def test_trees_on_different_contexts_are_refused():
    from starkperp import _lib, state
    lib = _lib.ensure_init()
    if lib.sp_device_count() <= 1:
        pytest.skip("one context in this process: every tree lives on it")
    a, b = state.LibrarySparseTree(16, 0, context=0), state.LibrarySparseTree(16, 0, context=1)
    write(a, {1: 2})
    keys, va, vb = (np.full(n, PAT, dtype=np.uint64) for n in (2, 8, 8))
    count, more = ctypes.c_size_t(12345), ctypes.c_int(77)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = lib.sp_tree_diff(a._handle, b._handle, 0, 10, 2, ptr(keys), ptr(va), ptr(vb), ctypes.byref(count), ctypes.byref(more))
    assert rc == BAD_ARGUMENT and lib.sp_last_error()
    assert (keys == PAT).all() and (va == PAT).all() and (vb == PAT).all() and (count.value, more.value) == (12345, 77)
    a.close(), b.close()


# ---- 10. two threads diff in both argument orders while a third updates ------------------------------------------------------
def test_diffs_in_both_orders_beside_an_update():
    """diff(a, b) and diff(b, a) take the two mutexes in the same (handle) order, so they cannot block each other; every
    result is the diff against b before the update or after it, never a mixture (the update rewrites EVERY key of b)."""
    rng = random.Random(10)
    keys = D.distinct_keys(rng, 64, 300)
    in_a, old_b, new_b = D.leaves_for(rng, keys), D.leaves_for(rng, keys), D.leaves_for(rng, keys)
    new_b.update(D.leaves_for(rng, D.distinct_keys(rng, 64, 40)))
    a, b = lib_tree(64), lib_tree(64)
    write(a, in_a)
    write(b, old_b)
    allowed = [D.differing(in_a, old_b), D.differing(in_a, new_b)]
    assert allowed[0] != allowed[1]
    results, errors, started = {"ab": [], "ba": []}, [], threading.Event()

    def differ(name, x, y):
        try:
            for _ in range(50):
                results[name].append(x.diff(y, capacity=4096))
                started.set()
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append(e)

    def updater():
        try:
            started.wait(10)
            write(b, new_b)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=differ, args=("ab", a, b), daemon=True),
               threading.Thread(target=differ, args=("ba", b, a), daemon=True),
               threading.Thread(target=updater, daemon=True)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors
    assert len(results["ab"]) == 50 and len(results["ba"]) == 50
    for name, want in (("ab", allowed), ("ba", [D.swapped(t) for t in allowed])):
        seen = []
        for triples, more in results[name]:
            assert not more and triples in want, name
            seen.append(want.index(triples))
        assert seen == sorted(seen), name  # once a diff shows the new state, every later one does
    assert a.diff(b) == (allowed[1], False)
    a.close(), b.close()


# ---- 11. SharedState --------------------------------------------------------------------------------------------------------
def random_position(rng, n_assets):
    ids = set()
    while len(ids) < n_assets:
        ids.add(rng.randrange(1, 2**120))
    assets = tuple((i, rng.randrange(-(2**63), 2**63), rng.randrange(-(2**63), 2**63)) for i in sorted(ids))
    return (rng.randrange(2**251), rng.randrange(-(2**63), 2**63), assets)


def test_shared_state_fork_delta_and_apply_delta():
    from starkperp import batch_np, state
    rng = random.Random(11)
    empty = state.SharedState.EMPTY_POSITION
    p = [random_position(rng, n) for n in (2, 0, 5, 1)]
    base = state.SharedState(64, 16)
    base.apply_state_updates([(TOP64, empty, p[0]), (77, empty, p[1])], [(9, 0, 10), (2**16 - 1, 0, 3)])
    roots = (base.positions_root, base.orders_root)
    fork = base.fork()
    assert (fork.positions_root, fork.orders_root) == roots
    fork.apply_state_updates([(77, p[1], p[2]), (5, empty, p[3])], [(9, 10, 11), (40, 0, 2)])
    assert (base.positions_root, base.orders_root) == roots and fork.positions_root != roots[0]
    d = fork.delta(base)
    assert d["positions"]["keys"].tolist() == [5, 77] and d["orders"]["keys"].tolist() == [9, 40]
    assert batch_np.ints_from_felts(d["positions"]["leaves"]) == state.position_hashes_many([p[3], p[2]])
    assert d["orders"]["leaves"][:, 0].tolist() == [11, 2]
    assert (d["positions"]["base_root"], d["orders"]["base_root"]) == roots
    # a state that stands elsewhere in the ORDERS tree: the positions tree is not written either
    other = base.fork()
    write(other.orders, {1: 1})
    before = (other.positions_root, other.orders_root)
    with pytest.raises(ValueError):
        other.apply_delta(d)
    assert (other.positions_root, other.orders_root) == before
    assert base.apply_delta(d) == ((roots[0], fork.positions_root), (roots[1], fork.orders_root))
    assert base.positions.diff(fork.positions) == ([], False) and base.orders.diff(fork.orders) == ([], False)
    # a second fork keeps going where the first stands
    second = base.fork()
    step = ([(5, p[3], p[0])], [(40, 2, 3)])
    assert second.apply_state_updates(*step) == fork.apply_state_updates(*step)
    for s in (base, fork, other, second):
        s.close()


def test_delta_round_trip_through_the_library_and_the_twin():
    from starkperp import state
    start, rounds = D.pair_batches(64, sizes=(300, 50), seed=12)
    base = lib_tree(64)
    write(base, start)
    cur = base.clone()
    in_cur = dict(start)
    for mods, _ in rounds:
        write(cur, mods)
        in_cur.update(mods)
    delta = cur.delta(base, page=100)
    triples = D.differing(in_cur, start)
    assert delta["keys"].tolist() == [t[0] for t in triples] and (delta["base_root"], delta["root"]) == (base.root, cur.root)
    target = base.clone()
    assert target.apply_delta(delta, chunk=64) == (base.root, cur.root)
    assert target.diff(cur) == ([], False)
    elsewhere = base.clone()
    write(elsewhere, {0: 4242})
    before = (elsewhere.root, elsewhere.scan())
    with pytest.raises(ValueError):
        elsewhere.apply_delta(delta)
    assert (elsewhere.root, elsewhere.scan()) == before
    # the library's delta applies to a twin standing at the same root
    twin = state.SparseMerkleTree(64, 0, hash_many=oracle_hash_many)
    twin.update(start)
    assert twin.apply_delta(delta) == (base.root, cur.root)
    for tree in (base, cur, target, elsewhere):
        tree.close()


# ---- 12. a plain-C consumer -------------------------------------------------------------------------------------------------
def test_c_consumer_clones_a_tree_and_pages_the_diff():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_diff")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_diff.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.splitlines() == [
        "key 0 a 11 0 b 12 0", "key 8 a 0 0 b 66 2", "page 0 n 2 more 1",
        "key 9223372036854775808 a 33 0 b 0 0", "key 9223372036854775809 a 44 1 b 45 1", "page 1 n 2 more 1",
        "key 18446744073709551615 a 55 0 b 56 0", "page 2 n 1 more 0", "cabi_diff ok"]
