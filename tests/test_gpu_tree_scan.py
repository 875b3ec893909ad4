"""Ordered range scan of the library's persistent trees (sp_tree_scan; include/starkperp.h), snapshot, restore and
compaction built on it.  Ground truth: the plain dictionary of what the test wrote (tree_scan_cases.live / expected),
and, where the twin is cheap enough, starkperp.state.SparseMerkleTree.scan on the C oracle hash (checked against the
dictionary in tests/test_tree_scan_cpu.py).  Every comparison is exact.

Launch decomposition under test (csrc/merkle.hip): tree_scan_top_kernel walks the levels in one workgroup while the
frontier fits its 1024 threads (SCAN_TOP) and finishes the descent alone when capacity + 2 <= 1024; below the hand-over
one tree_scan_step_kernel launch per level with 256 nodes per block (SCAN_BLOCK).  A step block sums the totals of the
blocks in front of it itself, so there is NO further tile (no scan of block totals) whose width a test would have to
cross; test_many_blocks covers a frontier of many blocks instead."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

import tree_scan_cases as C
from witness_replay import oracle_hash_many

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.P
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


# ---- 1. library against twin and dictionary ------------------------------------------------------------------------
def compare(tree, twin, written, what):
    pairs = C.live(written)
    assert tree.root == twin.root, what
    for name, lo, hi, cap in C.queries(tree.height, pairs):
        got = tree.scan(lo, hi, cap)
        assert got == C.expected(pairs, lo, hi, cap), (what, name, lo, hi, cap)
        assert got == twin.scan(lo, hi, cap), (what, name, lo, hi, cap)
    assert list(tree.items(page=3)) == pairs, what


@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_library_scan_equals_the_twin_and_the_dictionary_over_a_sequence_of_batches(height):
    from starkperp import state
    tree = lib_tree(height)
    twin = state.SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    written = {}
    compare(tree, twin, written, "a tree never updated")
    bad_leaf = np.array([[P & TOP64, 0, 0, P >> 192]], dtype=np.uint64)
    with pytest.raises(AssertionError):  # a rejected update on the fresh tree: its table exists and holds nothing
        tree.update_arrays(np.array([0], dtype=np.uint64), bad_leaf)
    compare(tree, twin, written, "a fresh tree after a rejected update")
    for r, mods in enumerate(C.batches(height, sizes=(40, 7, 40))):
        assert tree.update(mods) == twin.update(mods)
        written.update(mods)
        compare(tree, twin, written, "after batch %d" % r)
        if r == 1:  # a rejected update in between: the scan shows the old state
            with pytest.raises(AssertionError):
                tree.update_arrays(np.array([sorted(written)[0]], dtype=np.uint64), bad_leaf)
            compare(tree, twin, written, "after a rejected update")
    tree.close()


# ---- 2. frontier sizes where the kernel path changes -----------------------------------------------------------------
@pytest.mark.parametrize("height", [16, 64])
def test_frontier_sizes_at_the_wave_block_and_workgroup_edges(height):
    """63 / 64 / 65 leaves (wave edge), 255 / 256 / 257 (SCAN_BLOCK), 1023 / 1024 / 1025 (SCAN_TOP: at 1025 the top
    kernel hands over to the step launches).  Per size: a page that holds everything and makes the step launches
    (capacity 4096), a page of exactly n, and n - 1 (cut at level 0 only)."""
    rng = random.Random(900 + height)
    order = C.distinct_keys(rng, height, 1025, (0, (1 << height) - 1))
    rng.shuffle(order)
    tree, written = lib_tree(height), {}
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        fresh = C.leaves_for(rng, order[len(written):n])
        write(tree, fresh)
        written.update(fresh)
        pairs = C.live(written)
        assert len(pairs) == n
        for cap in (4096, n, n - 1):
            assert tree.scan(capacity=cap) == C.expected(pairs, capacity=cap), (n, cap)
        lo, hi = pairs[n // 3][0], pairs[2 * n // 3][0]
        assert tree.scan(lo + 1, hi, 4096) == C.expected(pairs, lo + 1, hi, 4096), n
    tree.close()


# ---- 3. no further tile: many blocks instead ---------------------------------------------------------------------------
def test_many_blocks():
    """The decomposition has no tile of block totals (a step block sums the totals in front of it itself).  What is left
    to cover is a frontier of many blocks: 20 000 leaves on a height-20 tree are 79 blocks of SCAN_BLOCK = 256 nodes; one
    page holds them all, and pages of 5000 cut frontiers of 20 blocks above level 0."""
    from starkperp import batch_np
    rng = np.random.default_rng(20)
    keys = np.sort(rng.choice(1 << 20, size=20000, replace=False).astype(np.uint64))
    leaves = rng.integers(1, 2**63, size=(20000, 4), dtype=np.uint64)
    leaves[:, 3] >>= np.uint64(8)  # below p
    tree = lib_tree(20)
    tree.update_arrays(keys, leaves)
    got_k, got_v, more = batch_np.tree_scan(tree, 0, (1 << 20) - 1, 32768)
    assert not more and (got_k == keys).all() and (got_v == leaves).all()
    lo, parts, mores = 0, [], []
    while True:
        k, v, more = batch_np.tree_scan(tree, lo, (1 << 20) - 1, 5000)
        parts.append((k, v))
        mores.append(more)
        if not more:
            break
        lo = int(k[-1]) + 1
    assert mores == [True, True, True, False]
    assert (np.concatenate([k for k, _ in parts]) == keys).all() and (np.concatenate([v for _, v in parts]) == leaves).all()
    a, b = int(keys[3000]), int(keys[17000])
    got_k, got_v, more = batch_np.tree_scan(tree, a + 1, b, 16000)
    assert not more and (got_k == keys[3001:17001]).all() and (got_v == leaves[3001:17001]).all()
    tree.close()


def test_a_page_above_the_staging_limit_equals_a_staged_one():
    """The page's capacity decides how it travels, not what the tree holds: (h + 1) 32 + 16 + (cap + 2) 8 + cap 32 bytes
    come back through the tree's page-locked buffer in one copy up to 4 MiB; above, the header comes back first and the
    n keys and leaves follow directly (csrc/merkle.hip sp_tree_scan).  Capacity 4096 is 0.16 MiB, capacity 2^17 is
    5 MiB: the same 100 keys both ways."""
    from starkperp import batch_np
    size = lambda cap: 65 * 32 + 16 + (cap + 2) * 8 + cap * 32
    assert size(4096) <= 4 << 20 < size(1 << 17)
    rng = random.Random(17)
    mods = C.leaves_for(rng, C.distinct_keys(rng, 64, 100, (0, TOP64)))
    tree = lib_tree(64)
    write(tree, mods)
    small, large = (batch_np.tree_scan(tree, 0, TOP64, cap) for cap in (4096, 1 << 17))
    assert large[0].tolist() == sorted(mods) and not large[2]
    assert (small[0] == large[0]).all() and (small[1] == large[1]).all() and small[2] == large[2]
    lo, hi = sorted(mods)[10] + 1, sorted(mods)[60]
    small, large = (batch_np.tree_scan(tree, lo, hi, cap) for cap in (4096, 1 << 17))
    assert len(large[0]) == 50 and (small[0] == large[0]).all() and (small[1] == large[1]).all()
    tree.close()


# ---- 4. the cut ------------------------------------------------------------------------------------------------------
def test_the_cut_above_level_0():
    """700 leaves, 600 of them under one level-12 node: the frontiers above level 12 have about 100 nodes, the ones below
    overflow any page smaller than the answer, so the cut happens above level 0.  The pages concatenate to the
    dictionary and `more` is False exactly on the last call."""
    rng = random.Random(44)
    written = C.leaves_for(rng, C.clustered_keys(600, 100))
    tree = lib_tree(64)
    write(tree, written)
    pairs = C.live(written)
    assert len(pairs) == 700
    for cap in (1, 255, 256, 257, 699, 700, 701):
        got, mores = C.pages(tree.scan, 0, TOP64, cap)
        assert got == pairs, cap
        assert mores == [True] * (-(-700 // cap) - 1) + [False], cap
    # a range that starts just behind a key of the cluster and ends inside it
    lo, hi = pairs[350][0] + 1, pairs[600][0]
    for cap in (1, 100, 1100):
        got, mores = C.pages(tree.scan, lo, hi, cap)
        assert got == C.expected(pairs, lo, hi)[0], cap
    tree.close()


# ---- 5. reset leaves on the device; 8. compaction -----------------------------------------------------------------------
def test_reset_leaves_are_pruned_by_value_and_compaction_drops_their_slots():
    """300 written, 299 set back to the empty leaf, the survivor being the LARGEST key.  The slots of the 299 are still in
    the table (get returns the empty leaf, the entry count has not shrunk): a descent that tested presence only would
    fill the page of 1 with a dead node.  compacted() holds the same tree in no more entries."""
    rng = random.Random(5)
    written = C.leaves_for(rng, C.distinct_keys(rng, 64, 300))
    tree = lib_tree(64)
    write(tree, written)
    before = tree.entries
    assert before >= 300
    largest = max(written)
    reset = {k: 0 for k in written if k != largest}
    write(tree, reset)
    written.update(reset)
    assert tree.get_many(sorted(reset)) == [0] * 299
    assert tree.entries >= before
    assert tree.scan(capacity=1) == ([(largest, written[largest])], False)
    assert tree.scan(0, largest - 1, 1) == ([], False)
    assert tree.scan() == ([(largest, written[largest])], False)
    small = tree.compacted()
    assert small.entries <= 65 < tree.entries  # one leaf and its path up to the root
    assert small.root == tree.root and small.scan() == tree.scan()
    small.close()
    write(tree, {largest: 0})
    assert tree.scan() == ([], False) and tree.scan(capacity=1) == ([], False)
    tree.close()


# ---- 6. one leaf's interval, the upper half ------------------------------------------------------------------------------
def test_range_of_one_key_between_written_neighbours_and_the_upper_half():
    rng = random.Random(6)
    k = (rng.randrange(1 << 62) << 1) | 1  # odd: its neighbours sit under different parents
    written = C.leaves_for(rng, [0, k - 1, k, k + 1, 2**63 - 1, 2**63, 2**63 + 5, TOP64])
    tree = lib_tree(64)
    write(tree, written)
    pairs = C.live(written)
    assert tree.scan(k, k) == ([(k, written[k])], False)
    assert tree.scan(k, k, 1) == ([(k, written[k])], False)
    assert tree.scan(k - 1, k + 1, 2) == ([(k - 1, written[k - 1]), (k, written[k])], True)
    assert tree.scan(2**63, TOP64) == (pairs[-3:], False)
    assert tree.scan(2**63, TOP64, 2) == (pairs[-3:-1], True)
    assert tree.scan(TOP64, TOP64) == (pairs[-1:], False)
    assert tree.scan(0, 2**63 - 1) == (pairs[:-3], False)
    assert tree.scan(2**63 - 1, 2**63) == (pairs[4:6], False)
    tree.close()


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched():
    from starkperp import _lib
    lib = _lib.ensure_init()
    tree = lib_tree(16)
    write(tree, {3: 4, 9: 5})
    PAT = 0xA5A5A5A5A5A5A5A5
    keys, leaves = np.full(4, PAT, dtype=np.uint64), np.full((4, 4), PAT, dtype=np.uint64)
    count, more = ctypes.c_size_t(12345), ctypes.c_int(77)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(handle, lo, hi, cap, k=keys, v=leaves, n=ctypes.byref(count), m=ctypes.byref(more)):
        return lib.sp_tree_scan(handle, lo, hi, cap, ptr(k) if k is not None else None, ptr(v) if v is not None else None, n, m)

    handle = tree._handle
    dead = lib_tree(16)
    dead_handle = dead._handle
    dead.close()
    for name, rc in {
        "lo > hi": call(handle, 5, 4, 4),
        "hi = 2^16 on height 16": call(handle, 0, 1 << 16, 4),
        "capacity = 0": call(handle, 0, 10, 0),
        "a destroyed handle": call(dead_handle, 0, 10, 4),
        "an unknown handle": call(handle + 100000, 0, 10, 4),
        "null keys": call(handle, 0, 10, 4, k=None),
        "null leaves": call(handle, 0, 10, 4, v=None),
        "null count": call(handle, 0, 10, 4, n=None),
        "null more": call(handle, 0, 10, 4, m=None),
    }.items():
        assert rc == BAD_ARGUMENT, name
        assert lib.sp_last_error(), name
        assert (keys == PAT).all() and (leaves == PAT).all() and count.value == 12345 and more.value == 77, name
    assert call(handle, 0, (1 << 16) - 1, 4) == 0
    assert (count.value, more.value, keys[:2].tolist(), leaves[:2, 0].tolist()) == (2, 0, [3, 9], [4, 5])
    assert keys[2] == PAT and (leaves[2:] == PAT).all()  # nothing behind the answer
    tree.close()


# ---- 8. snapshot -> restore ------------------------------------------------------------------------------------------------
def test_snapshot_restores_to_an_equal_tree_on_context_0():
    from starkperp import state
    rng = random.Random(8)
    tree, written = lib_tree(64, 7), {}
    for mods in C.batches(64, sizes=(300, 50), seed=8):
        mods = {k: (v or 7) for k, v in mods.items()}  # this tree's empty leaf is 7
        write(tree, mods)
        written.update(mods)
    pairs = C.live(written, 7)
    snap = tree.snapshot(page=128)
    assert (snap["height"], snap["empty_leaf"], snap["root"]) == (64, 7, tree.root)
    assert snap["keys"].tolist() == [k for k, _ in pairs]
    again = state.LibrarySparseTree.restore(snap, context=0, chunk=100)
    assert again.root == tree.root and again.scan() == tree.scan() == (pairs, False)
    probe = [k for k, _ in pairs[:20]] + [pairs[5][0] ^ 1, rng.randrange(2**64)]
    assert again.witness(probe) == tree.witness(probe) and again.prove(probe) == tree.prove(probe)
    assert again.entries <= tree.entries
    again.close()
    spoiled = dict(snap, leaves=snap["leaves"].copy())
    spoiled["leaves"][17, 0] ^= np.uint64(1)
    with pytest.raises(ValueError):
        state.LibrarySparseTree.restore(spoiled)
    # a twin's snapshot (lists) restores to the library as well
    listed = dict(snap, keys=[k for k, _ in pairs], leaves=[v for _, v in pairs])
    third = state.LibrarySparseTree.restore(listed)
    assert third.root == tree.root
    third.close()
    tree.close()


# ---- 9. SharedState ----------------------------------------------------------------------------------------------------------
def random_position(rng, n_assets):
    ids = set()
    while len(ids) < n_assets:
        ids.add(rng.randrange(1, 2**120))
    ids = sorted(ids)
    assets = tuple((a, rng.randrange(-(2**63), 2**63), rng.randrange(-(2**63), 2**63)) for a in ids)
    return (rng.randrange(2**251), rng.randrange(-(2**63), 2**63), assets)


def test_shared_state_snapshot_and_restore():
    from starkperp import state
    rng = random.Random(9)
    empty = state.SharedState.EMPTY_POSITION
    one = state.SharedState(64, 16)
    p = [random_position(rng, n) for n in (2, 0, 5)]
    one.apply_state_updates([(TOP64, empty, p[0]), (77, empty, p[1]), (5, empty, p[2])], [(9, 0, 10), (2**16 - 1, 0, 3)])
    snap = one.snapshot()
    assert snap["positions"]["keys"].tolist() == [5, 77, TOP64] and snap["orders"]["keys"].tolist() == [9, 2**16 - 1]
    assert snap["orders"]["leaves"][:, 0].tolist() == [10, 3]
    two = state.SharedState.restore(snap)
    assert (two.positions_root, two.orders_root) == (one.positions_root, one.orders_root)
    assert two.positions.scan() == one.positions.scan() and two.orders.scan() == one.orders.scan()
    assert len(one.positions.scan()[0]) == 3
    # the restored state goes on where the first one stands
    step = ([(77, p[1], p[0])], [(9, 10, 11)])
    assert two.apply_state_updates(*step) == one.apply_state_updates(*step)
    one.close(), two.close()


# ---- 10. a second thread updates while the first pages -------------------------------------------------------------------------
def test_pages_beside_an_update_from_another_thread():
    """Every page is taken under the tree's mutex, so it shows the state before the update or the state after it, never
    a mixture: page i is the page an observer gets who resumes behind page i - 1 in one of the two states.  The update
    rewrites the leaf of EVERY key, so a single page already tells which state it saw."""
    rng = random.Random(10)
    keys = C.distinct_keys(rng, 64, 400)
    old, new = C.leaves_for(rng, keys), C.leaves_for(rng, keys)
    extra = C.leaves_for(rng, C.distinct_keys(rng, 64, 50))
    new.update(extra)
    tree = lib_tree(64)
    write(tree, old)
    states = [C.live(old), C.live(new)]
    started, errors = threading.Event(), []

    def updater():
        try:
            started.wait(10)
            write(tree, new)
        except BaseException as e:  # noqa: BLE001 - handed to the main thread
            errors.append(e)

    t = threading.Thread(target=updater)
    t.start()
    lo, seen, got = 0, [], []
    while True:
        page, more = tree.scan(lo, TOP64, 16)
        started.set()
        fits = [i for i, pairs in enumerate(states) if (page, more) == C.expected(pairs, lo, TOP64, 16)]
        assert fits, "a page that is neither the state before nor the state after"
        seen.append(fits)
        got += page
        if not more:
            break
        lo = page[-1][0] + 1
    t.join()
    assert not errors, errors
    # the states are ordered: once a page shows the new state, every later page does
    which = [f[-1] if len(f) == 1 else None for f in seen]
    firm = [w for w in which if w is not None]
    assert firm == sorted(firm)
    if firm and firm[0] == 1 and which[0] == 1:
        assert got == states[1]
    if firm and firm[-1] == 0:
        assert got == states[0]
    assert tree.scan() == (states[1], False)
    tree.close()


# ---- a plain-C consumer ------------------------------------------------------------------------------------------------------------
def test_c_consumer_pages_through_a_tree():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_scan")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_scan.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.splitlines() == [
        "key 0 leaf 11 0", "key 7 leaf 22 0", "page 0 n 2 more 1",
        "key 9223372036854775808 leaf 33 0", "key 9223372036854775809 leaf 44 1", "page 1 n 2 more 1",
        "key 18446744073709551615 leaf 55 0", "page 2 n 1 more 0", "cabi_scan ok"]
