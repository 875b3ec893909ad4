"""Ordered range scan of a persistent tree, the part that needs no GPU: the host twin state.SparseMerkleTree.scan / items /
snapshot / restore with the ORACLE hash plugged in (witness_replay.oracle_hash_many), as tests/test_tree_witness_cpu.py
plugs it in.  The twin makes the descent sp_tree_scan makes on the device (frontier per level, pruning by value, the cut
after every step).

Expected values: the plain dictionary of what the test wrote (tree_scan_cases.live / expected).  Every comparison is
exact.  The states stay at a few hundred oracle hashes each."""
import random

import pytest

import tree_scan_cases as C
from witness_replay import oracle_hash_many

P = C.P


def twin_of(height, empty_leaf=0):
    from starkperp import state
    return state.SparseMerkleTree(height, empty_leaf, hash_many=oracle_hash_many)


def check_queries(tree, pairs, what):
    for name, lo, hi, cap in C.queries(tree.height, pairs):
        assert tree.scan(lo, hi, cap) == C.expected(pairs, lo, hi, cap), (what, name, lo, hi, cap)
    assert tree.scan() == (pairs, False), what


@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_scan_equals_the_dictionary_over_a_sequence_of_batches(height):
    tree = twin_of(height)
    assert tree.scan() == ([], False)
    check_queries(tree, [], "a tree never updated")
    written = {}
    for r, mods in enumerate(C.batches(height, sizes=(6, 3, 6))):
        tree.update(mods)
        written.update(mods)
        check_queries(tree, C.live(written), "after batch %d" % r)


@pytest.mark.parametrize("height", [16, 64])
def test_bounds_are_inclusive_at_both_ends_of_the_key_range(height):
    top = (1 << height) - 1
    a, b = 5 << (height - 8), 9 << (height - 6)
    written = C.leaves_for(random.Random(height), [0, a, a + 1, b, top])
    tree = twin_of(height)
    tree.update(written)
    pairs = C.live(written)
    assert [k for k, _ in pairs] == [0, a, a + 1, b, top]
    assert tree.scan(a, a) == ([(a, written[a])], False)                 # lo == hi on a written key
    assert tree.scan(a + 2, a + 2) == ([], False)                       # ... and on an unwritten key
    assert tree.scan(a + 1, b - 1) == ([(a + 1, written[a + 1])], False)  # lo just above a written key, hi just below one
    assert tree.scan(a + 2, b - 1) == ([], False)
    assert tree.scan(0, 0) == ([(0, written[0])], False)
    assert tree.scan(top, top) == ([(top, written[top])], False)
    assert tree.scan(0, top) == (pairs, False) and tree.scan() == (pairs, False)
    assert tree.scan(1, top - 1) == (pairs[1:-1], False)
    assert tree.scan(0, top, 4) == (pairs[:4], True) and tree.scan(0, top, 5) == (pairs, False)
    with pytest.raises(AssertionError):
        tree.scan(3, 2)
    with pytest.raises(AssertionError):
        tree.scan(0, top + 1)
    with pytest.raises(AssertionError):
        tree.scan(0, top, 0)


@pytest.mark.parametrize("empty_leaf", [0, 12345])
def test_leaves_set_back_to_the_empty_leaf_are_pruned_by_value(empty_leaf):
    """40 leaves written, 39 set back to the empty leaf, the LARGEST key kept: the paths of the 39 are still in the
    facts store.  A descent that followed every node it finds would fill a page of 1 with dead nodes."""
    height = 16
    rng = random.Random(40)
    written = C.leaves_for(rng, C.distinct_keys(rng, height, 40))
    tree = twin_of(height, empty_leaf)
    tree.update(written)
    largest = max(written)
    reset = {k: empty_leaf for k in written if k != largest}
    tree.update(reset)
    written.update(reset)
    assert C.live(written, empty_leaf) == [(largest, written[largest])]
    assert tree.scan(capacity=1) == ([(largest, written[largest])], False)
    assert tree.scan() == ([(largest, written[largest])], False)
    tree.update({largest: empty_leaf})
    assert tree.scan() == ([], False) and tree.scan(capacity=1) == ([], False)
    assert tree.root == tree.empties[height]


def test_pages_concatenate_to_the_dictionary_and_more_is_exact():
    height, n = 16, 23
    rng = random.Random(23)
    written = C.leaves_for(rng, C.distinct_keys(rng, height, n, (0, (1 << height) - 1)))
    tree = twin_of(height)
    tree.update(written)
    pairs = C.live(written)
    calls = []
    scan = tree.scan
    tree.scan = lambda lo=0, hi=None, capacity=None: (calls.append((lo, hi, capacity)), scan(lo, hi, capacity))[1]
    for cap in (1, 7, n - 1, n, n + 1):
        got, mores = C.pages(scan, 0, (1 << height) - 1, cap)
        assert got == pairs, cap
        # `more` is exact, so no call is needed to find out that the last page was the last
        assert mores == [True] * (-(-n // cap) - 1) + [False], cap
        del calls[:]
        assert list(tree.items(page=cap)) == pairs, cap
        assert len(calls) == -(-n // cap), cap
        assert [c[0] for c in calls] == [0] + [pairs[i * cap - 1][0] + 1 for i in range(1, len(calls))], cap
    lo, hi = pairs[3][0], pairs[17][0]
    assert list(tree.items(lo, hi, page=4)) == pairs[3:18]
    assert list(tree.items(pairs[3][0] + 1, pairs[4][0] - 1)) == []


@pytest.mark.parametrize("height", [3, 64])
def test_snapshot_restores_to_the_same_root_and_scan(height):
    from starkperp import state
    tree = twin_of(height, 9)
    written = {}
    for mods in C.batches(height, sizes=(5, 3)):
        mods = {k: (v or 9) for k, v in mods.items()}  # this tree's empty leaf is 9: the reset writes 9
        tree.update(mods)
        written.update(mods)
    snap = tree.snapshot()
    pairs = C.live(written, 9)
    assert snap == {"height": height, "empty_leaf": 9, "root": tree.root, "keys": [k for k, _ in pairs],
                    "leaves": [v for _, v in pairs]}
    # by hand on a fresh twin: updates in ascending chunks
    fresh = twin_of(height, snap["empty_leaf"])
    for at in range(0, len(pairs), 2):
        fresh.update(dict(zip(snap["keys"][at:at + 2], snap["leaves"][at:at + 2])))
    assert fresh.root == tree.root and fresh.scan() == tree.scan() == (pairs, False)
    again = state.SparseMerkleTree.restore(snap, oracle_hash_many, chunk=3)
    assert again.root == tree.root and again.scan() == (pairs, False)
    spoiled = dict(snap, leaves=[snap["leaves"][0] ^ 1] + snap["leaves"][1:])
    with pytest.raises(ValueError):
        state.SparseMerkleTree.restore(spoiled, oracle_hash_many)


def test_shared_state_snapshot_and_restore_on_the_host_route():
    """SharedState with an injected hash keeps host twins: snapshot after one batch, restore, equal roots and scans, and
    the restored state goes on where the first one stands."""
    from oracle import ref_py as R
    from starkperp.state import SharedState
    ph = lambda ps: [R.position_hash(p[0], p[1], list(p[2])) for p in ps]
    one = SharedState(8, 6, hash_many=oracle_hash_many, position_hashes=ph)
    empty = (0, 0, ())
    p1, q1 = (123, 50, ((7, 1, -2),)), (456, -9, ())
    one.apply_state_updates([(3, empty, p1), (200, empty, q1)], [(9, 0, 10), (63, 0, 4)])
    snap = one.snapshot()
    assert snap["positions"]["keys"] == [3, 200] and snap["positions"]["leaves"] == ph([p1, q1])
    assert (snap["orders"]["keys"], snap["orders"]["leaves"]) == ([9, 63], [10, 4])
    two = SharedState.restore(snap, hash_many=oracle_hash_many, position_hashes=ph)
    assert (two.positions_root, two.orders_root) == (one.positions_root, one.orders_root)
    assert two.positions.scan() == one.positions.scan() and two.orders.scan() == one.orders.scan()
    step = ([(200, q1, p1)], [(9, 10, 11)])
    assert two.apply_state_updates(*step) == one.apply_state_updates(*step)
    snap["orders"]["leaves"][0] += 1
    with pytest.raises(ValueError):
        SharedState.restore(snap, hash_many=oracle_hash_many, position_hashes=ph)
