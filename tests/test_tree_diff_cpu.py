"""Clone, diff and delta of a persistent tree, the part that needs no GPU: the host twin state.SparseMerkleTree.clone /
diff / diff_items / delta / apply_delta with the ORACLE hash plugged in (witness_replay.oracle_hash_many), as
tests/test_tree_scan_cpu.py plugs it in.  The twin makes the descent sp_tree_diff makes on the device: a frontier per
level from the two roots, pruning by value, the cut after every step.

Expected values: the two plain dictionaries of what the test wrote into A and into B (tree_diff_cases.differing /
expected).  Every comparison is exact."""
import random

import pytest

import tree_diff_cases as D
from witness_replay import oracle_hash_many

P = D.P


def twin_of(height, empty_leaf=0):
    from starkperp import state
    return state.SparseMerkleTree(height, empty_leaf, hash_many=oracle_hash_many)


def check_queries(a, b, triples, what):
    for name, lo, hi, cap in D.queries(a.height, triples):
        assert a.diff(b, lo, hi, cap) == D.expected(triples, lo, hi, cap), (what, name, lo, hi, cap)
    assert a.diff(b) == (triples, False), what
    assert b.diff(a) == (D.swapped(triples), False), what
    assert list(a.diff_items(b, page=3)) == triples, what


# ---- 1. twin against the dictionaries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_diff_equals_the_dictionaries_over_a_sequence_of_batches(height):
    start, rounds = D.pair_batches(height, sizes=(40, 7, 40))
    a, b = twin_of(height), twin_of(height)
    assert a.diff(b) == ([], False)
    check_queries(a, b, [], "two trees never updated")
    a.update(start)
    in_a, in_b = dict(start), {}
    check_queries(a, b, D.differing(in_a, in_b), "one tree never updated")
    b.update(start)
    in_b.update(start)
    assert a.root == b.root
    check_queries(a, b, [], "equal trees")
    for r, (mods_a, mods_b) in enumerate(rounds):
        a.update(mods_a)
        b.update(mods_b)
        in_a.update(mods_a)
        in_b.update(mods_b)
        triples = D.differing(in_a, in_b)
        assert triples, r
        check_queries(a, b, triples, "after batch %d" % r)


def test_the_batches_play_every_role():
    """The case table itself: at a height with room, every batch overwrites a shared key with different values and one
    with the same value, resets a key in one tree only and writes a key in one tree only."""
    start, rounds = D.pair_batches(64)
    in_a, in_b = dict(start), dict(start)
    for mods_a, mods_b in rounds:
        both = set(mods_a) & set(mods_b)
        held = set(in_a) & set(in_b)
        assert any(k in held and mods_a[k] != mods_b[k] for k in both)
        assert any(k in held and mods_a[k] == mods_b[k] for k in both)
        assert any(v == 0 and k in held and k not in other for mods, other in ((mods_a, mods_b), (mods_b, mods_a))
                   for k, v in mods.items())
        assert any(k not in in_a and k not in in_b for k in set(mods_a) ^ set(mods_b))
        in_a.update(mods_a)
        in_b.update(mods_b)


# ---- 2. paging with capacity 1 ----------------------------------------------------------------------------------------
def test_pages_of_one_resume_inside_the_node_that_holds_the_previous_key():
    """Differing keys that are neighbours: after a page of one the next range starts at previous key + 1, inside the
    level-1 (and level-2, ...) node that also holds the previous key.  That node differs, sticks out of the range on
    the left and has no differing leaf IN range when the previous key was its last: a cut to `capacity` nodes alone
    would keep only it and return an empty page with `more` set.  tree_scan_cases.pages asserts that no page is empty
    while `more` is set."""
    height = 16
    keys = [8, 9, 10, 11, 13, 40, 41, 0x7fff, 0x8000, 0xffff]
    rng = random.Random(2)
    in_a = D.leaves_for(rng, keys + [100, 200])
    in_b = dict(in_a)
    in_b.update(D.leaves_for(rng, keys[:6]))  # other values
    for k in keys[6:]:
        del in_b[k]                           # absent from B
    a, b = twin_of(height), twin_of(height)
    a.update(in_a)
    b.update(in_b)
    triples = D.differing(in_a, in_b)
    assert [t[0] for t in triples] == keys
    for lo, hi in ((0, 0xffff), (9, 0x8000), (10, 41), (12, 12), (14, 39)):
        want = D.expected(triples, lo, hi)[0]
        for cap in (1, 2, 3):
            got, mores = D.pages(lambda l, h, c: a.diff(b, l, h, c), lo, hi, cap)
            assert got == want, (lo, hi, cap)
            assert mores == [True] * (max(-(-len(want) // cap), 1) - 1) + [False], (lo, hi, cap)


# ---- 3. reset by value; clone -----------------------------------------------------------------------------------------
def test_a_leaf_written_and_reset_equals_a_leaf_never_written():
    height = 16
    rng = random.Random(3)
    shared = D.leaves_for(rng, D.distinct_keys(rng, height, 12))
    a, b = twin_of(height), twin_of(height)
    a.update(shared)
    b.update(shared)
    k = next(k for k in range(1 << height) if k not in shared)
    a.update({k: 77})
    assert a.diff(b) == ([(k, 77, 0)], False) and b.diff(a) == ([(k, 0, 77)], False)
    a.update({k: 0})  # the path stays in A's store with empty-root values; B never had it
    assert a.root == b.root
    assert a.diff(b) == ([], False) and a.diff(b, k, k, 1) == ([], False)
    # ... and below a node that differs for another reason
    a.update({k ^ 1: 5})
    assert a.diff(b) == ([(k ^ 1, 5, 0)], False)
    assert a.diff(b, k, k) == ([], False)


@pytest.mark.parametrize("empty_leaf", [0, 7])
def test_clone_is_equal_and_independent(empty_leaf):
    height = 16
    rng = random.Random(33)
    written = D.leaves_for(rng, D.distinct_keys(rng, height, 20))
    tree = twin_of(height, empty_leaf)
    tree.update(written)
    copy = tree.clone()
    assert copy.root == tree.root and copy.scan() == tree.scan() and copy.empties == tree.empties
    assert tree.diff(copy) == ([], False)
    k = sorted(written)[5]
    copy.update({k: 123})
    assert tree.diff(copy) == ([(k, written[k], 123)], False)
    assert tree.get(k) == written[k] and tree.scan() == (sorted(written.items()), False)
    tree.update({k ^ 1: 9})
    assert copy.get(k ^ 1) == written.get(k ^ 1, empty_leaf)
    fresh = twin_of(height, empty_leaf).clone()
    assert fresh.root == fresh.empties[height] and fresh.scan() == ([], False)
    with pytest.raises(AssertionError):
        tree.diff(twin_of(height, empty_leaf + 1))
    with pytest.raises(AssertionError):
        tree.diff(twin_of(height - 1, empty_leaf))
    with pytest.raises(AssertionError):
        tree.diff(copy, 3, 2)
    with pytest.raises(AssertionError):
        tree.diff(copy, 0, 1 << height)
    with pytest.raises(AssertionError):
        tree.diff(copy, 0, 5, 0)


# ---- 4. delta ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [3, 64])
def test_delta_round_trip(height):
    start, rounds = D.pair_batches(height, sizes=(6, 3))
    base = twin_of(height)
    base.update(start)
    cur = base.clone()
    in_base, in_cur = dict(start), dict(start)
    for mods, _ in rounds:
        cur.update(mods)
        in_cur.update(mods)
    delta = cur.delta(base, page=2)
    triples = D.differing(in_cur, in_base)
    assert delta == {"height": height, "empty_leaf": 0, "base_root": base.root, "root": cur.root,
                     "keys": [k for k, _, _ in triples], "leaves": [v for _, v, _ in triples]}
    target = base.clone()
    assert target.apply_delta(delta, chunk=2) == (base.root, cur.root)
    assert target.root == cur.root and target.scan() == cur.scan() and target.diff(cur) == ([], False)
    # a tree that stands somewhere else: refused, nothing written
    elsewhere = base.clone()
    elsewhere.update({0: 4242})
    before = (elsewhere.root, elsewhere.scan())
    with pytest.raises(ValueError):
        elsewhere.apply_delta(delta)
    assert (elsewhere.root, elsewhere.scan()) == before
    for key, value in (("height", height + 1), ("empty_leaf", 1)):
        with pytest.raises(ValueError):
            base.clone().apply_delta(dict(delta, **{key: value}))
    # a delta whose leaves do not lead to its root: ValueError, and the tree holds the delta's leaves
    spoiled = dict(delta, leaves=[delta["leaves"][0] ^ 1] + delta["leaves"][1:])
    victim = base.clone()
    with pytest.raises(ValueError):
        victim.apply_delta(spoiled)
    assert victim.get(spoiled["keys"][0]) == spoiled["leaves"][0]
    # nothing changed: an empty delta
    same = base.clone().delta(base)
    assert (same["keys"], same["leaves"], same["root"]) == ([], [], base.root)
    assert base.clone().apply_delta(same) == (base.root, base.root)


def test_shared_state_fork_delta_and_apply_delta_on_the_host_route():
    from oracle import ref_py as R
    from starkperp.state import SharedState
    ph = lambda ps: [R.position_hash(p[0], p[1], list(p[2])) for p in ps]
    empty = (0, 0, ())
    p1, q1 = (123, 50, ((7, 1, -2),)), (456, -9, ())
    base = SharedState(8, 6, hash_many=oracle_hash_many, position_hashes=ph)
    base.apply_state_updates([(3, empty, p1)], [(9, 0, 10)])
    fork = base.fork()
    assert (fork.positions_root, fork.orders_root) == (base.positions_root, base.orders_root)
    roots = (base.positions_root, base.orders_root)
    fork.apply_state_updates([(3, p1, q1), (200, empty, p1)], [(9, 10, 11), (63, 0, 4)])
    assert (base.positions_root, base.orders_root) == roots  # the fork shares nothing mutable
    d = fork.delta(base)
    assert d["positions"]["keys"] == [3, 200] and d["positions"]["leaves"] == ph([q1, p1])
    assert (d["orders"]["keys"], d["orders"]["leaves"]) == ([9, 63], [11, 4])
    # a state that stands elsewhere in ONE tree: neither tree is written
    other = base.fork()
    other.apply_state_updates([], [(5, 0, 1)])
    before = (other.positions_root, other.orders_root)
    with pytest.raises(ValueError):
        other.apply_delta(d)
    assert (other.positions_root, other.orders_root) == before
    assert base.apply_delta(d) == ((roots[0], fork.positions_root), (roots[1], fork.orders_root))
    second = base.fork()
    step = ([(200, p1, q1)], [(63, 4, 5)])
    assert second.apply_state_updates(*step) == fork.apply_state_updates(*step)
