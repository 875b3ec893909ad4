"""Witness export, the part that needs no GPU: sp_tree_witness_size (host arithmetic inside the library, callable before
sp_init), and the host twin - SparseMerkleTree.witness / prove, facts_of, proof_root and SharedState.apply_state_updates(
..., facts=d) - with the ORACLE hash plugged in (oracle/starkref.c through oracle.cref, spot-checked against
oracle.ref_py), as tests/test_state_tree_cpu.py plugs it in.

Expected values: witness_replay.node_values recomputes every node of a witness from scratch out of the written leaves;
witness_replay.replay_multi_update is the consumer - the walk of merkle_multi_update (state/state.cairo:155-173) from the
previous root and from the new root through nothing but the dictionary of preimages.  Every comparison is exact."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_py as R
from witness_replay import (check_witness, empties, layout, oracle_hash, oracle_hash_many, replay_multi_update,
                            witness_size)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.FIELD_PRIME
BAD_ARGUMENT = -3


def test_oracle_hash_is_the_reference_hash():
    assert oracle_hash(3, 4) == R.pedersen_hash(3, 4)
    assert oracle_hash_many([0, P - 1], [0, 5]) == [R.pedersen_hash(0, 0), R.pedersen_hash(P - 1, 5)]


# ---- sp_tree_witness_size --------------------------------------------------------------------------
def size_call(height, keys):
    from starkperp import _lib
    arr = np.array(keys, dtype=np.uint64)
    count = ctypes.c_size_t(12345)
    rc = _lib.load().sp_tree_witness_size(height, arr.ctypes.data_as(ctypes.c_void_p), len(keys), ctypes.byref(count))
    return rc, count.value


def key_sets(height):
    rng = random.Random(1000 + height)
    top = (1 << height) - 1
    sets = {"one key": [rng.randrange(top + 1)], "both ends": [0, top]}
    if top >= 7:
        sets["two siblings"] = [6, 7]
    # 1025 random keys, or every key of a tree that has fewer
    many = set()
    while len(many) < min(1025, top + 1):
        many.add(rng.randrange(top + 1))
    sets["1025 random"] = sorted(many)
    return sets


@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_witness_size_equals_the_count_of_distinct_prefixes(height):
    for name, keys in key_sets(height).items():
        assert size_call(height, keys) == (0, witness_size(height, keys)), name
    assert size_call(height, []) == (0, 0)


def test_witness_size_rejects_bad_keys_and_heights():
    for name, (height, keys) in {
        "a repeated key": (16, [3, 9, 9]),
        "a decreasing pair": (16, [3, 9, 8]),
        "a key equal to 2^h": (16, [3, 1 << 16]),
        "a key equal to 2^h, height 1": (1, [0, 2]),
        "height 0": (0, [0]),
        "height 65": (65, [0, 1]),
    }.items():
        assert size_call(height, keys) == (BAD_ARGUMENT, 12345), name


ORDER_TEXT = "keys must be strictly increasing"
RANGE_TEXT = "key out of range for height"


def test_key_check_edges_and_error_texts():
    """The library's one key check (order and range), reached through the caller that needs no device.  Every expectation
    is the definition: keys strictly increasing, every key below 2^height; a height-64 tree takes every 64-bit key."""
    from starkperp import _lib
    top64 = (1 << 64) - 1
    for name, (height, keys, text) in {
        "height 1, one key": (1, [1], None),
        "height 1, both keys": (1, [0, 1], None),
        "height 64, one key": (64, [top64], None),
        "height 64, the last two keys": (64, [top64 - 1, top64], None),
        "height 63, the last key": (63, [(1 << 63) - 1], None),
        "equal neighbours": (64, [5, 5], ORDER_TEXT),
        "equal neighbours, height 1": (1, [1, 1], ORDER_TEXT),
        "decreasing neighbours": (64, [0, top64, top64 - 1], ORDER_TEXT),
        "decreasing neighbours, height 1": (1, [1, 0], ORDER_TEXT),
        "2^h alone, height 1": (1, [2], RANGE_TEXT),
        "2^h behind valid keys, height 1": (1, [0, 1, 2], RANGE_TEXT),
        "2^h alone, height 63": (63, [1 << 63], RANGE_TEXT),
        "2^h behind a valid key, height 63": (63, [(1 << 63) - 1, 1 << 63], RANGE_TEXT),
    }.items():
        if text is None:
            assert size_call(height, keys) == (0, witness_size(height, keys)), name
        else:
            assert size_call(height, keys) == (BAD_ARGUMENT, 12345), name
            assert _lib.last_error() == text, name


def test_witness_size_runs_before_sp_init():
    """A process that never initialises the library (and could not: no device is asked for) gets the count."""
    code = ("import ctypes, sys\n"
            "sys.path.insert(0, %r)\n"
            "from starkperp import _lib\n"
            "lib = _lib.load()\n"
            "keys = (ctypes.c_uint64 * 3)(1, 2, 2**63)\n"
            "count = ctypes.c_size_t()\n"
            "assert lib.sp_is_initialised() == 0\n"
            "assert lib.sp_tree_witness_size(64, keys, 3, ctypes.byref(count)) == 0\n"
            "assert lib.sp_is_initialised() == 0\n"
            "print(count.value)\n" % os.path.join(ROOT, "stark-perpetual_amd"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout) == witness_size(64, [1, 2, 2**63]) == 3 + 2 * 62 + 1


# ---- the twin --------------------------------------------------------------------------------------
def three_batches(height, seed):
    """A twin after three batches (the third overwrites a key and writes a sibling of one), and what it holds."""
    from starkperp.state import SparseMerkleTree
    rng = random.Random(seed)
    tree = SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    top = (1 << height) - 1
    leaves = {}
    for r in range(3):
        mods = {rng.randrange(top + 1): rng.randrange(1, P) for _ in range(3)}
        if r == 0:
            mods[0], mods[top] = rng.randrange(1, P), rng.randrange(1, P)
        if r == 2:
            known = sorted(leaves)
            mods[known[1]] = rng.randrange(1, P)
            mods[known[2] ^ 1] = rng.randrange(1, P)
        tree.update(mods)
        leaves.update(mods)
    return tree, leaves, rng


@pytest.mark.parametrize("height", [3, 64])
def test_twin_witness_is_the_induced_subtree_in_layout_order(height):
    tree, leaves, rng = three_batches(height, 40 + height)
    top = (1 << height) - 1
    written = sorted(leaves)
    emp = empties(height, 0)
    never = [k for k in (5, top - 2, rng.randrange(top + 1)) if k not in leaves]
    assert never
    for keys in (written, written[:1], never, written[:2] + never + [written[0] ^ 1, written[-1] ^ 2]):
        wit = tree.witness(keys)
        check_witness(height, leaves, 0, keys, wit)  # order, every value from scratch, every record hashes
        assert wit[-1][:3] == (height, 0, tree.root)
    # unsorted input with repeats is sorted and made distinct first
    assert tree.witness([written[1], written[0], written[1]]) == tree.witness(written[:2])
    assert tree.witness([]) == []
    # never-written keys: below the point where their path leaves every written path, all three values are empty roots
    for key in never:
        wit = tree.witness([key])
        split = min((key ^ k).bit_length() for k in leaves)  # the level at which the path meets a written one
        assert 1 <= split <= height and len(wit) == height
        for level, idx, node, left, right in wit:
            if level < split:
                assert (node, left, right) == (emp[level], emp[level - 1], emp[level - 1])
            else:
                assert node != emp[level]


@pytest.mark.parametrize("height", [3, 64])
def test_twin_proofs_fold_to_the_root(height):
    from starkperp.state import proof_root
    tree, leaves, rng = three_batches(height, 60 + height)
    top = (1 << height) - 1
    absent = next(k for k in (top - 1, 3, 4, 2) if k not in leaves)
    keys = sorted(leaves) + [absent, 0, sorted(leaves)[1]]  # any order, a repeat
    proofs = tree.prove(keys)
    assert len(proofs) == len(keys)
    for key, (leaf, siblings) in zip(keys, proofs):
        assert leaf == leaves.get(key, 0) and len(siblings) == height
        assert proof_root(key, leaf, siblings, oracle_hash_many) == tree.root
    leaf, siblings = proofs[len(leaves)]
    assert leaf == 0 and proof_root(absent, 0, siblings, oracle_hash_many) == tree.root  # the empty leaf folds to the root
    assert proof_root(absent, 1, siblings, oracle_hash_many) != tree.root
    assert tree.prove([]) == []


# ---- sufficiency: what apply_state_updates(..., facts=d) collects is what the consumer needs -------------------
def position_hashes(positions):
    return [R.position_hash(p[0], p[1], list(p[2]), hash_function=oracle_hash) for p in positions]


EMPTY = (0, 0, ())
P1 = (123, 50, ((7, 1, -2),))
P2 = (123, 40, ((7, 1, 3),))
Q1 = (456, -9, ())


def replay_both(st_heights, roots, pos_mods, ord_mods, facts):
    (old_p, new_p), (old_o, new_o) = roots
    replay_multi_update(st_heights[0], old_p, new_p, pos_mods, facts)
    replay_multi_update(st_heights[1], old_o, new_o, ord_mods, facts)


@pytest.mark.parametrize("heights", [(8, 6), (64, 64)], ids=["h8_6", "h64_64"])
def test_facts_of_a_batch_replay_both_multi_updates(heights):
    from starkperp.state import SharedState
    st = SharedState(*heights, hash_many=oracle_hash_many, position_hashes=position_hashes)
    h = dict(zip((EMPTY, P1, P2, Q1), position_hashes([EMPTY, P1, P2, Q1])))
    top_p, top_o = (1 << heights[0]) - 1, (1 << heights[1]) - 1
    d = {}
    roots = st.apply_state_updates([(3, EMPTY, P1), (200, EMPTY, Q1), (3, P1, P2), (top_p, EMPTY, P1)],
                                   [(9, 0, 10), (9, 10, 25), (1, 0, 4), (top_o, 0, 7)], facts=d)
    pos_mods = {3: (h[EMPTY], h[P2]), 200: (h[EMPTY], h[Q1]), top_p: (h[EMPTY], h[P1])}
    ord_mods = {9: (0, 25), 1: (0, 4), top_o: (0, 7)}
    replay_both(heights, roots, pos_mods, ord_mods, d)
    assert all(oracle_hash(left, right) == node for node, (left, right) in d.items())
    # a second batch continues from the stored state: an overwritten key, an unchanged position, a sibling key
    d2 = {}
    roots2 = st.apply_state_updates([(200, Q1, Q1), (2, EMPTY, P1), (3, P2, P1)], [(1, 4, 6), (8, 0, 5)], facts=d2)
    pos_mods2 = {200: (h[Q1], h[Q1]), 2: (h[EMPTY], h[P1]), 3: (h[P2], h[P1])}
    ord_mods2 = {1: (4, 6), 8: (0, 5)}
    replay_both(heights, roots2, pos_mods2, ord_mods2, d2)
    assert roots2[0][0] == roots[0][1] and roots2[1][0] == roots[1][1]
    # a wrong expectation is noticed by the replay itself
    with pytest.raises(AssertionError):
        replay_both(heights, roots2, pos_mods2, {1: (4, 7), 8: (0, 5)}, d2)
    # every single fact is needed
    if heights == (8, 6):
        for node in list(d2):
            short = dict(d2)
            del short[node]
            with pytest.raises(KeyError):
                replay_both(heights, roots2, pos_mods2, ord_mods2, short)
    else:
        rng = random.Random(5)
        for node in rng.sample(sorted(d2), 12):
            short = dict(d2)
            del short[node]
            with pytest.raises(KeyError):
                replay_both(heights, roots2, pos_mods2, ord_mods2, short)
    # facts=None reads nothing back and returns the same roots as the twin fed with a dict
    other = SharedState(*heights, hash_many=oracle_hash_many, position_hashes=position_hashes)
    assert other.apply_state_updates([(3, EMPTY, P1), (200, EMPTY, Q1), (3, P1, P2), (top_p, EMPTY, P1)],
                                     [(9, 0, 10), (9, 10, 25), (1, 0, 4), (top_o, 0, 7)]) == roots


def test_a_failed_batch_leaves_the_facts_dict_as_it_was():
    """The failing second update of test_apply_state_updates_is_all_or_nothing, and its precondition failures."""
    from starkperp.state import SharedState
    st = SharedState(8, 6, hash_many=oracle_hash_many, position_hashes=position_hashes)
    d = {}
    st.apply_state_updates([(3, EMPTY, P1)], [(9, 0, 10)], facts=d)
    assert d
    before, roots = dict(d), (st.positions_root, st.orders_root)
    for bad_orders in ([(9, 10, 11), (9, 99, 12)], [(9, 7, 11)], [(9, 10, P)], [(1 << 6, 0, 1)]):
        with pytest.raises(AssertionError):
            st.apply_state_updates([(3, P1, P2)], bad_orders, facts=d)
        assert d == before and (st.positions_root, st.orders_root) == roots
    real_update = st.orders.update

    def failing_update(mods):
        raise AssertionError("Unhashable input.")
    st.orders.update = failing_update
    with pytest.raises(AssertionError):
        st.apply_state_updates([(3, P1, P2)], [(9, 10, 11)], facts=d)
    st.orders.update = real_update
    assert d == before and (st.positions_root, st.orders_root) == roots
    new = st.apply_state_updates([(3, P1, P2)], [(9, 10, 11)], facts=d)
    assert set(before) < set(d)
    h = position_hashes([P1, P2])
    replay_both((8, 6), new, {3: (h[0], h[1])}, {9: (10, 11)}, d)
