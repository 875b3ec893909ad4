"""The host side of the Merkle path calls, without a GPU: the yardstick of tests/test_gpu_merkle_paths.py (the oracle
fold of tests/merkle_path_cases.py) against an oracle-built tree, the arguments the NumPy binding builds for the
uniform and the ragged form, and the argument validation that is pure Python."""
import random

import numpy as np
import pytest

import merkle_path_cases as cases
from witness_replay import oracle_hash_many

P = cases.P


@pytest.mark.parametrize("height", [1, 3, 64])
def test_oracle_fold_of_a_twin_trees_proofs_is_its_root(height):
    from starkperp.state import SparseMerkleTree, proof_root
    rng = random.Random(height)
    tree = SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    written = sorted({rng.randrange(1 << height) for _ in range(12)})
    tree.update({k: rng.randrange(1, P) for k in written})
    keys = written + [rng.randrange(1 << height) for _ in range(6)] + written[:2]
    proofs = tree.prove(keys)
    items = [(k, leaf, sib) for k, (leaf, sib) in zip(keys, proofs)]
    assert cases.oracle_roots(items) == [tree.root] * len(keys)
    # the batched fold is the fold of state.proof_root
    assert cases.oracle_roots(items[:3]) == [proof_root(k, leaf, sib, oracle_hash_many) for k, leaf, sib in items[:3]]
    # and the twin's own verify, which folds with its hash_many
    assert tree.verify(keys, proofs) == [True] * len(keys)
    bad = [(leaf, list(sib)) for leaf, sib in proofs]
    bad[1][1][height // 2] ^= 2
    bad[2] = (bad[2][0] ^ 4, bad[2][1])
    bad[3] = (bad[3][0], bad[3][1] + [0])           # a sibling too many
    bad[4] = (P, bad[4][1])                         # not a field element
    bad_keys = list(keys)
    bad_keys[5] = 1 << height                       # outside the tree
    assert tree.verify(bad_keys, bad) == [i not in (1, 2, 3, 4, 5) for i in range(len(keys))]
    old_root = tree.root
    tree.update({written[0]: 12345})
    assert tree.root != old_root
    assert tree.verify(keys[:1], proofs[:1]) == [False]


def test_pool_items_are_distinct_and_stable():
    for length in (0, 1, 3, 64):
        items = cases.pool(length)
        assert len(items) == 31 and all(len(s) == length and 0 <= k < (1 << length) for k, _, s in items)
        assert len({leaf for _, leaf, _ in items}) == 31
        assert cases.pool(length) is items
    assert cases.oracle_roots(cases.pool(0)) == [leaf for _, leaf, _ in cases.pool(0)]
    assert cases.ragged_lengths(9) == [0, 64, 1, 0, 17, 2, 64, 0, 3]


def test_uniform_and_ragged_arguments_agree():
    from starkperp import batch_np
    items = cases.batch_of([3] * 40)
    leaves, sib, off, keys = cases.arrays(items)
    lv_u, sib_u, off_u, h_u, k_u = batch_np.merkle_path_args(leaves, sib.reshape(40, 3, 4), keys, height=3)
    lv_r, sib_r, off_r, h_r, k_r = batch_np.merkle_path_args(leaves, sib, keys, offsets=off)
    assert off_u is None and h_u == 3 and h_r == 0
    assert (batch_np.uniform_path_offsets(40, 3) == off_r).all() and off_r.dtype == np.uint32
    assert (lv_u == lv_r).all() and (sib_u == sib_r).all() and (k_u == k_r).all()
    assert sib_u.shape == (120, 4) and sib_u.flags["C_CONTIGUOUS"] and k_u.dtype == np.uint64
    # the largest uniform batch of height-64 paths whose offsets fit 32 bits
    off = batch_np.uniform_path_offsets(3, 64)
    assert list(off) == [0, 64, 128, 192]
    # height 0: no siblings at all
    lv, sib0, off0, h0, _ = batch_np.merkle_path_args(leaves, np.zeros((0, 4), dtype=np.uint64), np.zeros(40, dtype=np.uint64),
                                                     height=0)
    assert sib0.shape == (0, 4) and off0 is None and h0 == 0


def test_python_side_validation():
    from starkperp import batch, batch_np, state
    leaves, sib, off, keys = cases.arrays(cases.batch_of([2, 0, 5]))
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib, keys)                          # neither height nor offsets
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib, keys, height=2, offsets=off)   # both
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib, keys[:2], offsets=off)         # keys of another length
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib, keys, offsets=off[:3])         # n offsets
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib[:6], keys, offsets=off)         # offsets[n] != rows
    with pytest.raises(AssertionError):
        batch_np.merkle_path_args(leaves, sib, keys, height=65)
    with pytest.raises(ValueError):
        batch_np.merkle_path_args(leaves, sib, keys, height=3)                # 7 rows are not 3 x 3
    with pytest.raises(AssertionError):
        batch_np.merkle_verify_paths(leaves, sib, keys, np.zeros((2, 4), dtype=np.uint64), offsets=off)  # 2 roots for 3
    # the list API asserts before it reaches the library
    with pytest.raises(AssertionError):
        batch.merkle_fold_paths([4], [(1, [2, 3])])          # key bit 2 for a path of two siblings
    with pytest.raises(AssertionError):
        batch.merkle_fold_paths([0], [(1, [2] * 65)])        # a path longer than 64
    with pytest.raises(AssertionError):
        batch.merkle_fold_paths([0], [(P, [])])
    with pytest.raises(AssertionError):
        batch.merkle_fold_paths([0], [(1, [P])])
    with pytest.raises(AssertionError):
        batch.merkle_fold_paths([0, 1], [(1, [2])])
    assert batch.merkle_fold_paths([], []) == [] and state.proof_roots_many([], []) == []
    empty = batch_np.merkle_fold_paths(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
                                       np.zeros(0, dtype=np.uint64), height=64)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0,)
