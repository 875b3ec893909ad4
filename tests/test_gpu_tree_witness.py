"""Witness export of the library's persistent trees (sp_tree_witness, sp_tree_prove; include/starkperp.h) against the host
twin: starkperp.state.SparseMerkleTree on the C oracle hash (oracle/starkref.c), as in tests/test_gpu_state_batch.py.
The twin's own witness is checked from scratch in tests/test_tree_witness_cpu.py; here the library must return the
IDENTICAL objects for identical state, and the consumer's walk (witness_replay.replay_multi_update) must get through what
SharedState.apply_state_updates(..., facts=d) collects on the sp_state_batch route.  Every comparison is exact."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from oracle import ref_py as R
from witness_replay import oracle_hash, oracle_hash_many, replay_multi_update, witness_size

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.FIELD_PRIME
BAD_ARGUMENT = -3


def distinct_keys(rng, height, n, forced=()):
    out = set(forced)
    room = min(n, 1 << height)
    while len(out) < room:
        out.add(rng.randrange(1 << height))
    return sorted(out)


def key_sets(rng, height, leaves, large):
    """The witness key sets of one comparison: where the kernels can go wrong.  large: with the sets of 65, 257 and
    1025 keys (which kernel path they take does not depend on what the tree holds: once per state is not needed)."""
    top = (1 << height) - 1
    written = sorted(leaves)
    sets = {"both ends": [0, top]}
    if written:
        k = written[len(written) // 2]
        sets["n = 1"] = [k]
        sets["two siblings"] = [k & ~1, k | 1]
        # written keys, their siblings and keys that share a prefix of every length with a written one
        near = {w ^ (1 << b) for w in written[:6] for b in range(0, height, max(1, height // 7))}
        sets["written and unwritten with shared prefixes"] = sorted(set(written[:9]) | near)
    else:
        sets["n = 1"] = [rng.randrange(top + 1)]
    never = [k for k in distinct_keys(rng, height, 40) if k not in leaves]
    if never:
        sets["never written"] = never
    for n in (65, 257, 1025) if large else ():  # wave edge, block edge, the 1024-key tile of tree_level_nodes_kernel
        sets["n = %d" % n] = distinct_keys(rng, height, n, forced=written[:n // 2])
    return sets


def compare(lib_tree, twin, rng, leaves, what, large=False):
    assert lib_tree.root == twin.root, what
    for name, keys in key_sets(rng, lib_tree.height, leaves, large).items():
        got = lib_tree.witness(keys)
        assert got == twin.witness(keys), (what, name)
        assert got[-1][:3] == (lib_tree.height, 0, twin.root), (what, name)
        assert len(got) == witness_size(lib_tree.height, keys)
        shuffled = list(keys[:300]) + list(keys[:3])  # prove: any order, repeats
        rng.shuffle(shuffled)
        assert lib_tree.prove(shuffled) == twin.prove(shuffled), (what, name)
    assert lib_tree.witness([]) == [] and lib_tree.prove([]) == []


@pytest.mark.parametrize("height", [1, 3, 16, 64])
def test_library_witness_and_proofs_equal_the_twin_over_a_sequence_of_batches(height):
    from starkperp import state
    rng = random.Random(300 + height)
    lib_tree = state.LibrarySparseTree(height, 0)
    twin = state.SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    leaves = {}
    compare(lib_tree, twin, rng, leaves, "a tree never updated", large=True)
    # a rejected update (a leaf out of range) on the fresh tree: its table exists now and holds nothing
    with pytest.raises(AssertionError):
        lib_tree.update_arrays(np.array([0], dtype=np.uint64), np.array([[P & (2**64 - 1), 0, 0, P >> 192]], dtype=np.uint64))
    compare(lib_tree, twin, rng, leaves, "a fresh tree after a rejected update")
    top = (1 << height) - 1
    for r, n in enumerate((40, 7, 40)):
        forced = (0, top) if r == 0 else tuple(sorted(leaves)[:2]) + (sorted(leaves)[-1] ^ 1,)
        mods = {k: rng.randrange(1, P) for k in distinct_keys(rng, height, n, forced)}
        assert lib_tree.update(mods) == twin.update(mods)
        leaves.update(mods)
        compare(lib_tree, twin, rng, leaves, "after batch %d" % r, large=r == 1)
    # a rejected update on a tree that holds state: the witness shows the old state
    bad_keys = np.array(sorted(leaves)[:2], dtype=np.uint64)
    bad = np.array([[5, 0, 0, 0], [P & (2**64 - 1), 0, 0, P >> 192]], dtype=np.uint64)
    with pytest.raises(AssertionError):
        lib_tree.update_arrays(bad_keys, bad)
    compare(lib_tree, twin, rng, leaves, "after a rejected update")
    lib_tree.close()


def test_witness_after_the_slot_table_has_grown():
    """A fresh table has 2^16 slots and grows when an update could take it above half full (csrc/merkle.hip
    tree_reserve).  Two updates of 300 distinct keys write about 17 000 nodes each: the second one makes the table grow
    (rehash on the tree's stream, the old table retired).  The witness of the FIRST update's keys, written before the
    growth, equals the twin's."""
    from starkperp import state
    rng = random.Random(71)
    lib_tree = state.LibrarySparseTree(64, 0)
    twin = state.SparseMerkleTree(64, 0, hash_many=oracle_hash_many)
    batches = [distinct_keys(rng, 64, 300) for _ in range(2)]
    nodes = [len(keys) + witness_size(64, keys) for keys in batches]
    assert not set(batches[0]) & set(batches[1]) and sum(nodes) > 2**15, "the second update must need a larger table"
    leaves = {}
    for keys in batches:
        mods = {k: rng.randrange(1, P) for k in keys}
        assert lib_tree.update(mods) == twin.update(mods)
        leaves.update(mods)
    assert lib_tree.witness(batches[0]) == twin.witness(batches[0])
    mixed = batches[0][:50] + batches[1][:50] + [k ^ 1 for k in batches[0][:20]]
    assert lib_tree.witness(mixed) == twin.witness(mixed)
    assert lib_tree.prove(mixed) == twin.prove(mixed)
    lib_tree.close()


def test_proofs_on_both_sides_of_the_staging_limit_equal_their_two_halves():
    """sp_tree_prove moves (h + 1) 32 + 8 n + (n + n h) 32 bytes: through the tree's page-locked buffer up to 4 MiB, in
    direct copies above (csrc/context.hpp StagedTrip).  At height 64 that is 2080 + 2088 n: 2007 keys are the most that
    stage, 2008 are the fewest that do not (the sets above stop at 303).  Both calls must agree, key by key, with the
    proofs of the same keys asked for in two halves (staged, compared with the twin above)."""
    from starkperp import batch_np, state
    size = lambda n: 65 * 32 + 8 * n + (n + 64 * n) * 32
    assert size(2007) <= 4 << 20 < size(2008)
    rng = random.Random(2008)
    tree = state.LibrarySparseTree(64, 0)
    written = distinct_keys(rng, 64, 600)
    tree.update_arrays(np.array(written, dtype=np.uint64),
                       batch_np.felts_from_ints([rng.randrange(1, P) for _ in written]))
    keys = written + [k ^ 1 for k in written[:300]] + distinct_keys(rng, 64, 1108)
    rng.shuffle(keys)
    keys = np.array(keys[:2008], dtype=np.uint64)
    halves = [batch_np.tree_prove(tree, part) for part in (keys[:1004], keys[1004:])]
    leaves, siblings = (np.concatenate([h[i] for h in halves]) for i in (0, 1))
    assert len({row.tobytes() for row in leaves}) > 600  # written leaves are distinct, the others are the empty leaf
    for n in (2007, 2008):
        got_leaves, got_siblings = batch_np.tree_prove(tree, keys[:n])
        assert (got_leaves == leaves[:n]).all() and (got_siblings == siblings[:n]).all(), n
    tree.close()


# ---- the sp_state_batch route ------------------------------------------------------------------------
def oracle_position_hashes(positions):
    return [R.position_hash(p[0], p[1], list(p[2]), hash_function=oracle_hash) for p in positions]


def random_position(rng, n_assets):
    ids = sorted(rng.sample(range(1, 2**60), n_assets))
    assets = tuple((a, rng.randrange(-(2**63), 2**63), rng.randrange(-(2**63), 2**63)) for a in ids)
    return (rng.randrange(2**251), rng.randrange(-(2**63), 2**63), assets)


def test_state_batch_route_collects_the_same_facts_as_the_twin():
    from starkperp import state
    rng = random.Random(19)
    lib_state = state.SharedState(64, 64)
    twin = state.SharedState(64, 64, hash_many=oracle_hash_many, position_hashes=oracle_position_hashes)
    assert isinstance(lib_state.positions, state.LibrarySparseTree)
    empty = state.SharedState.EMPTY_POSITION
    pos_now, ord_now = {}, {}
    for r in range(2):
        pos_keys = distinct_keys(rng, 64, 9, forced=(0, 2**64 - 1) if r == 0 else tuple(sorted(pos_now)[:3]))
        ord_keys = distinct_keys(rng, 64, 12, forced=() if r == 0 else (sorted(ord_now)[0], sorted(ord_now)[1] ^ 1))
        pos = [(k, pos_now.get(k, empty), pos_now.get(k, empty) if i % 4 == 3 else random_position(rng, i % 4))
               for i, k in enumerate(pos_keys)]
        orders = [(k, ord_now.get(k, 0), rng.randrange(P)) for k in ord_keys]
        d_lib, d_twin = {}, {}
        roots = lib_state.apply_state_updates(pos, orders, facts=d_lib)
        assert roots == twin.apply_state_updates(pos, orders, facts=d_twin)
        assert d_lib == d_twin and d_lib
        prev_h, new_h = (oracle_position_hashes([u[j] for u in pos]) for j in (1, 2))
        replay_multi_update(64, roots[0][0], roots[0][1], {u[0]: (a, b) for u, a, b in zip(pos, prev_h, new_h)}, d_lib)
        replay_multi_update(64, roots[1][0], roots[1][1], {k: (a, b) for k, a, b in orders}, d_lib)
        pos_now.update({k: q for k, _, q in pos})
        ord_now.update({k: q for k, _, q in orders})
    # one previous-leaf mismatch: the batch fails on the device, nothing is committed, the dict stays
    before = dict(d_lib)
    k = sorted(pos_now)[0]
    stale = [(k, random_position(rng, 2), random_position(rng, 1))]
    roots_before = (lib_state.positions_root, lib_state.orders_root)
    with pytest.raises(AssertionError):
        lib_state.apply_state_updates(stale, [(sorted(ord_now)[0], ord_now[sorted(ord_now)[0]], 5)], facts=d_lib)
    assert d_lib == before and (lib_state.positions_root, lib_state.orders_root) == roots_before
    lib_state.close()


# ---- bad arguments through ctypes ----------------------------------------------------------------------
def test_bad_arguments_write_nothing_and_leave_the_tree():
    from starkperp import _lib, state
    lib = _lib.ensure_init()
    tree = state.LibrarySparseTree(16, 0)
    tree.update({3: 7, 400: 9, 65535: 11})
    root = tree.root
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def witness(handle, keys, capacity=None):
        keys = np.array(keys, dtype=np.uint64)
        cap = 64 if capacity is None else capacity
        level = np.full(64, 0xEE, dtype=np.uint8)
        arrays = [np.full(64, 0xA5A5, dtype=np.uint64)] + [np.full((64, 4), 0xA5A5, dtype=np.uint64) for _ in range(3)]
        count = ctypes.c_size_t(4242)
        rc = lib.sp_tree_witness(handle, ptr(keys), len(keys), cap, ptr(level), *[ptr(a) for a in arrays],
                                 ctypes.byref(count))
        untouched = (level == 0xEE).all() and all((a == 0xA5A5).all() for a in arrays)
        return rc, untouched, count.value

    def prove(handle, keys):
        keys = np.array(keys, dtype=np.uint64)
        leaves = np.full((len(keys), 4), 0xA5A5, dtype=np.uint64)
        siblings = np.full((len(keys), 16, 4), 0xA5A5, dtype=np.uint64)
        rc = lib.sp_tree_prove(handle, ptr(keys), len(keys), ptr(leaves), ptr(siblings))
        return rc, (leaves == 0xA5A5).all() and (siblings == 0xA5A5).all()

    good = [3, 400, 401]
    size = witness_size(16, good)
    assert witness(tree._handle, good) == (0, False, size)
    assert witness(tree._handle, [400, 3]) == (BAD_ARGUMENT, True, 4242), "unsorted keys"
    assert witness(tree._handle, [3, 3]) == (BAD_ARGUMENT, True, 4242), "a repeated key"
    assert witness(tree._handle, [3, 65536]) == (BAD_ARGUMENT, True, 4242), "a key out of range"
    assert witness(tree._handle, good, capacity=size - 1) == (BAD_ARGUMENT, True, size), "capacity one short"
    assert witness(987654, good) == (BAD_ARGUMENT, True, 4242), "an unknown handle"
    assert prove(tree._handle, [400, 3, 400]) == (0, False)
    assert prove(tree._handle, [3, 65536]) == (BAD_ARGUMENT, True), "a key out of range"
    assert prove(987654, good) == (BAD_ARGUMENT, True), "an unknown handle"
    assert tree.root == root
    handle = tree._handle
    tree.close()
    assert witness(handle, good) == (BAD_ARGUMENT, True, 4242), "a destroyed handle"
    assert prove(handle, good) == (BAD_ARGUMENT, True), "a destroyed handle"


# ---- two threads, one tree ---------------------------------------------------------------------------
def test_a_witness_beside_updates_always_describes_a_batch_boundary():
    from starkperp import state
    rng = random.Random(23)
    tree = state.LibrarySparseTree(64, 0)
    twin = state.SparseMerkleTree(64, 0, hash_many=oracle_hash_many)
    first = {k: rng.randrange(1, P) for k in distinct_keys(rng, 64, 20)}
    assert tree.update(first) == twin.update(first)
    fixed = sorted(first)[:6] + [sorted(first)[7] ^ 1, rng.randrange(2**64)]
    updates = [{k: rng.randrange(1, P) for k in rng.sample(sorted(first), 3) + distinct_keys(rng, 64, 2)}
               for _ in range(8)]
    roots, seen, errors = [tree.root], [], []
    done = threading.Event()

    def updater():
        try:
            for mods in updates:
                roots.append(tree.update(mods)[1])
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)
        finally:
            done.set()

    def reader():
        try:
            while True:
                last = done.is_set()
                seen.append(tree.witness(fixed))
                if last:
                    return
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=reader), threading.Thread(target=updater)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(roots) == 9 and len(set(roots)) == 9 and seen
    # the twin's witness at each of the nine batch boundaries: every witness seen is one of them, whole
    boundary = {twin.root: twin.witness(fixed)}
    for mods in updates:
        twin.update(mods)
        boundary[twin.root] = twin.witness(fixed)
    assert sorted(boundary) == sorted(roots)
    for wit in seen:
        assert wit[-1][2] in boundary and wit == boundary[wit[-1][2]]
    assert seen[-1] == boundary[roots[-1]]
    distinct = {rec for wit in seen for rec in wit}
    assert oracle_hash_many([r[3] for r in distinct], [r[4] for r in distinct]) == [r[2] for r in distinct]
    tree.close()


# ---- a plain-C caller ----------------------------------------------------------------------------------
def test_c_consumer_of_the_witness_export_runs():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_witness")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_witness.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "cabi_witness ok" in out.stdout
