"""sp_merkle_verify_update[_dev] (include/starkperp.h) against its host twin, starkperp.state.verify_update_records on the
C oracle hash, over the shared case table (tests/witness_update_cases.py): witnesses from LibrarySparseTree.witness before
and after `update`, every tamper of the table, the consistent forgery.  The library must return the twin's verdict and
the twin's 2 R status bytes, which are also the bytes the table derives from the positions.  Every comparison is exact."""
import ctypes
import random
import threading

import numpy as np
import pytest

import witness_update_cases as W
from witness_replay import oracle_hash, oracle_hash_many, replay_multi_update

pytestmark = pytest.mark.gpu
BAD_ARGUMENT = -3
_built = {}


def built(name):
    """(instance, arrays) of a case on the library's tree, built once and never changed: arrays = the node, left, right
    felts of both halves, uint64[2 R, 4] each."""
    from starkperp import batch_np, state
    if name not in _built:
        inst, tree = W.build(W.CASES[name], lambda h, e: state.LibrarySparseTree(h, e))
        tree.close()
        records = inst.before + inst.after
        _built[name] = (inst, tuple(batch_np.felts_from_ints([rec[i] for rec in records]) for i in (2, 3, 4)))
    return _built[name]


def arrays_of(t, inst, base):
    """The record arrays of `t`, a changed clone of `inst`: rows of the records that were replaced are packed anew."""
    from starkperp import batch_np
    out = [a.copy() for a in base]
    for h in (0, 1):
        for u, (mine, theirs) in enumerate(zip(t.half(h), inst.half(h))):
            if mine is not theirs:
                for a, value in zip(out, mine[2:5]):
                    a[h * inst.records + u] = batch_np.felts_from_ints([value])[0]
    return out


def call_args(t, arrays):
    from starkperp import batch_np
    felts = batch_np.felts_from_ints
    return (np.array(t.keys, dtype=np.uint64), felts(t.prev_leaves), felts(t.new_leaves), felts([t.prev_root]),
            felts([t.new_root])) + tuple(arrays)


def library(t, arrays):
    """batch_np.merkle_verify_update with the halves of `arrays` standing for tree_witness's tuples."""
    from starkperp import batch_np
    keys, prev, new, prev_root, new_root, node, left, right = call_args(t, arrays)
    r = t.records
    halves = [(None, None, node[h * r:(h + 1) * r], left[h * r:(h + 1) * r], right[h * r:(h + 1) * r]) for h in (0, 1)]
    verdict, status = batch_np.merkle_verify_update(t.height, keys, prev, new, prev_root, new_root, *halves)
    assert status.shape == (2, r) and status.dtype == np.uint8
    return verdict, status.tolist()


def library_dev(t, arrays, with_status=True):
    """sp_merkle_verify_update_dev on a side stream with torch tensors; keys and roots (host) are scribbled over as soon
    as the call returns.  The verdict byte sits in the middle of a word whose other bytes must survive."""
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    keys, prev, new, prev_root, new_root, node, left, right = call_args(t, arrays)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    d_prev, d_new, d_node, d_left, d_right = (dev(a) for a in (prev, new, node, left, right))
    d_status = torch.full((2 * t.records,), 0xEE, dtype=torch.uint8, device="cuda")
    d_verdict = torch.full((8,), 0x77, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.stream(side):
        _lib.check(lib.sp_merkle_verify_update_dev(
            t.height, ptr(keys), len(t.keys), d_prev.data_ptr(), d_new.data_ptr(), ptr(prev_root), ptr(new_root),
            d_node.data_ptr(), d_left.data_ptr(), d_right.data_ptr(), t.records, d_verdict.data_ptr() + 5,
            d_status.data_ptr() if with_status else None, side.cuda_stream), "sp_merkle_verify_update_dev")
    keys[:] = 0
    prev_root[:] = 0
    new_root[:] = 0
    side.synchronize()
    word = d_verdict.cpu().tolist()
    assert word[:5] == [0x77] * 5 and word[6:] == [0x77] * 2 and word[5] in (0, 1)
    status = d_status.cpu().numpy().reshape(2, t.records)
    if not with_status:
        assert (status == 0xEE).all()
    return word[5] == 1, status.tolist()


def twin(t):
    from starkperp import state
    return state.verify_update_records(t.height, t.keys, t.prev_leaves, t.new_leaves, t.prev_root, t.new_root, t.before,
                                       t.after, oracle_hash_many)


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_an_honest_update_verifies_on_both_entry_points(name):
    inst, base = built(name)
    assert library(inst, base) == twin(inst) == (True, inst.clean())
    assert library_dev(inst, base) == (True, inst.clean())
    assert library_dev(inst, base, with_status=False)[0] is True


@pytest.mark.parametrize("name", W.TAMPERED)
def test_every_tamper_gives_the_twins_bytes(name):
    inst, base = built(name)
    for i, (what, t, want) in enumerate(W.tampers(inst)):
        arrays = arrays_of(t, inst, base)
        got = library(t, arrays)
        assert got == (False, want), (name, what)
        assert got == twin(t), (name, what)
        if i % 7 == 0:  # the device entry point on every seventh: each kind of tamper gets its turn
            assert library_dev(t, arrays) == got, (name, what)
            assert library_dev(t, arrays, with_status=False)[0] is False, (name, what)


@pytest.mark.parametrize("name", W.FORGED)
def test_a_consistent_forgery_fails_on_the_sibling_check_alone(name):
    from starkperp import state
    inst, base = built(name)

    def make(h, e):
        make.tree = state.LibrarySparseTree(h, e)
        return make.tree

    forged, want = W.forge(W.CASES[name], inst, make)
    make.tree.close()
    arrays = arrays_of(forged, inst, base)
    got = library(forged, arrays)
    assert got == (False, want) and got == twin(forged)
    assert library_dev(forged, arrays) == got
    facts = state.facts_of(forged.before + forged.after)
    mods = {k: (a, b) for k, a, b in zip(forged.keys, forged.prev_leaves, forged.new_leaves)}
    assert state.verify_multi_update(facts, forged.height, forged.prev_root, forged.new_root, mods) is False
    honest = state.facts_of(inst.before + inst.after)
    assert state.verify_multi_update(honest, inst.height, inst.prev_root, inst.new_root, mods) is True


def test_witnesses_above_the_staging_limit_go_up_in_direct_copies():
    """The host call moves 3 (2 R 32) + 2 n 32 + 4 + 2 R bytes: through the lane's page-locked buffer up to 4 MiB, in
    direct copies above (csrc/context.hpp StagedTrip).  Case D (R about 1.7 x 10^4) stays below; 400 random keys at
    height 64 have R >= 21 850 and cross.  Witnesses straight from sp_tree_witness before and after one update: the
    verdict is true and every status byte 0; one felt of one record flipped: false, and that record is flagged."""
    from starkperp import batch_np, state
    rng = random.Random(400)
    tree = state.LibrarySparseTree(64, 0)
    tree.update({rng.randrange(2**64): rng.randrange(1, W.P) for _ in range(300)})
    keys = np.array(sorted({rng.randrange(2**64) for _ in range(400)}), dtype=np.uint64)
    n, records = len(keys), batch_np.tree_witness_size(64, keys)
    assert 3 * (2 * records * 32) + 2 * n * 32 + 4 + 2 * records > 4 << 20
    prev = batch_np.felts_from_ints(tree.get_many(keys.tolist()))
    new = batch_np.felts_from_ints([rng.randrange(1, W.P) for _ in range(n)])
    before = batch_np.tree_witness(tree, keys)
    prev_root, new_root = tree.update_arrays(keys, new)
    after = batch_np.tree_witness(tree, keys)
    tree.close()
    verdict, status = batch_np.merkle_verify_update(64, keys, prev, new, prev_root, new_root, before, after)
    assert verdict is True and status.shape == (2, records) and not status.any()
    u = records // 3
    after[2][u, 0] ^= np.uint64(1)  # the node value of one record of the after half
    verdict, status = batch_np.merkle_verify_update(64, keys, prev, new, prev_root, new_root, before, after)
    assert verdict is False and status[1, u] != 0 and not status[0].any()


def test_bad_arguments_write_nothing_and_no_keys_compare_the_roots():
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    inst, base = built("B")
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def host(height=inst.height, keys=inst.keys, n_records=inst.records, roots=None, n=None, null=None):
        keys_a, prev, new, prev_root, new_root, node, left, right = call_args(inst, base)
        keys_a = np.array(keys, dtype=np.uint64)
        if roots is not None:
            prev_root, new_root = (np.array([[r, 0, 0, 0]], dtype=np.uint64) for r in roots)
        verdict = np.full(4, 0xEE, dtype=np.uint8)
        status = np.full(2 * inst.records + 2, 0xEE, dtype=np.uint8)
        args = [ptr(keys_a), len(keys_a) if n is None else n, ptr(prev), ptr(new), ptr(prev_root), ptr(new_root), ptr(node),
                ptr(left), ptr(right), n_records, ptr(verdict), ptr(status)]
        if null is not None:
            args[null] = None
        rc = lib.sp_merkle_verify_update(height, *args)
        return rc, verdict.tolist(), bool((status == 0xEE).all())

    untouched = [0xEE] * 4
    assert host() == (0, [1, 0xEE, 0xEE, 0xEE], False)
    assert host(keys=inst.keys[::-1]) == (BAD_ARGUMENT, untouched, True), "keys not increasing"
    assert host(keys=inst.keys[:-1] + [inst.keys[-2]]) == (BAD_ARGUMENT, untouched, True), "a repeated key"
    assert host(keys=inst.keys[:-1] + [8]) == (BAD_ARGUMENT, untouched, True), "a key out of range"
    assert host(n_records=inst.records - 1) == (BAD_ARGUMENT, untouched, True), "n_records one short"
    assert host(n_records=inst.records + 1) == (BAD_ARGUMENT, untouched, True), "n_records one over"
    assert host(height=0) == (BAD_ARGUMENT, untouched, True) and host(height=65) == (BAD_ARGUMENT, untouched, True)
    for null in (0, 2, 3, 4, 5, 6, 7, 8, 10):  # every pointer but status
        assert host(null=null) == (BAD_ARGUMENT, untouched, True), null
    # n == 0: the verdict says whether the roots are equal, nothing else is read or written
    assert host(n=0, n_records=0, roots=(5, 5)) == (0, [1, 0xEE, 0xEE, 0xEE], True)
    assert host(n=0, n_records=0, roots=(5, 6)) == (0, [0, 0xEE, 0xEE, 0xEE], True)
    assert host(n=0, n_records=1, roots=(5, 5)) == (BAD_ARGUMENT, untouched, True)
    # the _dev call validates the same way, before anything is enqueued
    keys_a, prev, new, prev_root, new_root, node, left, right = call_args(inst, base)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    d_prev, d_new, d_node, d_left, d_right = (dev(a) for a in (prev, new, node, left, right))
    d_verdict = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2 * inst.records,), 0xEE, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def device(height=inst.height, keys=keys_a, n=len(inst.keys), n_records=inst.records, roots=(prev_root, new_root)):
        rc = lib.sp_merkle_verify_update_dev(height, ptr(keys), n, d_prev.data_ptr(), d_new.data_ptr(), ptr(roots[0]),
                                             ptr(roots[1]), d_node.data_ptr(), d_left.data_ptr(), d_right.data_ptr(),
                                             n_records, d_verdict.data_ptr(), d_status.data_ptr(), stream)
        torch.cuda.synchronize()
        return rc, d_verdict.cpu().tolist(), bool((d_status == 0xEE).all().item())

    assert device(keys=np.ascontiguousarray(keys_a[::-1])) == (BAD_ARGUMENT, untouched, True)
    assert device(n_records=inst.records + 1) == (BAD_ARGUMENT, untouched, True)
    assert device(height=0) == (BAD_ARGUMENT, untouched, True) and device(height=65) == (BAD_ARGUMENT, untouched, True)
    assert device(n=0, n_records=0, roots=(prev_root, new_root)) == (0, [0, 0xEE, 0xEE, 0xEE], True)
    assert device(n=0, n_records=0, roots=(prev_root, prev_root)) == (0, [1, 0xEE, 0xEE, 0xEE], True)
    assert device() == (0, [1, 0xEE, 0xEE, 0xEE], False)


def test_update_checked_audits_its_own_update():
    from starkperp import state
    case = W.CASES["C"]
    tree = state.LibrarySparseTree(case.height, case.empty_leaf)
    twin_tree = state.SparseMerkleTree(case.height, case.empty_leaf, hash_many=oracle_hash_many)
    assert tree.update_checked({}) == twin_tree.update({})
    assert tree.update_checked(case.initial) == twin_tree.update(case.initial)
    assert tree.update_checked(case.modifications) == twin_tree.update(case.modifications)
    assert tree.root == twin_tree.root
    tree.close()


def test_shared_state_checks_the_facts_it_collects():
    """The small two-tree batch of tests/test_gpu_tree_witness.py on the sp_state_batch route with check_facts=True: the
    same roots and the same dict as the twin's, and the consumer's walk gets through it."""
    from oracle import ref_py as R
    from starkperp import state
    rng = random.Random(19)
    hashes = lambda positions: [R.position_hash(p[0], p[1], list(p[2]), hash_function=oracle_hash) for p in positions]

    def position(n_assets):
        ids = sorted(rng.sample(range(1, 2**60), n_assets))
        return (rng.randrange(2**251), rng.randrange(-(2**63), 2**63),
                tuple((a, rng.randrange(-(2**63), 2**63), rng.randrange(-(2**63), 2**63)) for a in ids))

    lib_state = state.SharedState(64, 64)
    twin_state = state.SharedState(64, 64, hash_many=oracle_hash_many, position_hashes=hashes)
    assert isinstance(lib_state.positions, state.LibrarySparseTree)
    empty = state.SharedState.EMPTY_POSITION
    pos_now, ord_now = {}, {}
    for r in range(2):
        pos_keys = sorted({rng.randrange(2**64) for _ in range(7)} | ({0, 2**64 - 1} if r == 0 else set(sorted(pos_now)[:3])))
        ord_keys = sorted({rng.randrange(2**64) for _ in range(11)} | (set() if r == 0 else {sorted(ord_now)[0]}))
        pos = [(k, pos_now.get(k, empty), pos_now.get(k, empty) if i % 4 == 3 else position(i % 4))
               for i, k in enumerate(pos_keys)]
        orders = [(k, ord_now.get(k, 0), rng.randrange(W.P)) for k in ord_keys]
        d_lib, d_twin = {}, {}
        roots = lib_state.apply_state_updates(pos, orders, facts=d_lib, check_facts=True)
        assert roots == twin_state.apply_state_updates(pos, orders, facts=d_twin, check_facts=True)
        assert d_lib == d_twin and d_lib
        replay_multi_update(64, roots[1][0], roots[1][1], {k: (a, b) for k, a, b in orders}, d_lib)
        assert state.verify_multi_update(d_lib, 64, roots[1][0], roots[1][1], {k: (a, b) for k, a, b in orders}) is True
        pos_now.update({k: q for k, _, q in pos})
        ord_now.update({k: q for k, _, q in orders})
    # an orders-only batch: the positions tree has no keys, its statement is old root == new root
    k = sorted(ord_now)[1]
    roots = lib_state.apply_state_updates([], [(k, ord_now[k], 77)], facts=d_lib, check_facts=True)
    assert roots[0][0] == roots[0][1] and roots[1][0] != roots[1][1]
    lib_state.close()


def test_four_threads_verify_at_once():
    inst, base = built("D")
    forged_inst = inst.clone()
    u = inst.records // 2
    forged_inst.after[u] = inst.after[u][:2] + ((inst.after[u][2] + 1) % W.P,) + inst.after[u][3:]
    jobs = [(inst, base), (forged_inst, arrays_of(forged_inst, inst, base))] * 2
    expected = [library(t, arrays) for t, arrays in jobs[:2]] * 2
    assert expected[0] == (True, inst.clean()) and expected[1][0] is False
    results, errors = [None] * 4, []
    barrier = threading.Barrier(4)

    def run(i):
        try:
            barrier.wait()
            for _ in range(3):
                results[i] = library(*jobs[i])
                assert results[i] == expected[i]
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results == expected
