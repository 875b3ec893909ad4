"""sp_order_batch (include/starkperp.h, csrc/merkle.hip; verifier: verify_batch_keyed_gated of csrc/ecdsa.hip) against
the cases of tests/order_batch_cases.py, whose every expectation is integers on the oracle: message hashes, verdict
bytes, both roots, the status byte, and what the tree holds afterwards (sp_tree_root, sp_tree_get at the order ids,
sp_tree_scan).  Every call runs under a watchdog: a way out of the call that leaves the verifier thread at its gate
would hang the caller."""
import ctypes
import threading

import numpy as np
import pytest

import order_batch_cases as C

pytestmark = pytest.mark.gpu
WATCHDOG_SECONDS = 60


def guarded(fn):
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001 - the outcome is inspected by the caller
            box["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(WATCHDOG_SECONDS)
    assert not t.is_alive(), "sp_order_batch did not return: the verifier was left at its gate"
    return box


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def direct(call, handle, with_status=True, depth=None, id_shift=None, n=None):
    """lib.sp_order_batch itself -> (rc, z, verdicts, old root, new root, status byte or None)."""
    from starkperp import _lib
    words, r, s, qx, qy, leaves = call.arrays()
    n = call.n if n is None else n
    z = np.zeros((max(call.n, 1), 4), dtype=np.uint64)
    verdicts = np.full(max(call.n, 1), 0xEE, dtype=np.uint8)
    old, new = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    st = np.full(1, 0xEE, dtype=np.uint8)
    lib = _lib.ensure_init()
    out = guarded(lambda: lib.sp_order_batch(_ptr(words), call.depth if depth is None else depth, n, _ptr(r), _ptr(s),
                                             _ptr(qx), _ptr(qy), handle, _ptr(leaves),
                                             call.id_shift if id_shift is None else id_shift, _ptr(z), _ptr(verdicts),
                                             _ptr(old), _ptr(new), _ptr(st) if with_status else None))
    assert "error" not in out, out
    return (out["value"], C.ints_of(z)[:call.n], verdicts.tolist()[:call.n], C.ints_of(old)[0], C.ints_of(new)[0],
            int(st[0]) if with_status else None)


def new_tree(case):
    from starkperp import state
    tree = state.LibrarySparseTree(case.height, case.empty_leaf)
    if case.seed:
        tree.update(case.seed)
    assert tree.root == case.seed_root
    return tree


def check_tree(tree, case, call):
    """The tree holds exactly call.after: root, the leaves at the call's ids, the ordered scan."""
    assert tree.root == call.new_root
    if call.ids is not None:
        ids = [i for i in call.ids if i < 2**case.height]
        assert tree.get_many(ids) == [call.after.get(i, case.empty_leaf) for i in ids]
    items, more = tree.scan(capacity=4096)
    assert not more and items == sorted((k, v) for k, v in call.after.items() if v != case.empty_leaf)


def check_call(tree, case, call):
    """One call through batch_np.order_batch (and through the library itself where order_batch raises) against its
    expectation."""
    from starkperp import batch_np as bn
    from starkperp._lib import StarkPerpError
    words, r, s, qx, qy, leaves = call.arrays()
    out = guarded(lambda: bn.order_batch(words, r, s, qx, tree, leaves, qy=qy, id_shift=call.id_shift))
    if call.rc == C.OK and call.status in (0, C.NOT_COMMITTED):
        assert "error" not in out, (call.note, out)
        z, verdicts, old, new, committed = out["value"]
        assert C.ints_of(z) == call.z
        assert verdicts.dtype == np.uint8 and verdicts.tolist() == call.verdicts
        assert (old, new, bool(committed)) == (call.old_root, call.new_root, call.committed), call.note
        assert committed or old == new
    elif call.rc == C.OK:  # a hash status: order_batch raises signature.py's assertion, the call itself tells more
        assert isinstance(out.get("error"), AssertionError), (call.note, out)
        rc, z, verdicts, old, new, status = direct(call, tree._handle)
        assert (rc, status) == (C.OK, call.status), call.note
        assert verdicts == call.verdicts, call.note
        assert old == new == call.old_root == call.new_root
        assert call.z is None or z == call.z
    else:
        assert isinstance(out.get("error"), StarkPerpError), (call.note, out)
        rc = direct(call, tree._handle)[0]
        assert rc == call.rc
    check_tree(tree, case, call)


def run_case(case):
    tree = new_tree(case)
    try:
        for call in case.calls:
            check_call(tree, case, call)
    finally:
        tree.close()


# ---- the families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_shift", C.ID_SHIFTS)
def test_id_window(id_shift):
    """Depth 1, crafted hashes: the window all zeros / all ones / single bits at both ends with the bits outside it
    set - a wrong shift, a dropped or misplaced carry or a 63-bit window writes some leaf at another key."""
    run_case(C.id_window_case(id_shift))


@pytest.mark.parametrize("pattern,n", C.SORT_SHAPES, ids=["%s-%d" % s for s in C.SORT_SHAPES])
def test_sort_shape(pattern, n):
    """Skewed and extreme id patterns at the sizes where the bucket count steps; the leaves are pairwise distinct, so
    a leaf that does not follow its id through the sort shows in sp_tree_get."""
    run_case(C.sort_case(pattern, n))


@pytest.mark.parametrize("where,n", C.DUPLICATES, ids=["%s-%d" % d for d in C.DUPLICATES])
def test_duplicate_ids_are_refused_and_the_next_batch_commits(where, n):
    run_case(C.duplicate_case(where, n))


@pytest.mark.parametrize("id_shift,height", C.DEPTH_TREES, ids=["shift%d-height%d" % t for t in C.DEPTH_TREES])
@pytest.mark.parametrize("kind", C.DEPTH_KINDS)
def test_chain_depths(kind, id_shift, height):
    run_case(C.depth_case(kind, id_shift, height))


@pytest.mark.parametrize("height", C.LOW_HEIGHTS)
def test_low_trees_take_ids_that_fit_and_refuse_one_that_does_not(height):
    run_case(C.low_tree_case(height))


@pytest.mark.parametrize("xonly", (False, True), ids=("points", "xonly"))
@pytest.mark.parametrize("which", C.VERDICT_BATCHES)
def test_verdict_codes(which, xonly):
    """Every verdict code out of this call, through both of its verification paths: a batch with a hash of 2^251 or
    more is verified without the thread ("codes"), every other one on the verifier thread."""
    run_case(C.verdict_batch(which, xonly))


def test_leaf_values_and_leaves_out_of_range():
    run_case(C.leaves_case())


def test_words_out_of_range():
    run_case(C.words_case())


def test_history_on_one_tree():
    """Commit, overwrite, refuse, refuse after the slot table has grown, commit: old root == previous new root
    throughout, and the refused growth loses nothing."""
    from starkperp import batch_np as bn
    case = C.history_case(0)
    tree = new_tree(case)
    try:
        sizes = []  # (entries, slots) of the node table after every call
        for call in case.calls:
            check_call(tree, case, call)
            sizes.append(bn.tree_table_size(tree))
        assert [sl for _, sl in sizes] == [C.TABLE_SLOTS] * 3 + [sizes[3][1]] * 2 and sizes[3][1] > C.TABLE_SLOTS, sizes
        # one entry per node position ever written: overwritten and refused batches add none, the rehash loses none
        assert [e for e, _ in sizes] == [C.node_count(64, list(call.after)) for call in case.calls], sizes
    finally:
        tree.close()


def test_two_histories_at_once_on_two_trees():
    """Two threads, a tree each, the key cache and the verifier's lanes shared: each reaches its own oracle roots."""
    cases = [C.history_case(0), C.history_case(1)]
    errors = {}

    def run(case):
        try:
            run_case(case)
        except BaseException as e:  # noqa: BLE001 - reported below
            errors[case.name] = e
    threads = [threading.Thread(target=run, args=(c,), daemon=True) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join(4 * WATCHDOG_SECONDS)
    assert not any(t.is_alive() for t in threads), "a history did not finish"
    assert not errors, errors


def test_key_cache_reset_between_batches():
    """The all-valid batch straight after sp_ecdsa_key_cache_reset, again with its keys registered, again after
    another reset: the same verdicts and roots each time (a fresh tree each time)."""
    from starkperp import batch
    for xonly in (False, True):
        case = C.verdict_batch("repeated", xonly)
        for reset in (True, False, True):
            if reset:
                batch.key_cache_reset()
            run_case(case)


# ---- arguments ------------------------------------------------------------------------------------------------------
def test_argument_edges_and_null_status():
    case = C.small_good_case()
    call = case.calls[0]
    tree = new_tree(case)
    try:
        ghost = 987654  # a handle the library never issued
        for what, kw, handle in (("depth 0", {"depth": 0}, tree._handle), ("id_shift 193", {"id_shift": 193}, tree._handle),
                                 ("unknown handle, n = 0", {"n": 0}, ghost), ("unknown handle, n = 4", {}, ghost)):
            rc = direct(call, handle, **kw)[0]
            assert rc == C.BAD_ARGUMENT, what
            assert tree.root == case.seed_root and tree.get_many(call.ids) == [0] * call.n, what
        # id_shift 192 is the last legal one; n = 0 on a real tree is legal: nothing to verify, nothing to write
        rc, _, _, old, new, status = direct(call, tree._handle, n=0)
        assert (rc, status, old, new) == (C.OK, 0, case.seed_root, case.seed_root)
        # tree_status == NULL: legal, and the batch commits
        rc, z, verdicts, old, new, status = direct(call, tree._handle, with_status=False)
        assert (rc, status, z, verdicts) == (C.OK, None, call.z, call.verdicts)
        assert (old, new) == (call.old_root, call.new_root)
        check_tree(tree, case, call)
        # ... and a refusal without a status byte still shows as old == new
        bad = C.Call(call.words, list(zip(call.r, [call.s[0], call.s[1] ^ 8] + call.s[2:])), call.keys,
                     [v ^ 1 for v in call.leaves])
        C.expect(bad, case.height)
        assert bad.status == C.NOT_COMMITTED and sum(v != 1 for v in bad.verdicts) == 1
        rc, _, verdicts, old, new, _ = direct(bad, tree._handle, with_status=False)
        assert (rc, verdicts, old, new) == (C.OK, bad.verdicts, call.new_root, call.new_root)
        check_tree(tree, case, call)
    finally:
        tree.close()
