"""The cases of tests/order_batch_cases.py checked against the pure-Python oracle and against themselves, without a
GPU: what tests/test_gpu_order_batch.py expects of sp_order_batch is only as good as these."""
import random

import pytest

import order_batch_cases as C
from oracle import ref_py as R

P = C.P


def c_hash(a, b):
    return C.hash_many([a], [b])[0][0]


# ---- roots ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,empty_leaf,n", [(1, 0, 1), (1, 5, 2), (8, 0, 7), (8, 12345, 9), (64, 0, 12), (64, P - 1, 5)])
def test_level_by_level_root_is_the_oracles_multi_update(height, empty_leaf, n):
    rng = random.Random("root-%d-%d" % (height, n))
    top = (1 << height) - 1
    keys = {0, top} if n >= 2 else {top}
    while len(keys) < n:
        keys.add(rng.randrange(top + 1))
    if height > 1 and n >= 4:
        keys = set(list(keys)[:n - 1]) | {min(keys) ^ 1}  # a sibling pair that is both written
    mods = {k: rng.randrange(P) for k in keys}
    assert C.sparse_root(height, mods, empty_leaf) == R.merkle_multi_update_sparse(height, mods, empty_leaf, c_hash)
    assert C.sparse_root(height, {}, empty_leaf) == R.empty_subtree_roots(height, empty_leaf, c_hash)[height]


def test_the_c_hash_is_the_python_hash_on_a_small_tree():
    mods = {0: 3, 1: P - 1, 6: 2**251}
    assert C.sparse_root(3, mods, 9) == R.merkle_multi_update_sparse(3, mods, 9)  # ref_py.pedersen_hash throughout


# ---- signatures and verdicts ----------------------------------------------------------------------------------------
def test_integer_signer_is_ref_py_sign_from_its_nonce_on():
    rng = random.Random("signer")
    ds, pts = C.signers(8)
    zs = [1, C.BOUND - 1] + [rng.randrange(C.BOUND) for _ in range(6)]
    sigs = C.sign_many(zs, ds, rng)
    for z, d, pt, (r, s) in list(zip(zs, ds, pts, sigs))[:4]:
        assert pt == R.private_key_to_ec_point_on_stark_curve(d)
        assert R.verify(z, r, s, pt) and R.verify(z, r, s, pt[0])
    assert C.cref.verify_codes(zs, [a for a, _ in sigs], [b for _, b in sigs], pts) == [1] * 8
    # the nonce ref_py.sign would have drawn gives ref_py.sign's signature
    k = R.generate_k_rfc6979(zs[3], ds[3])
    assert C.sign_with_nonce(zs[3], ds[3], k, R.ec_mult(k, tuple(R.EC_GEN))[0]) in (R.sign(zs[3], ds[3]), None)


@pytest.mark.parametrize("which", ("repeated", "distinct"))
def test_both_oracles_agree_on_the_valid_batches(which):
    """cref.verify_codes (point keys) against ref_py.verify (the integer key) on the two all-valid batches: 64
    signatures.  The other families verify under cref.verify_codes alone (ref_py.verify takes 40 ms a signature)."""
    points, xonly = C.verdict_batch(which, False).calls[0], C.verdict_batch(which, True).calls[0]
    assert points.verdicts == xonly.verdicts == [1] * 32 and points.committed and xonly.committed
    assert points.z == xonly.z and points.r == xonly.r and points.keys == xonly.keys
    assert len(set(points.keys)) == (4 if which == "repeated" else 32)


@pytest.mark.parametrize("which", ("codes", "codes-signed"))
def test_verdict_cases_carry_the_codes_their_labels_say(which):
    points, xonly = C.verdict_batch(which, False), C.verdict_batch(which, True)
    cp, cx = points.calls[0], xonly.calls[0]
    assert points.labels == xonly.labels and len(points.labels) == (9 if which == "codes" else 8)
    for pos in range(cp.n):
        lab = points.labels.get(pos)
        if lab is None:
            assert cp.verdicts[pos] == cx.verdicts[pos] == 1, pos
            continue
        want = C.CODE_LABELS[lab]
        if want is not None:
            assert cp.verdicts[pos] == want, (pos, lab)
        # x-only keys: an x on no curve point is False, not an assertion; the other labels keep their code; -y is
        # the same key
        assert cx.verdicts[pos] == {"off curve": 0, "y negated": 1}.get(lab, want), (pos, lab)
        if lab == "y negated":
            assert cp.verdicts[pos] == 0 and R.is_point_on_curve(*cp.keys[pos])
            assert not R.verify(cp.z[pos], cp.r[pos], cp.s[pos], cp.keys[pos])
        if lab == "off curve":
            assert not R.is_point_on_curve(*cp.keys[pos]) and not R.is_valid_stark_key(cp.keys[pos][0])
        if lab == "w >= 2^251":
            assert 1 <= cp.s[pos] < C.EC_ORDER and R.inv_mod_curve_size(cp.s[pos]) >= C.BOUND
        if lab == "z >= 2^251":
            assert C.BOUND <= cp.z[pos] < P
    codes = set(cp.verdicts)
    assert codes == ({0, 1, 2, 3, 4, 5, 6} if which == "codes" else {0, 1, 2, 3, 4, 6})
    for call in (cp, cx):
        assert (call.status, call.committed, call.rc) == (C.NOT_COMMITTED, False, C.OK)
        assert call.before == call.after and call.old_root == call.new_root


@pytest.mark.parametrize("which,pos", (("first", 0), ("last", 31)))
def test_single_bad_signature_at_either_end(which, pos):
    for xonly in (False, True):
        call = C.verdict_batch(which, xonly).calls[0]
        assert call.verdicts == [0 if i == pos else 1 for i in range(32)] and call.status == C.NOT_COMMITTED


# ---- message hashes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.DEPTH_KINDS)
def test_folded_hashes_are_the_python_oracles(kind):
    words, args = C.depth_words(kind)
    z, st = C.fold_words(words)
    assert not any(st) and len(z) == 64 and all(v < C.BOUND for v in z)
    for i in (0, 37, 63):
        acc = words[0][i]
        for row in words[1:]:
            acc = R.pedersen_hash(acc, row[i])
        assert z[i] == acc
    if args:
        assert len(words) == 5 and z[5] == R.get_limit_order_msg(*args[5])
    for id_shift, height in C.DEPTH_TREES:
        call = C.depth_case(kind, id_shift, height).calls[0]
        assert call.committed and call.z == z and all(i < 2**height for i in call.ids)


# ---- order ids ------------------------------------------------------------------------------------------------------
def mutant_id(name, z, id_shift):
    zw = [(z >> (64 * j)) & C.MASK64 for j in range(4)]
    if name == "shift + 1":
        id_shift += 1
    elif name == "shift - 1":
        id_shift -= 1
    w, sh = id_shift >> 6, id_shift & 63
    v = zw[w] >> sh
    if sh and w + 1 < 4 and name != "carry dropped":
        v |= (zw[w + 1] << ((63 if name == "carry shifted by 63 - sh" else 64) - sh)) & C.MASK64
    if name == "top bit masked off":
        v &= 2**63 - 1
    return v


MUTANTS = ("shift + 1", "shift - 1", "carry dropped", "carry shifted by 63 - sh", "top bit masked off")
# (mutant, shift) pairs at which the mutant computes the same id for EVERY message hash below 2^251, or is no
# extraction at all - nothing can separate it there:
#   shift - 1 at 0           there is no shift -1
#   the carry mutants        at 0, 64, 128, 192 the window starts on a word boundary: sh == 0, no carry is taken
#   top bit masked off       from 188 on the window's bit 63 lies at bit 251 or above, which no signed message has
NOT_SEPARABLE = {("shift - 1", 0)} | {(m, s) for m in ("carry dropped", "carry shifted by 63 - sh") for s in (0, 64, 128, 192)} \
    | {("top bit masked off", s) for s in (188, 191, 192)}


def case_kinds(id_shift):
    return C.id_window_case(id_shift).kinds


def window_kind(i, id_shift):
    """What the window of an order holds, from its true id alone: nearly empty, nearly full, or neither."""
    ones = bin(i).count("1")
    return "sparse" if ones <= 2 else "dense" if ones >= C.window_bits(id_shift) - 1 else "random"


def test_id_extraction_restated_equals_the_integer_window_on_every_case():
    for id_shift in C.ID_SHIFTS:
        call = C.id_window_case(id_shift).calls[0]
        assert call.committed and call.n == 12 and call.depth == 1
        assert call.ids == [C.c_order_id(z, id_shift) for z in call.z]
        assert call.ids == [mutant_id(None, z, id_shift) for z in call.z]
        a = C.window_bits(id_shift)
        assert case_kinds(id_shift) == [window_kind(i, id_shift) for i in call.ids]
        assert {0, 1, (1 << a) - 1, 1 << (a - 1)} <= set(call.ids)  # all zeros, all ones, a single bit at each end
        below, above = id_shift - 1, id_shift + 64  # the bits just outside the window, set beside an empty window
        assert id_shift == 0 or any((z >> below) & 1 and i == 0 for z, i in zip(call.z, call.ids))
        assert above >= 251 or any((z >> above) & 1 and i == 0 for z, i in zip(call.z, call.ids))
    rng = random.Random("ids")
    for id_shift in range(193):
        for z in [rng.randrange(C.BOUND) for _ in range(20)] + [C.BOUND - 1, 0]:
            assert C.c_order_id(z, id_shift) == (z >> id_shift) & C.MASK64


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_id_mutant_changes_an_id_at_every_shift_where_it_can(mutant):
    """A mutant must show twice at every shift: on an order whose window is nearly empty (a spurious or misplaced
    bit) and on one whose window is nearly full (a missing bit) - so that catching it does not hang on what random
    bits happen to be.  Where it is listed as not separable it must really agree on every hash tried."""
    rng = random.Random("mutants")
    for id_shift in C.ID_SHIFTS:
        case = C.id_window_case(id_shift)
        call = case.calls[0]
        if (mutant, id_shift) in NOT_SEPARABLE:
            if mutant == "shift - 1":
                continue
            for z in call.z + [rng.randrange(C.BOUND) for _ in range(200)] + [C.BOUND - 1]:
                assert mutant_id(mutant, z, id_shift) == C.c_order_id(z, id_shift)
            continue
        caught = {window_kind(i, id_shift) for z, i in zip(call.z, call.ids) if mutant_id(mutant, z, id_shift) != i}
        assert {"sparse", "dense"} <= caught, (mutant, id_shift, caught)


# ---- sort shapes, duplicates, low trees -------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,n", C.SORT_SHAPES)
def test_sort_shapes_are_unsorted_with_distinct_leaves(pattern, n):
    call = C.sort_case(pattern, n).calls[0]
    assert call.n == n and call.committed and call.status == 0 and call.verdicts == [1] * n
    assert len(set(call.leaves)) == n and len(set(call.ids)) == n
    if n >= 2:
        assert call.ids != sorted(call.ids)
    if pattern == "top16":
        assert len({i >> 48 for i in call.ids}) == 1
    if pattern == "descending":
        assert call.ids == sorted(call.ids, reverse=True)
    if pattern == "extremes":
        assert {0, C.MASK64} <= set(call.ids)
    if pattern == "adjacent":
        assert sum(1 for i in call.ids if i ^ 1 in call.ids) >= n - 3
        assert n < 3 or any(i + 1 in call.ids and i % 2 for i in call.ids)  # neighbours that are no siblings, too
    assert call.after == {**call.before, **dict(zip(call.ids, call.leaves))}


@pytest.mark.parametrize("where,n", C.DUPLICATES)
def test_duplicate_cases_hold_one_pair_and_differ_below_the_window(where, n):
    bad, good = C.duplicate_case(where, n).calls
    assert (bad.rc, good.rc, good.committed) == (C.BAD_ARGUMENT, C.OK, True) and bad.before == bad.after
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if bad.ids[i] == bad.ids[j]]
    assert pairs == [{"ends": (0, n - 1), "front": (0, 1), "middle": (n // 2 - 1, n // 2 + 1)}[where]]
    assert len(set(bad.z)) == n
    if where == "middle":
        assert len({i >> 48 for i in bad.ids}) == 1


@pytest.mark.parametrize("height", C.LOW_HEIGHTS)
def test_low_tree_cases(height):
    fits, over, again = C.low_tree_case(height).calls
    assert fits.committed and again.committed and {0, 2**height - 1} <= set(fits.ids)
    assert over.rc == C.BAD_ARGUMENT and sum(1 for i in over.ids if i >= 2**height) == 1 and over.before == over.after
    assert again.old_root == fits.new_root != again.new_root


# ---- leaves, words, history ---------------------------------------------------------------------------------------------
def test_leaf_and_word_cases_follow_the_pinned_rules():
    calls = C.leaves_case().calls
    assert [(c.status, c.committed) for c in calls] == [(0, True), (1, False), (1, False), (1, False), (0, True)]
    assert calls[1].verdicts == [1] * 8 and calls[2].verdicts == [1, 1, 1, 1, 1, 0, 1, 1]
    assert {12345, P - 1, 0} <= set(calls[0].leaves) and calls[3].leaves[2] == 2**256 - 1
    assert calls[1].old_root == calls[3].new_root == calls[0].new_root != calls[4].new_root
    calls = C.words_case().calls
    assert [(c.status, c.committed) for c in calls] == [(1, False), (1, False), (0, True), (0x80, False), (0x80, False),
                                                        (0x80, False), (0, True)]
    assert calls[0].verdicts == calls[1].verdicts == [0] * 8 and calls[0].z is None
    assert calls[3].verdicts == calls[4].verdicts == calls[5].verdicts == [1, 1, 1, 1, 1, 1, 5, 1]
    assert calls[5].rc == C.OK and calls[5].z[0] >> 187 == calls[5].z[1] >> 187 and calls[5].leaves[2] == P


def test_history_grows_the_table_only_in_the_refused_call():
    for case in (C.history_case(0),):
        calls = case.calls
        assert [(c.status, c.committed, c.n) for c in calls] == [(0, True, 64), (0, True, 64), (0x80, False, 64),
                                                                 (0x80, False, C.GROWTH_ORDERS), (0, True, 64)]
        assert calls[0].ids == calls[1].ids and calls[0].leaves != calls[1].leaves
        assert sum(v != 1 for v in calls[2].verdicts) == 1 == sum(v != 1 for v in calls[3].verdicts)
        for prev, call in zip(calls, calls[1:]):
            assert call.old_root == prev.new_root
        assert calls[0].old_root == case.seed_root and len(calls[-1].after) == 50 + 64 + 64
        # an update grows the table when the nodes it holds (an upper bound: every committed update's nodes) and
        # the update's own would fill more than half of it - refused or not, the decision comes afterwards
        held = C.node_count(64, list(case.seed))
        for k, call in enumerate(calls):
            need = C.node_count(64, call.ids)
            if k == 3:
                assert 2 * need > C.TABLE_SLOTS  # on its own account, whatever the tree held
            else:
                assert 2 * (held + need) <= C.TABLE_SLOTS, k
            if call.committed:
                held += need
