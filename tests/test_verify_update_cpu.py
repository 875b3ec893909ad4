"""The host twin of sp_merkle_verify_update (starkperp.state.verify_update_records) on the shared case table
(tests/witness_update_cases.py), every hash through the C oracle (oracle/starkref.c).  The expected status bytes come
from the case table, which derives them from the records' positions; the verdict is also held against the consumer's
walk (witness_replay.replay_multi_update) plus a hash check of every record.  tests/test_gpu_verify_update.py holds the
library to this twin byte for byte.  No GPU."""
import pytest

import witness_update_cases as W
from witness_replay import oracle_hash_many, replay_multi_update

_built = {}


def built(name):
    """(instance, tree) of a case on the host twin, built once and never changed."""
    from starkperp import state
    if name not in _built:
        _built[name] = W.build(W.CASES[name], lambda h, e: state.SparseMerkleTree(h, e, hash_many=oracle_hash_many))
    return _built[name]


def twin(inst):
    from starkperp import state
    return state.verify_update_records(inst.height, inst.keys, inst.prev_leaves, inst.new_leaves, inst.prev_root,
                                       inst.new_root, inst.before, inst.after, oracle_hash_many)


def consumer_accepts(inst):
    """merkle_multi_update's walk through the union of the two witnesses, and every record a true preimage."""
    from starkperp import state
    records = inst.before + inst.after
    if any(not (0 <= v < W.P) for rec in records for v in rec[3:5]):
        return False
    if oracle_hash_many([rec[3] for rec in records], [rec[4] for rec in records]) != [rec[2] for rec in records]:
        return False
    facts = state.facts_of(records)
    mods = {k: (a, b) for k, a, b in zip(inst.keys, inst.prev_leaves, inst.new_leaves)}
    try:
        replay_multi_update(inst.height, inst.prev_root, inst.new_root, mods, facts)
    except (AssertionError, KeyError):
        return False
    return True


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_an_honest_update_verifies_with_every_byte_zero(name):
    from starkperp import state
    inst, _ = built(name)
    assert inst.records == len(inst.before) == len(inst.after)
    verdict, status = twin(inst)
    assert verdict is True and status == inst.clean()
    assert consumer_accepts(inst)
    # the reference's dictionary, walked from both roots, gives the records back in witness order
    for root, wit in ((inst.prev_root, inst.before), (inst.new_root, inst.after)):
        assert state.records_from_facts(state.facts_of(wit), root, inst.height, inst.keys) == wit
    facts = state.facts_of(inst.before + inst.after)
    mods = {k: (a, b) for k, a, b in zip(inst.keys, inst.prev_leaves, inst.new_leaves)}
    assert state.verify_multi_update(facts, inst.height, inst.prev_root, inst.new_root, mods,
                                     hash_many=oracle_hash_many) is True
    missing = dict(facts)
    del missing[inst.before[0][2]]
    with pytest.raises(KeyError):
        state.records_from_facts(missing, inst.prev_root, inst.height, inst.keys)


@pytest.mark.parametrize("name", W.TAMPERED)
def test_every_tamper_raises_exactly_its_bits(name):
    inst, _ = built(name)
    tampers = W.tampers(inst)
    for what, t, want in tampers:
        verdict, status = twin(t)
        assert status == want, (name, what)
        assert verdict is False, (name, what)
        assert consumer_accepts(t) is False, (name, what)
    bits = {b for _, _, want in tampers for half in want for b in half}
    for bit in (W.OUT_OF_RANGE, W.HASH_MISMATCH, W.LINK_MISMATCH, W.ROOT_MISMATCH):
        assert any(b & bit for b in bits), "no tamper of %s raises bit 0x%02x" % (name, bit)
    if name != "A2":  # with both keys of a height-1 tree modified there is no side off a path
        assert any(b & W.SIBLING_CHANGED for b in bits)
    assert verdict_of_clean_is_unchanged(inst)


def verdict_of_clean_is_unchanged(inst):
    """The shared instance was not touched by the tampers."""
    return twin(inst) == (True, inst.clean())


@pytest.mark.parametrize("name", W.FORGED)
def test_a_consistent_forgery_fails_on_the_sibling_check_alone(name):
    from starkperp import state
    inst, _ = built(name)
    forged, want = W.forge(W.CASES[name], inst,
                           lambda h, e: state.SparseMerkleTree(h, e, hash_many=oracle_hash_many))
    assert forged.new_root != inst.new_root
    verdict, status = twin(forged)
    assert status == want and verdict is False
    assert sum(1 for b in status[0] if b) == 1 and sum(1 for b in status[1] if b) == 1
    # every record of the forgery hashes, and both inclusion statements alone would pass: only the walk that compares
    # the untouched sides refuses it
    records = forged.before + forged.after
    assert oracle_hash_many([r[3] for r in records], [r[4] for r in records]) == [r[2] for r in records]
    assert consumer_accepts(forged) is False
    facts = state.facts_of(records)
    mods = {k: (a, b) for k, a, b in zip(forged.keys, forged.prev_leaves, forged.new_leaves)}
    assert state.verify_multi_update(facts, forged.height, forged.prev_root, forged.new_root, mods,
                                     hash_many=oracle_hash_many) is False


def test_no_keys_and_bad_arguments():
    from starkperp import state
    assert state.verify_update_records(64, [], [], [], 5, 5, [], [], oracle_hash_many) == (True, [[], []])
    assert state.verify_update_records(64, [], [], [], 5, 6, [], [], oracle_hash_many) == (False, [[], []])
    assert state.verify_multi_update({}, 64, 5, 5, {}, hash_many=oracle_hash_many) is True
    inst, _ = built("B")
    args = lambda **kw: {**dict(height=inst.height, keys=inst.keys, prev_leaves=inst.prev_leaves,
                                new_leaves=inst.new_leaves, prev_root=inst.prev_root, new_root=inst.new_root,
                                before=inst.before, after=inst.after, hash_many=oracle_hash_many), **kw}
    for bad in (dict(keys=inst.keys[::-1]), dict(keys=inst.keys[:-1] + [8]), dict(height=0), dict(height=65),
                dict(before=inst.before[:-1])):
        with pytest.raises(AssertionError):
            state.verify_update_records(**args(**bad))


def test_shared_state_checks_the_facts_it_collects():
    """apply_state_updates(..., facts=d, check_facts=True) on the host route: same roots and the same facts as
    without the check, and a dict that verifies both trees' statements."""
    import random
    from oracle import ref_py as R
    from witness_replay import oracle_hash
    from starkperp import state
    rng = random.Random(5)
    hashes = lambda positions: [R.position_hash(p[0], p[1], list(p[2]), hash_function=oracle_hash) for p in positions]
    make = lambda: state.SharedState(64, 64, hash_many=oracle_hash_many, position_hashes=hashes)
    checked, plain = make(), make()
    empty = state.SharedState.EMPTY_POSITION
    pos = [(k, empty, (rng.randrange(2**251), rng.randrange(2**62), ())) for k in (0, 9, 2**64 - 1)]
    orders = [(k, 0, rng.randrange(W.P)) for k in sorted(rng.randrange(2**64) for _ in range(4))]
    d_checked, d_plain = {}, {}
    roots = checked.apply_state_updates(pos, orders, facts=d_checked, check_facts=True)
    assert roots == plain.apply_state_updates(pos, orders, facts=d_plain)
    assert d_checked == d_plain and d_checked
    assert state.verify_multi_update(d_checked, 64, roots[1][0], roots[1][1], {k: (a, b) for k, a, b in orders},
                                     hash_many=oracle_hash_many) is True
    with pytest.raises(AssertionError):
        plain.apply_state_updates(pos, orders, check_facts=True)
