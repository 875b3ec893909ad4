"""Host side of the ragged hash chains, no GPU: the two C-ABI symbols are declared and bound, the mixed-batch
message packer produces the words of the per-type packers, and the list API packs its chains as CSR."""
import os
import re

import pytest

from oracle import ref_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.FIELD_PRIME
NAMES = ("sp_pedersen_chains_ragged", "sp_pedersen_chains_ragged_dev")


def spy(a, b):
    return (a * 3 + b * 5 + 1) % P


def test_header_and_binding_declare_the_calls():
    from starkperp import _lib
    text = open(os.path.join(ROOT, "include", "starkperp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.declared_symbols()
        # the threading / multi-device paragraphs list them next to the equal-depth calls
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name
    res, args = _lib._SIGNATURES["sp_pedersen_chains_ragged"]
    assert len(args) == 5
    res, args = _lib._SIGNATURES["sp_pedersen_chains_ragged_dev"]
    assert len(args) == 6


def mixed_items():
    price = (0x4D616B6572, 0x42544355534400000000000000000000, 0x5F590C1E, 0xAC9F3163AD52B000)
    return [
        ("limit_order", (7, 8, 1, 9, 10, 11, 12, 13, 14, 15)),
        ("price", price),
        ("transfer", (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)),
        ("limit_order", (7, 8, 0, 9, 10, 11, 12, 13, 14, 15)),
        ("conditional_transfer", (5, 6, 7, 99, 8, 9, 10, 11, 12, 13, 14)),
        ("withdrawal_to_address", (5, 6, "0xabc", 7, 8, 9)),
        ("withdrawal", (5, 6, 7, 8, 9)),
        ("withdrawal_to_address", (5, 6, 0xABC, 7, 8, 9)),
    ]


def test_mixed_packer_matches_the_per_type_packers():
    from starkperp import perpetual_messages as pm
    items = mixed_items()
    scalar = {"limit_order": pm.get_limit_order_msg, "price": pm.get_price_msg, "transfer": pm.get_transfer_msg,
              "conditional_transfer": pm.get_conditional_transfer_msg,
              "withdrawal_to_address": pm.get_withdrawal_to_address_msg, "withdrawal": pm.get_withdrawal_msg}
    oracle = {"limit_order": R.get_limit_order_msg, "price": R.get_price_msg, "transfer": R.get_transfer_msg,
              "conditional_transfer": R.get_conditional_transfer_msg,
              "withdrawal_to_address": R.get_withdrawal_to_address_msg, "withdrawal": R.get_withdrawal_msg}
    got = pm.message_hashes_mixed(items, hash_function=spy)
    for (kind, args), v in zip(items[:-1], got):  # the last item gives the address as an int: *_many only
        assert v == scalar[kind](*args, hash_function=spy), kind
        assert v == oracle[kind](*args, hash_function=spy), kind
    assert got[-1] == got[-3]
    assert sorted(pm.MIXED_KINDS) == ["conditional_transfer", "limit_order", "price", "transfer", "withdrawal",
                                      "withdrawal_to_address"]
    with pytest.raises(ValueError):
        pm.message_hashes_mixed([("deposit", ())], hash_function=spy)
    # chain lengths: 2 words for prices and old-API withdrawals, 3 / 5 / 6 for the others
    lengths = {k: len(pm.MIXED_KINDS[k](a)) for k, a in items}
    assert lengths == {"limit_order": 5, "price": 2, "transfer": 5, "conditional_transfer": 6,
                       "withdrawal_to_address": 3, "withdrawal": 2}


class StubLib:
    """A pure-Python sp_pedersen_chains_ragged: folds every chain with `spy` and records what it was handed."""

    def __init__(self):
        self.calls = []

    def sp_pedersen_chains_ragged(self, elems, off, n, out, st):
        raw = bytes(elems)
        words = [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]
        offsets = list(off)
        self.calls.append((words, offsets, n))
        assert len(offsets) == n + 1 and offsets[0] == 0 and offsets[-1] == len(words)
        for i in range(n):
            chain = words[offsets[i]: offsets[i + 1]]
            acc = chain[0]
            for w in chain[1:]:
                acc = spy(acc, w)
            for k in range(4):
                out[4 * i + k] = (acc >> (64 * k)) & (2**64 - 1)
            st[i] = self.status.get(i, 0)
        return 0

    status = {}


@pytest.fixture()
def stub(monkeypatch):
    from starkperp import _lib
    s = StubLib()
    monkeypatch.setattr(_lib, "ensure_init", lambda *a, **k: s)
    return s


def test_list_api_packs_csr(stub):
    from starkperp import batch, perpetual_messages as pm, state
    chains = [[1, 2, 3], [P - 1], [4, 5], [6, 7, 8, 9, 10, 11, 12, 13, 14]]
    got = batch.pedersen_chains_ragged(chains)
    words, offsets, n = stub.calls[0]
    assert n == 4 and offsets == [0, 3, 4, 6, 15] and words == [w for c in chains for w in c]
    assert got == [spy(spy(1, 2), 3), P - 1, spy(4, 5)] + [got[3]] and got[3] < P
    assert batch.pedersen_chains_ragged([]) == [] and len(stub.calls) == 1
    # the routed callers hand over their chains in input order, in one call
    del stub.calls[:]
    items = mixed_items()
    assert pm.message_hashes_mixed(items) == pm.message_hashes_mixed(items, hash_function=spy)
    assert len(stub.calls) == 1 and stub.calls[0][1] == [0, 5, 7, 12, 17, 23, 26, 28, 31]
    del stub.calls[:]
    poss = [(11, -5, [(3, -7, 9), (4, 8, -1)]), (12, 6, []), (13, 0, [(9, 1, 2)])]
    want = []
    for p in poss:
        w = state.position_words(p)
        acc = w[0]
        for v in w[1:]:
            acc = spy(acc, v)
        want.append(acc)
    assert state.position_hashes_many(poss) == want
    assert len(stub.calls) == 1 and stub.calls[0][1] == [0, 5, 8, 12]
    # status bytes map to the exceptions of pedersen_chains_many
    stub.status = {2: 2}
    with pytest.raises(AssertionError, match="Unhashable input."):
        batch.pedersen_chains_ragged(chains)
    stub.status = {0: 1}
    with pytest.raises(AssertionError):
        batch.pedersen_chains_ragged(chains)
