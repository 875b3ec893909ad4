"""Host side of the one-call state update (starkperp.state.pack_state_batch and the status -> assertion mapping of
SharedState's one-call route).  No GPU: the packer is pure host code, and the route is driven with a stand-in for
batch_np.state_batch."""
import numpy as np
import pytest

from oracle import cref
from oracle import ref_py as R
from starkperp import state

P = R.FIELD_PRIME
EMPTY = (0, 0, ())


def position(n_assets, salt):
    """A position with `n_assets` assets, values inside the bounds of definitions/constants.cairo:11-38."""
    assets = tuple((1000 * salt + 7 * a + 1, (-1) ** a * (salt * 977 + a), 2**62 - salt - a) for a in range(n_assets))
    return (2**250 - 12345 * salt - n_assets, -(2**63) + salt if salt % 2 else 2**63 - 1 - salt, assets)


def fold(words):
    """Left fold of one chain with the C oracle's hash."""
    acc = words[0]
    for w in words[1:]:
        acc = cref.opt_pedersen_hash_many([acc], [w])[0][0]
    return acc


def rows(arr, lo, hi):
    return [int.from_bytes(arr[i].astype("<u8").tobytes(), "little") for i in range(lo, hi)]


def test_pack_state_batch_words_offsets_and_dtypes():
    """Asset counts 0..6 mixed (chains of 3 to 9 words), changed and unchanged positions interleaved: the packed rows
    are position_words chain after chain, folding them with the oracle hash gives the oracle's leaf (R.position_hash,
    pure Python), and an unchanged position has a new chain of length zero."""
    prevs = [position(n, 1 + n) for n in (3, 0, 6, 1, 5, 2, 4)]
    news = [position((n + 3) % 7, 20 + n) if i % 2 == 0 else prevs[i] for i, n in enumerate((3, 0, 6, 1, 5, 2, 4))]
    pos = [(10 + 3 * i, p, q) for i, (p, q) in enumerate(zip(prevs, news))]
    orders = [(5, 0, 17), (2**64 - 1, P - 1, 2**200 + 3)]
    pos_keys, prev_words, prev_off, new_words, new_off, ord_keys, ord_prev, ord_new = state.pack_state_batch(pos, orders)
    assert pos_keys.dtype == np.uint64 and pos_keys.tolist() == [10 + 3 * i for i in range(7)]
    assert ord_keys.dtype == np.uint64 and ord_keys.tolist() == [5, 2**64 - 1]
    for off in (prev_off, new_off):
        assert off.dtype == np.uint32 and off.shape == (8,) and off[0] == 0
    for arr in (prev_words, new_words, ord_prev, ord_new):
        assert arr.dtype == np.uint64 and arr.ndim == 2 and arr.shape[1] == 4 and arr.flags["C_CONTIGUOUS"]
    assert prev_off.tolist() == [0] + list(np.cumsum([len(p[2]) + 3 for p in prevs]))
    assert prev_words.shape[0] == prev_off[-1] and new_words.shape[0] == new_off[-1]
    assert rows(ord_prev, 0, 2) == [0, P - 1] and rows(ord_new, 0, 2) == [17, 2**200 + 3]
    for i, (_, p, q) in enumerate(pos):
        got = rows(prev_words, prev_off[i], prev_off[i + 1])
        assert got == state.position_words(p)
        assert fold(got) == R.position_hash(p[0], p[1], list(p[2]))
        if p == q:
            assert new_off[i + 1] == new_off[i]
        else:
            got = rows(new_words, new_off[i], new_off[i + 1])
            assert len(got) == len(q[2]) + 3 and got == state.position_words(q)
            if i in (0, 2):
                assert fold(got) == R.position_hash(q[0], q[1], list(q[2]))


def test_pack_state_batch_empty_and_all_unchanged():
    out = state.pack_state_batch([], [])
    assert [a.shape for a in out] == [(0,), (0, 4), (1,), (0, 4), (1,), (0,), (0, 4), (0, 4)]
    assert [a.dtype for a in out] == [np.uint64, np.uint64, np.uint32, np.uint64, np.uint32] + [np.uint64] * 3
    assert out[2].tolist() == [0] and out[4].tolist() == [0]
    p = position(2, 3)
    _, prev_words, prev_off, new_words, new_off, _, _, _ = state.pack_state_batch([(1, EMPTY, EMPTY), (4, p, p)], [])
    assert prev_off.tolist() == [0, 3, 8] and new_off.tolist() == [0, 0, 0] and new_words.shape == (0, 4)
    assert rows(prev_words, 0, 3) == state.position_words(EMPTY)


class FakeTree(state.LibrarySparseTree):
    """A LibrarySparseTree that never touches the library: the one-call route only reads its height and handle."""

    def __init__(self, height):
        self.height, self._handle = height, None


def shared_state_without_a_gpu():
    st = state.SharedState.__new__(state.SharedState)
    st._position_hashes = state.position_hashes_many
    st.positions, st.orders = FakeTree(8), FakeTree(6)
    return st


def test_one_call_route_maps_status_bytes_to_the_assertions(monkeypatch):
    """SharedState._apply_in_one_call with a stand-in for batch_np.state_batch: committed batches hand the roots on,
    every status combination raises the text of the separate-call route, and the Python-side range asserts come
    before the call."""
    from starkperp import batch_np
    calls = []
    answer = {}

    def fake_state_batch(ptree, otree, pos_keys, prev_words, prev_off, new_words, new_off, ord_keys, ord_prev, ord_new):
        calls.append((pos_keys.tolist(), prev_off.tolist(), new_off.tolist(), ord_keys.tolist()))
        return ((1, 2), (3, 4), np.array(answer.get("pos", [0] * len(pos_keys)), dtype=np.uint8),
                np.array(answer.get("ord", [0] * len(ord_keys)), dtype=np.uint8), answer.get("batch", 0))

    monkeypatch.setattr(batch_np, "state_batch", fake_state_batch)
    st = shared_state_without_a_gpu()
    p1, p2 = position(1, 1), position(2, 2)
    accesses = [(200, EMPTY, p1), (3, EMPTY, p1), (3, p1, p2), (7, p2, p2)]
    orders = [(9, 0, 10), (9, 10, 25), (1, 0, 4)]
    assert st.apply_state_updates(accesses, orders) == ((1, 2), (3, 4))
    assert calls == [([3, 7, 200], [0, 3, 8, 11], [0, 5, 5, 9], [1, 9])]  # squashed, sorted; key 7 unchanged
    for status, text in (
            (dict(pos=[0, 0x10, 0], batch=0x90), "previous position does not match the tree"),
            (dict(ord=[0x10, 0], batch=0x90), "previous order state does not match the tree"),
            (dict(ord=[0, 1], batch=0x81), "order leaf out of range"),
            (dict(ord=[0, 0x11], pos=[0x10, 0, 0], batch=0x91), "previous position does not match the tree"),
            (dict(batch=0x82), "Unhashable input."),
            (dict(pos=[0, 0, 2], batch=0x82), "Unhashable input."),
            (dict(batch=0x81), "leaf out of range")):
        answer.clear()
        answer.update(status)
        with pytest.raises(AssertionError) as err:
            st.apply_state_updates(accesses, orders)
        assert str(err.value) == text, (status, str(err.value))
    answer.clear()
    answer.update(pos=[1, 0, 0], batch=0x81)  # a position word out of range: the bare assertion of signature.py:307
    with pytest.raises(AssertionError) as err:
        st.apply_state_updates(accesses, orders)
    assert str(err.value) == ""
    # range asserts before the call: nothing reaches the library
    del calls[:]
    for bad_orders, text in (([(9, 0, P)], "order leaf out of range"), ([(1 << 6, 0, 1)], "order leaf out of range"),
                             ([(9, -1, 1)], "previous order state does not match the tree")):
        with pytest.raises(AssertionError) as err:
            st.apply_state_updates(accesses, bad_orders)
        assert str(err.value) == text
    with pytest.raises(AssertionError):
        st.apply_state_updates([(1 << 8, EMPTY, p1)], [])
    assert calls == []
    # an injected position hash keeps the separate-call route
    st._position_hashes = lambda ps: [0] * len(ps)
    monkeypatch.setattr(state.SharedState, "_apply_in_separate_calls", lambda self, a, b: "separate")
    assert st.apply_state_updates(accesses, orders) == "separate" and calls == []
