"""GPU parity of the ragged hash chains (sp_pedersen_chains_ragged[_dev], the chain form of ped_fold_ragged_kernel):
chains of unequal length in one launch against the C oracle, the reference-pinned rows that now take this path,
per-chain status, bad arguments, the _dev variant, the per-step fallback, and the same data through the path form of
the kernel (sp_merkle_fold_paths)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chains_ragged_cases as cases
import workloads as wl
from oracle import ref_py as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
P = R.FIELD_PRIME


def load(name):
    return json.load(open(os.path.join(GOLD, name)))


def h(s):
    return int(s, 16)


@pytest.fixture(scope="module")
def batch():
    from starkperp import batch as b
    return b


@pytest.fixture(scope="module")
def batch_np():
    from starkperp import batch_np as b
    return b


# n: group, block and `dup` boundaries of the eight-quad class (1 .. 300), the first sizes of the four- and two-quad
# classes (2049, 4097), one slice boundary (8200 = 8192 + 8); lengths uniform in 1 .. 9, from 2049 on in 1 .. 4
# (about 24 000 oracle hashes in all)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 65, 300, 2049, 4097, 8200])
def test_random_lengths_vs_c_oracle(batch, n):
    chains = cases.random_chains(cases.random_lengths(n, 9 if n < 2049 else 4, seed=n), seed=1000 + n)
    assert batch.pedersen_chains_ragged(chains) == cases.oracle_fold(chains)


# 64 chains run one per wave (eight quads, every hash on two lane groups), four to a block: 16 blocks, each with
# its own loop bound
LENGTH_PATTERNS = {
    "all_one": [1] * 64,
    "long_in_first_block": [2] * 3 + [9] + [2] * 60,
    "long_in_middle_block": [2] * 35 + [9] + [2] * 28,
    "long_in_last_block": [2] * 63 + [9],
    "descending": [9 - i // 8 for i in range(64)],
    "ascending": [1 + i // 8 for i in range(64)],
}


@pytest.mark.parametrize("name", sorted(LENGTH_PATTERNS))
def test_length_patterns_vs_c_oracle(batch, name):
    chains = cases.random_chains(LENGTH_PATTERNS[name], seed=len(name))
    assert batch.pedersen_chains_ragged(chains) == cases.oracle_fold(chains)


def test_chains_and_paths_fold_the_same_data(batch_np):
    """A chain is a path with key 0 whose leaf is the chain's first word and whose siblings are the rest: the two
    forms of the one kernel give the same values and status bytes, and both are the oracle's."""
    chains = cases.random_chains([1, 2, 3, 7, 1, 2, 3, 7, 1], seed=77)
    words, off = cases.csr(chains)
    got_c, st_c = batch_np.pedersen_chains_ragged(words, off)
    leaves = batch_np.felts_from_ints([c[0] for c in chains])
    sib = batch_np.felts_from_ints([w for c in chains for w in c[1:]])
    sib_off = np.array([0] + list(np.cumsum([len(c) - 1 for c in chains])), dtype=np.uint32)
    got_p, st_p = batch_np.merkle_fold_paths(leaves, sib, np.zeros(len(chains), dtype=np.uint64), offsets=sib_off)
    assert (got_c == got_p).all() and (st_c == st_p).all() and not st_c.any()
    assert batch_np.ints_from_felts(got_c) == cases.oracle_fold(chains)


def test_a_batch_above_the_staging_limit_equals_the_equal_length_call(batch_np):
    """sp_pedersen_chains_ragged sends off[n] x 32 + 33 n bytes through page-locked memory up to 4 MiB and copies
    directly above (csrc/context.hpp StagedTrip); the largest batch above is 8200 chains, under 1 MiB.  33 000 chains of
    4 words are 5 313 000 bytes: hashes and status bytes come back in two direct copies.  The same chains through
    sp_pedersen_chains (word-major, pinned at this size by tests/test_gpu_pedersen.py) give the same rows."""
    n, depth = 33000, 4
    assert n * depth * 32 + 33 * n > 4 << 20
    rng = np.random.default_rng(33)
    words = rng.integers(0, 2**63, size=(depth, n, 4), dtype=np.uint64)
    words[:, :, 3] >>= np.uint64(8)  # below p
    chain_major = np.ascontiguousarray(words.transpose(1, 0, 2)).reshape(n * depth, 4)
    got, status = batch_np.pedersen_chains_ragged(chain_major, np.arange(n + 1, dtype=np.uint32) * np.uint32(depth))
    assert not status.any()
    assert (got == batch_np.pedersen_chains(words)).all()
    # the status bytes travel too: word 2 of chain 12345 becomes p, and that chain alone is flagged
    chain_major[12345 * depth + 2] = batch_np.felts_from_ints([R.FIELD_PRIME])[0]
    again, status = batch_np.pedersen_chains_ragged(chain_major, np.arange(n + 1, dtype=np.uint32) * np.uint32(depth))
    assert np.flatnonzero(status).tolist() == [12345] and status[12345] & 1  # SP_HASH_OUT_OF_RANGE
    keep = np.arange(n) != 12345
    assert (again[keep] == got[keep]).all()


class CountingLib:
    """The binding with the calls of the chain entry points counted."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("sp_pedersen"):
            def counted(*a):
                self.calls.append(name)
                return fn(*a)
            return counted
        return fn


@pytest.fixture()
def counting(monkeypatch):
    from starkperp import _lib
    spy = CountingLib(_lib.ensure_init())
    monkeypatch.setattr(_lib, "ensure_init", lambda *a, **k: spy)
    return spy


def test_mixed_messages_in_one_call(counting):
    from starkperp import perpetual_messages as pm
    g = load("g5_messages.json")
    orders = [wl.order_args(o) for o in wl.limit_orders(256, seed=g["seed"])]
    price = (0x4D616B6572, 0x42544355534400000000000000000000, 0x5F590C1E, 0xAC9F3163AD52B000)
    items, want = [], []
    for i, o in enumerate(orders):
        items.append(("limit_order", o))
        want.append(h(g["limit_order_z"][i]))
        if i % 16 == 1:
            a = (5 + i, 6, 7, 8, 9, 10, 11, 12, 13, 14)
            items.append(("transfer", a))
            want.append(R.get_transfer_msg(*a))
        if i % 16 == 5:
            a = (5, 6, 7, 99 + i, 8, 9, 10, 11, 12, 13, 14)
            items.append(("conditional_transfer", a))
            want.append(R.get_conditional_transfer_msg(*a))
        if i % 16 == 9:
            a = (5 + i, 6, "0x%040x" % (0xABC + i), 7, 8, 9)
            items.append(("withdrawal_to_address", a))
            want.append(R.get_withdrawal_to_address_msg(*a))
        if i % 16 == 13:
            a = (5 + i, 6 + i, 7, 8, 9 + i)
            items.append(("withdrawal", a))
            want.append(R.get_withdrawal_msg(*a))
        if i == 100:
            items.append(("price", price))
            want.append(h(g["price"]))
        if i % 64 == 3:
            a = (price[0], price[1] + i, price[2], price[3])
            items.append(("price", a))
            want.append(R.get_price_msg(*a))
    assert pm.message_hashes_mixed(items) == want
    assert counting.calls == ["sp_pedersen_chains_ragged"]
    with pytest.raises(ValueError):
        pm.message_hashes_mixed([("deposit", ())])


def test_position_hashes_take_the_ragged_call(counting):
    from starkperp import state
    g = load("g6_merkle.json")
    poss = wl.positions(64, seed=3)
    assert len({len(p[2]) for p in poss}) > 1  # chains of 3 .. 6 words
    assert state.position_hashes_many(poss) == [h(v) for v in g["position_hashes_seed3"]]
    assert counting.calls == ["sp_pedersen_chains_ragged"]
    # equal lengths keep the equal-depth call
    del counting.calls[:]
    same = [p for p in poss if len(p[2]) == 2]
    assert state.position_hashes_many(same) == [R.position_hash(*p) for p in same]
    assert counting.calls == ["sp_pedersen_chains"]
    # previous and new leaves of all updates: one call
    del counting.calls[:]
    ups = [(i, poss[i], poss[i + 1] if i % 2 else poss[i]) for i in range(8)]
    want = [(k, R.position_hash(*a), R.position_hash(*b)) for k, a, b in ups]
    assert state.hash_position_updates(ups) == want
    assert counting.calls == ["sp_pedersen_chains_ragged"]


def test_mixed_withdrawals_in_one_call(counting):
    from starkperp import perpetual_messages as pm
    mixed = [(5 + i, 6, 100 + (i % 2), 100, 7, 8, 9 + i) for i in range(6)]  # owner == signer on even i
    assert pm.withdrawal_hashes_many(mixed) == [R.withdrawal_hash(*a) for a in mixed]
    assert counting.calls == ["sp_pedersen_chains_ragged"]


def test_per_chain_status(batch, batch_np):
    cases.check_status_case(batch_np)
    chains, _ = cases.status_case()
    with pytest.raises(AssertionError):  # the list API asserts the range like pedersen_chains_many
        batch.pedersen_chains_ragged(chains)
    with pytest.raises(AssertionError):
        batch.pedersen_chains_ragged([[1, 2], [P]])
    with pytest.raises(AssertionError):
        batch.pedersen_chains_ragged([[1, 2], []])


def test_bad_arguments_leave_out_untouched(batch_np):
    from starkperp import _lib
    lib = _lib.ensure_init()
    words = batch_np.felts_from_ints([1, 2, 3, 4, 5])
    out = np.full((3, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    st = np.full(3, 0xEE, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for off in ([0, 2, 2, 5], [1, 2, 3, 5], [0, 3, 2, 5]):  # a zero-length chain, off[0] != 0, a falling offset
        o = np.array(off, dtype=np.uint32)
        assert lib.sp_pedersen_chains_ragged(ptr(words), ptr(o), 3, ptr(out), ptr(st)) == -3  # SP_ERR_BAD_ARGUMENT
        assert b"ragged" in lib.sp_last_error()
        assert (out == 0xA5A5A5A5A5A5A5A5).all() and (st == 0xEE).all()
    o = np.zeros(1, dtype=np.uint32)
    assert lib.sp_pedersen_chains_ragged(ptr(words), ptr(o), 0, ptr(out), ptr(st)) == 0
    assert lib.sp_pedersen_chains_ragged(None, None, 0, None, None) == 0
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    got, st0 = batch_np.pedersen_chains_ragged(np.zeros((0, 4), dtype=np.uint64), [0])
    assert got.shape == (0, 4) and st0.shape == (0,)


def test_dev_variant_on_a_side_stream(batch_np):
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    chains, _ = cases.status_case()
    chains += cases.random_chains(cases.random_lengths(200, 7, seed=5), seed=6)
    words, off = cases.csr(chains)
    n = len(chains)
    want, want_st = batch_np.pedersen_chains_ragged(words, off)
    side = torch.cuda.Stream()
    d_words = torch.from_numpy(words.view(np.int64)).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host_off = off.copy()
    with torch.cuda.stream(side):
        _lib.check(lib.sp_pedersen_chains_ragged_dev(d_words.data_ptr(), host_off.ctypes.data_as(ctypes.c_void_p), n,
                                                     d_out.data_ptr(), d_st.data_ptr(), side.cuda_stream),
                   "sp_pedersen_chains_ragged_dev")
        host_off[:] = 0  # the offsets were copied before the call returned
        # status = NULL is allowed
        d_out2 = torch.zeros_like(d_out)
        _lib.check(lib.sp_pedersen_chains_ragged_dev(d_words.data_ptr(), off.ctypes.data_as(ctypes.c_void_p), n,
                                                     d_out2.data_ptr(), None, side.cuda_stream),
                   "sp_pedersen_chains_ragged_dev")
    side.synchronize()
    assert (d_out.cpu().numpy().view(np.uint64) == want).all()
    assert (d_out2.cpu().numpy().view(np.uint64) == want).all()
    assert (d_st.cpu().numpy() == want_st).all() and want_st[5] == 1


@pytest.mark.parametrize("switch", ["STARKPERP_NO_QUAD", "STARKPERP_NO_CHAIN_RAGGED"])
def test_fallback_in_a_child_process(switch):
    """No fused kernel (the quad kernels switched off / the A/B switch of the ragged launch): one launch per step
    over the chains still running; 300 chains and the status case against the oracle, in a fresh interpreter."""
    env = dict(os.environ)
    env[switch] = "1"
    done = subprocess.run([sys.executable, os.path.join(HERE, "chains_ragged_cases.py")], env=env, timeout=120,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "chains_ragged child ok" in done.stdout, done.stdout[-2000:]
