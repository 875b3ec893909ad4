"""Every host-pointer batch makes its round trip through csrc/context.hpp StagedTrip: the inputs and outputs of a call
cross in one page-locked block up to 4 MiB (inputs + outputs) and in one direct copy per array above.  For each call
below: a batch just above the line in one call (direct) against its two halves in two calls (both staged) - equal item
by item - and 64 items at each end and in the middle against the oracle.  The chain calls and the persistent trees
have theirs in test_gpu_pedersen.py, test_gpu_chains_ragged.py and the tree tests."""
import numpy as np
import pytest

import sign_cases
from oracle import cref
from oracle import ref_py as R

pytestmark = pytest.mark.gpu

LIMIT = 4 << 20


@pytest.fixture(scope="module")
def bnp():
    from starkperp import batch_np
    return batch_np


def sizes(per_item, n):
    """n is the first direct size of a trip of per_item bytes an item; its halves are staged."""
    assert per_item * n > LIMIT >= per_item * (n - 1)
    half = n // 2
    assert per_item * (n - half) <= LIMIT
    return half


def sample(n):
    return list(range(64)) + list(range(n // 2 - 32, n // 2 + 32)) + list(range(n - 64, n))


def felts(rng, n, top_shift=6):
    a = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # odd: never zero
    a[:, 3] >>= np.uint64(top_shift)  # below 2^(256 - top_shift)
    return a


def four_keys(rng, bnp, n):
    ds = [int(v) for v in bnp.ints_from_felts(felts(rng, 4))]
    d = bnp.felts_from_ints([ds[i % 4] for i in range(n)])
    return ds, d


def halves_equal(call, arrays, n, half):
    """call(*arrays) -> tuple of arrays with n rows: the whole batch against its two halves, row by row."""
    whole = call(*arrays)
    lo = call(*[a[:half] for a in arrays])
    hi = call(*[a[half:] for a in arrays])
    for w, a, b in zip(whole, lo, hi):
        assert (w[:half] == a).all() and (w[half:] == b).all()
    return whole


def test_pedersen_batch(bnp):
    n = 43241
    half = sizes(97, n)  # x, y up; hash and status byte down
    rng = np.random.default_rng(11)
    x, y = felts(rng, n), felts(rng, n)
    (out,) = halves_equal(lambda a, b: (bnp.pedersen_hash_many(a, b),), [x, y], n, half)
    i = sample(n)
    assert bnp.ints_from_felts(out[i]) == cref.pedersen_hash_many(bnp.ints_from_felts(x[i]), bnp.ints_from_felts(y[i]))[0]


def test_public_key_batch(bnp):
    from starkperp import _lib
    n = 43241
    half = sizes(97, n)  # d up; qx, qy and status byte down
    d = felts(np.random.default_rng(12), n)

    def call(d):
        m = d.shape[0]
        d = np.ascontiguousarray(d)
        qx, qy, st = np.zeros((m, 4), np.uint64), np.zeros((m, 4), np.uint64), np.ones(m, np.uint8)
        _lib.check(_lib.ensure_init().sp_public_key_batch(bnp._ptr(d), bnp._ptr(qx), bnp._ptr(qy), bnp._ptr(st), m), "public keys")
        assert not st.any()
        return qx, qy

    qx, qy = halves_equal(call, [d], n, half)
    i = sample(n)
    assert list(zip(bnp.ints_from_felts(qx[i]), bnp.ints_from_felts(qy[i]))) == cref.public_keys_many(bnp.ints_from_felts(d[i]))


def test_sign_batch(bnp):
    from starkperp import _lib
    n = 26052
    half = sizes(161, n)  # z, d, k up; r, s and status byte down
    rng = np.random.default_rng(13)
    _, d = four_keys(rng, bnp, n)
    z, k = felts(rng, n), felts(rng, n)

    def call(z, d, k):
        m = z.shape[0]
        z, d, k = (np.ascontiguousarray(a) for a in (z, d, k))
        r, s, st = np.zeros((m, 4), np.uint64), np.zeros((m, 4), np.uint64), np.full(m, 9, np.uint8)
        _lib.check(_lib.ensure_init().sp_ecdsa_sign_batch(*[bnp._ptr(a) for a in (z, d, k, r, s, st)], m), "sign")
        return r, s, st

    r, s, st = halves_equal(call, [z, d, k], n, half)
    i = sample(n)
    zi, di, ki = (bnp.ints_from_felts(a[i]) for a in (z, d, k))
    sign_cases.prime_r(ki)
    want = [sign_cases.attempt(*item) for item in zip(zi, di, ki)]
    assert list(zip(st[i].tolist(), bnp.ints_from_felts(r[i]), bnp.ints_from_felts(s[i]))) == want


def test_sign_rfc6979_batch(bnp):
    n = 30616
    half = sizes(137, n)  # z, d, 8-byte seeds up; r, s and status byte down
    assert half > sign_cases.COMPACT_MIN and half % 4 == 0  # the compacted signer on both sides, no padding behind the seeds
    rng = np.random.default_rng(14)
    _, d = four_keys(rng, bnp, n)
    z = felts(rng, n)
    seeds = rng.integers(1, 2**63, size=n, dtype=np.uint64)
    r, s = halves_equal(bnp.sign_many, [z, d, seeds], n, half)
    i = sample(n)
    want = [R.sign(*item) for item in zip(bnp.ints_from_felts(z[i]), bnp.ints_from_felts(d[i]), seeds[i].tolist())]
    assert list(zip(bnp.ints_from_felts(r[i]), bnp.ints_from_felts(s[i]))) == want


def test_verify_batch_on_the_ladder_with_x_only_keys(bnp):
    from starkperp import batch
    n = 32514
    half = sizes(129, n)  # z, r, s, qx up; verdict byte down
    rng = np.random.default_rng(15)
    ds, d = four_keys(rng, bnp, n)
    pub = cref.public_keys_many(ds)
    qx = bnp.felts_from_ints([pub[i % 4][0] for i in range(n)])
    z = felts(rng, n)
    r, s = bnp.sign_many(z, d)
    z[::7, 0] ^= np.uint64(2)  # every seventh signature no longer verifies
    before = batch.get_verify_policy()
    batch.set_verify_policy(batch.VERIFY_POLICY_LADDER)
    try:
        (codes,) = halves_equal(lambda *a: (bnp.verify_codes(*a),), [z, r, s, qx], n, half)
    finally:
        batch.set_verify_policy(before)
    assert (codes == np.where(np.arange(n) % 7 == 0, batch.VERIFY_FALSE, batch.VERIFY_TRUE)).all()
    i = sample(n)
    want = cref.verify_codes(*[bnp.ints_from_felts(a[i]) for a in (z, r, s)], [pub[j % 4] for j in i])
    assert codes[i].tolist() == want


def test_merkle_fold_and_verify_paths(bnp):
    height, n = 20, 5950
    # leaf and 20 siblings up, root and status byte down; the verifier takes a root per path as well and brings back two bytes
    half = sizes((1 + height) * 32 + 33, n)
    assert ((2 + height) * 32 + 2) * n > LIMIT >= ((2 + height) * 32 + 2) * (n - half)
    rng = np.random.default_rng(16)
    leaves, sib = felts(rng, n), felts(rng, n * height).reshape(n, height, 4)
    keys = rng.integers(0, 1 << height, size=n, dtype=np.uint64)
    roots, st = halves_equal(lambda a, b, c: bnp.merkle_fold_paths(a, b, c, height=height), [leaves, sib, keys], n, half)
    assert not st.any()
    i = sample(n)
    node = bnp.ints_from_felts(leaves[i])
    for level in range(height):
        other = bnp.ints_from_felts(sib[i, level])
        right = [(int(k) >> level) & 1 for k in keys[i]]
        node = cref.pedersen_hash_many([o if b else v for v, o, b in zip(node, other, right)],
                                       [v if b else o for v, o, b in zip(node, other, right)])[0]
    assert bnp.ints_from_felts(roots[i]) == node
    expected = roots.copy()
    expected[::5, 1] ^= np.uint64(1)  # every fifth path is checked against another root
    verdict, st = halves_equal(lambda a, b, c, e: bnp.merkle_verify_paths(a, b, c, e, height=height),
                               [leaves, sib, keys, expected], n, half)
    assert not st.any() and (verdict == (np.arange(n) % 5 != 0)).all()
