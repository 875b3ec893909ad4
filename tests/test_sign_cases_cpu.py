"""tests/sign_cases.py against the oracle, no GPU: the attempt body against R.verify / R.sign, the candidate counter
against R.generate_k_rfc6979, the pinned pool against a recount, round_of and the thresholds against the constants of
csrc/ecdsa.hip they restate.  tests/test_gpu_sign_edges.py runs the library on exactly these cases."""
import os
import random
import re
from collections import Counter

import pytest

import sign_cases as C
from oracle import ref_py as R

N, TWO251 = C.N, C.TWO251
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return C.attempt_cases()


@pytest.fixture(scope="module")
def pool():
    return C.nonce_pool()


def test_every_kind_of_case_is_there(cases):
    kinds = Counter(C.attempt_kind(z, d, k)[3] for z, d, k, _ in cases)
    # the reachable rejections, at least 20 each; the r branch needs a discrete logarithm and stays empty
    assert kinds["retry_t"] >= 20 and kinds["retry_w"] >= 20 and kinds["bad_input"] >= 20 and kinds["ok"] >= 200
    assert kinds["retry_r"] == 0
    by_label = Counter(re.sub(r"0x[0-9a-f]+|\d+", "#", label.split(",")[0]) for _, _, _, label in cases)
    for family in ("t=#", "w=#", "w=random rejected", "w=random accepted", "z=# t=#", "z=# w=#", "d=# t=#", "d=# w=#",
                   "precedence z+N", "precedence d+N", "precedence k+N", "precedence d=#", "precedence k=#",
                   "precedence d=N", "precedence k=N", "precedence z=#^#", "k #^#", "k #^#-#", "k n-#^#", "k one", "k n-#",
                   "k (n-#)/#", "k (n+#)/#", "k w# digit full-# in window #", "k w# digit full in window #",
                   "k w# every digit #",
                   "k #.. # bits", "k #.. # bits mod N", "k #.. # bits >> #", "k extreme felt #"):
        assert by_label[family] > 0, family
    # what the labels promise
    for z, d, k, label in cases:
        status, _, _, kind = C.attempt_kind(z, d, k)
        if label.startswith("precedence"):
            assert status == C.BAD_INPUT, label
        elif label.endswith("t=0"):
            assert kind == "retry_t" and z < TWO251 and 0 < d < N, label
        elif " w=" in " " + label and "random" not in label:
            w = int(label.rsplit("w=", 1)[1], 16)
            assert kind == ("ok" if w < TWO251 else "retry_w"), label
            assert k * pow(z + C.r_of(k) * d, -1, N) % N == w, label
        elif label == "w=random rejected":
            assert kind == "retry_w"
        elif label.startswith("k "):
            assert status in (C.OK, C.RETRY), label
    assert {z for z, _, _, label in cases if label.startswith("z=")} == {0, 1, TWO251 - 1}
    assert {d for _, d, _, label in cases if label.startswith("d=")} == {1, 2, N - 1}
    for t in (1, N - 1):
        assert sum(1 for z, d, k, _ in cases if 0 < k < N and 0 < d < N and (z + C.r_of(k) * d) % N == t) >= 4


def test_scalar_patterns_cover_every_window_position():
    ks = dict(C.scalar_patterns())
    assert all(0 < k < N for k in ks)
    for i in range(252):
        assert 2**i in ks and N - 2**i in ks and (i == 0 or 2**i - 1 in ks)
    for w in C.WINDOW_WIDTHS:
        nwin = -(-252 // w)
        for j in range(nwin):
            assert 1 << (w * j) in ks
            if ((2**w - 1) << (w * j)) < N:
                assert (2**w - 1) << (w * j) in ks
        assert nwin * w >= 252 > (nwin - 1) * w


def test_ok_cases_verify_under_the_reference(cases):
    """Every accepted attempt is a signature the reference's verify() accepts under d G (z = 0 is signable, but the
    AIR-style verify() cannot multiply by 0 and answers False: signature.py:176-190, 251-257)."""
    C.prime_r([d for _, d, _, _ in cases])
    from oracle import cref
    ok = [(z, d, k) + C.attempt(z, d, k)[1:] for z, d, k, _ in cases if C.attempt(z, d, k)[0] == C.OK]
    pubs = cref.public_keys_many([d for _, d, _, _, _ in ok])
    assert pubs[:8] == [R.private_key_to_ec_point_on_stark_curve(d) for _, d, _, _, _ in ok[:8]]
    for (z, d, k, r, s), q in zip(ok, pubs):
        assert 1 <= r < TWO251 and 1 <= s < N
        assert R.verify(z, r, s, q) is (z != 0), (hex(z), hex(d), hex(k))


def test_attempt_is_the_body_of_the_reference_sign(pool):
    rng = random.Random(1)
    sample = [(rng.randrange(TWO251), rng.randrange(1, N), rng.choice([None, 1, 300, 2**40])) for _ in range(12)]
    sample += [(z, d, seed) for z, d, seed, _, _ in pool[::4]]
    for z, d, seed in sample:
        k = R.generate_k_rfc6979(z, d, seed)
        assert C.rejections(z, d, seed)[1] == k
        assert C.attempt(z, d, k) == (C.OK,) + tuple(R.sign(z, d, seed))
    assert C.attempt(TWO251, 5, 7)[0] == C.attempt(5, 0, 7)[0] == C.attempt(5, N, 7)[0] == C.BAD_INPUT
    assert C.attempt(5, 7, 0)[0] == C.attempt(5, 7, N)[0] == C.BAD_INPUT


def test_pool_counts_and_signatures_do_not_drift(pool):
    assert len(pool) >= 32
    for seed, count in C.POOL_SEEDS.items():
        assert C.rejections(C.POOL_Z, C.POOL_D, seed)[0] == count, seed
    counts = [c for _, _, _, c, _ in pool]
    assert set(C.POOL_COUNTS) <= set(counts)
    for z, d, seed, count, sig in pool:
        assert z < TWO251 and 0 < d < N and (seed is None or 0 <= seed < 2**64)
        n_rej, k = C.rejections(z, d, seed)
        assert n_rej == count and k == R.generate_k_rfc6979(z, d, seed)
        assert tuple(sig) == tuple(R.sign(z, d, seed)) == C.attempt(z, d, k)[1:]
    seeds = [seed for _, _, seed, _, _ in pool]
    assert None in seeds and 0 in seeds
    assert {1, 2, 4, 5, 8} <= {(s.bit_length() + 7) // 8 for s in seeds if s}
    assert any(z.bit_length() >= 248 and 1 <= z.bit_length() % 8 <= 4 for z, _, _, _, _ in pool)  # the pad rule
    assert any(z.bit_length() == 248 for z, _, _, _, _ in pool) and any(z == 0 for z, _, _, _, _ in pool)
    for z, d, seed in C.INVALID_ITEMS:
        assert C.attempt(z, d, 1)[0] == C.BAD_INPUT


def test_round_of_restates_the_pipeline():
    """A change of ROUNDS, of the threshold or of the device's seed budget in csrc/ecdsa.hip fails here: the pool of
    tests/sign_cases.py (POOL_COUNTS) and the sizes of tests/test_gpu_sign_edges.py are chosen for these values."""
    src = open(os.path.join(ROOT, "stark-perpetual_amd", "csrc", "ecdsa.hip")).read()
    assert int(re.search(r"constexpr int ROUNDS = (\d+);", src).group(1)) == C.ROUNDS
    assert int(re.search(r'getenv\("STARKPERP_SIGN_COMPACT_MIN"\);[^\n]*\n[^\n]*\(size_t\)(\d+);', src).group(1)) == C.COMPACT_MIN
    assert set(int(v) for v in re.findall(r"for \(int attempt = 0; attempt < (\d+); \+\+attempt\)", src)) == {C.DEVICE_SEEDS}
    assert "counters + ROUNDS, m, 64, kbuf" in src  # the straggler launch reads the list that ROUNDS launches left
    assert [C.round_of(c) for c in (0, 1, 2, 9, 10, 11, 12, 14)] == [0, 1, 2, 9, 10, 11, 11, 11]
    assert C.round_of(C.ROUNDS) == C.ROUNDS and C.round_of(C.ROUNDS + 1) == C.round_of(64) == C.ROUNDS + 1
    # every launch of the pipeline accepts an item of the pool: first, each end of the rounds, stragglers
    assert {C.round_of(c) for c in C.POOL_COUNTS} >= {0, 1, 2, C.ROUNDS - 1, C.ROUNDS, C.ROUNDS + 1}
    assert sum(1 for c in C.POOL_COUNTS if C.round_of(c) == C.ROUNDS + 1) >= 3


def test_batch_patterns(pool):
    counts = [c for _, _, _, c, _ in pool]
    for n in (1, 63, 64, 65, 129, 4097):
        pats = C.batch_patterns(n, pool)
        assert set(pats) == {"uniform_1", "uniform_10", "uniform_11", "shuffle", "wave_lane0", "wave_lane63", "wave_all",
                             "wave_none", "wave_alternating", "invalid_interleaved"}
        for name, idx in pats.items():
            assert len(idx) == n and all(0 <= i < len(pool) + len(C.INVALID_ITEMS) for i in idx), name
        rejected = {name: [i < len(pool) and counts[i] > 0 for i in idx] for name, idx in pats.items()}
        for c in (1, 10, 11):
            assert {counts[i] for i in pats["uniform_%d" % c]} == {c}
        assert rejected["wave_lane0"] == [i % 64 == 0 for i in range(n)]
        assert rejected["wave_lane63"] == [i % 64 == 63 for i in range(n)]
        assert all(rejected["wave_all"]) and not any(rejected["wave_none"])
        assert rejected["wave_alternating"] == [i % 2 == 1 for i in range(n)]
        bad = pats["invalid_interleaved"]
        assert bad[-1] >= len(pool)
        zs, ds, seeds, status, sigs = C.expand(bad, pool)
        assert status[-1] == C.BAD_INPUT and sigs[-1] == (0, 0)
        if n >= 64:
            assert {i - len(pool) for i in bad if i >= len(pool)} == {0, 1, 2} and C.OK in status
    # neighbouring chunks of 4096 carry different seeds at most positions of the shuffle: a chunk that read the seeds
    # (or wrote the status) of another chunk cannot give the expected signatures
    idx = C.batch_patterns(12325, pool)["shuffle"]
    seeds = C.expand(idx, pool)[2]
    assert sum(1 for i in range(4096, 12325) if seeds[i] != seeds[i - 4096]) > 7000
    assert sum(1 for i in range(4096, 12325) if seeds[i] != seeds[i % 4096]) > 7000
