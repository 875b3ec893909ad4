"""The dense C reference of the prover's transforms (oracle/starkref.c cref_ntt, cref_lde, cref_interpolate,
cref_coset_eval through oracle/cref.py) against oracle/stark_ref.py at the sizes Python lists reach, and against Horner
evaluation - the definition of a transform's output - at 2^16 and 2^20 points, where nothing else can check it."""
import random

import numpy as np
import pytest

import transform_cases as cases
import workloads as wl
from oracle import cref, stark_ref as S

P = S.P


def _columns(log_n, seed):
    """(name, ints) inputs of one size: random felts, and the extreme limb patterns (cycled through a shuffled list, so
    that all of them pass through the sizes that can hold them)."""
    n = 1 << log_n
    rng = random.Random(seed)
    ext = list(wl.extreme_felts())
    rng.shuffle(ext)
    return [("random", [rng.randrange(P) for _ in range(n)]),
            ("extreme", [ext[(i + log_n) % len(ext)] for i in range(n)])]


@pytest.mark.parametrize("log_n", range(0, 11))
def test_ntt_and_intt_equal_the_python_oracle(log_n):
    w = S.root_of_unity(log_n)
    for name, c in _columns(log_n, 100 + log_n):
        a = cases.felts_from_ints(c)
        assert cases.ints_from_felts(cref.ntt_dense(a)) == S.ntt(c, w), name
        assert cases.ints_from_felts(cref.ntt_dense(a, inverse=True)) == S.intt(c, w), name
        assert cases.ints_from_felts(a) == c  # the input array is left alone


LDE_SHAPES = [(log_n, b) for log_n in range(0, 7) for b in range(0, 5)] + [(0, 12), (2, 12), (1, 13)]


@pytest.mark.parametrize("log_n,log_blowup", LDE_SHAPES)
def test_lde_equals_the_python_oracle(log_n, log_blowup):
    rng = random.Random(1000 * log_n + log_blowup)
    cols = [c for _, c in _columns(log_n, 200 + log_n)]
    a = np.stack([cases.felts_from_ints(c) for c in cols])
    for shift in (3, P - 1, rng.randrange(1, P)):
        got = cref.lde_dense(a, log_blowup, shift)
        assert got.shape == (2, 1 << (log_n + log_blowup), 4) and got.dtype == np.uint64
        for c, g in zip(cols, got):
            assert cases.ints_from_felts(g) == S.lde(c, 1 << log_blowup, shift), shift


@pytest.mark.parametrize("log_n", (0, 1, 5, 8))
def test_interpolate_and_coset_eval_are_the_two_halves_of_the_lde(log_n):
    n = 1 << log_n
    rng = random.Random(300 + log_n)
    for _, c in _columns(log_n, 300 + log_n):
        coef = cref.interpolate_dense(cases.felts_from_ints(c))
        plain = S.intt(c, S.root_of_unity(log_n))
        rev = [int(format(k, "0%db" % log_n)[::-1], 2) if log_n else 0 for k in range(n)]
        assert cases.ints_from_felts(coef) == [n * plain[rev[j]] % P for j in range(n)]  # n c_k at the bit-reversed index
        for shift in (3, P - 1, rng.randrange(1, P)):
            assert cases.ints_from_felts(cref.coset_eval_dense(coef, shift)) == S.lde(c, 1, shift)


def test_horner_is_the_definition():
    rng = random.Random(5)
    c = [rng.randrange(P) for _ in range(37)]  # any length, not only powers of two
    xs = [0, 1, P - 1, 3] + [rng.randrange(P) for _ in range(5)]
    want = [sum(v * pow(x, k, P) for k, v in enumerate(c)) % P for x in xs]
    assert cases.ints_from_felts(cref.horner_dense(cases.felts_from_ints(c), xs)) == want
    assert cases.ints_from_felts(cref.horner_dense(cases.felts_from_ints(c[:1]), xs)) == [c[0]] * len(xs)


@pytest.mark.parametrize("log_n", (16, 20))
def test_dense_ntt_equals_horner_at_16_positions_and_inverts(log_n):
    n = 1 << log_n
    a = cases.random_column(n, seed=log_n)
    ev = cref.ntt_dense(a)
    rng = random.Random(log_n)
    spots = [0, 1, n // 2, n - 1] + rng.sample(range(2, n - 1), 12)
    assert len(set(spots)) == 16
    w = S.root_of_unity(log_n)
    want = cref.horner_dense(a, [pow(w, i, P) for i in spots])
    assert np.array_equal(ev[spots], want)
    assert cases.is_canonical(ev).all()
    assert np.array_equal(cref.ntt_dense(ev, inverse=True), a)
