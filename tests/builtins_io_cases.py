"""Cases of the builtins proof's boundary constraints, shared by tests/test_builtins_io_ref_cpu.py (the g++ shim of
csrc/builtins_boundary.hpp, no GPU) and tests/test_gpu_builtins_io.py: honest combined traces in integers for all 7
segment sets, each at the smallest log_n its segments admit and one size larger, the statement of each, the lying
claims, arbitrary columns with rows of EXTREMES, and the positions at which point form and dense form are compared.
Seeded and cached; neither torch nor the library is imported."""
import functools
import random

import builtins_io_ref as IO
import builtins_verify_cases as BV
from builtins_verify_cases import EXTREMES, NOT_FELTS, SEGMENT_SETS, felts_np, ints_of, mask_of, min_log_n  # noqa: F401
from oracle import ref_py as R
from oracle import stark_ref as S

P = S.P
OTHER_SHIFT = 0x123456789ABCDEF0123456789
SIZES = tuple((segs, min_log_n(segs) + up) for segs in SEGMENT_SETS for up in (0, 1))
size_id = lambda v: "+".join(v) if isinstance(v, tuple) else str(v)


def n_cols(segments):
    return sum(IO.SEG_DESC[s]["n_cols"] for s in segments)


def n_groups(segments):
    return sum(len(IO.SEG_DESC[s]["rows"]) for s in segments)


def rc_values_for(n, rng):
    """Values whose fill fits n / 8 cells: one value with the limbs lo .. lo + 7 in some order when there is one cell,
    else half as many values as cells with limbs in a band four times their number wide (at most one pad per two)."""
    cells = n // 8
    if cells == 1:
        limbs = list(range(300, 308))
        rng.shuffle(limbs)
        return [sum(l << (16 * k) for k, l in enumerate(limbs))]
    count = cells // 2
    return [sum(rng.randrange(300, 300 + 4 * count) << (16 * k) for k in range(8)) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _signature(i):
    rng = random.Random("builtins-io-sig-%d" % i)
    while True:
        z, d = rng.randrange(1, 2**251), rng.randrange(1, R.EC_ORDER)
        r, s = R.sign(z, d)
        if 1 <= R.inv_mod_curve_size(s) < 2**251:
            return (z, r, s, tuple(R.private_key_to_ec_point_on_stark_curve(d)))


@functools.lru_cache(maxsize=None)
def instances(segments, log_n):
    """(hash inputs, signatures, rc values) as prove_builtin_usage takes them, filling n = 2^log_n rows exactly."""
    n = 1 << log_n
    rng = random.Random("builtins-io-%s-%d" % ("+".join(segments), log_n))
    hashes = [(rng.randrange(P), rng.randrange(P)) for _ in range(n // 512)] if "pedersen" in segments else []
    sigs = [_signature(i) for i in range(n // 1024)] if "ecdsa" in segments else []
    values = rc_values_for(n, rng) if "rc16" in segments else []
    return hashes, sigs, values


@functools.lru_cache(maxsize=None)
def honest(segments, log_n):
    """(trace columns [n_cols][n], public inputs, trace LDE [n_cols][4 n]) of the honest combined trace."""
    n = 1 << log_n
    hashes, sigs, values = instances(segments, log_n)
    cols, pub = [], {}
    if "pedersen" in segments:
        ped = S.pedersen_trace(hashes)
        cols += ped
        pub["hashes"] = [[x, y, ped[1][512 * i + 511]] for i, (x, y) in enumerate(hashes)]
    if "ecdsa" in segments:
        cols += S.ecdsa_trace([S.ecdsa_instance(z, r, s, q) for z, r, s, q in sigs])
        pub["signatures"] = [[z, r, s, q[0], q[1]] for z, r, s, q in sigs]
    if "rc16" in segments:
        padded, lo, hi = S.rc16_fill(values, n // 8)
        cols += S.rc16_trace(padded)
        pub.update(rc_min=lo, rc_max=hi, rc_values=list(values))
    assert len(cols) == n_cols(segments) and all(len(c) == n for c in cols)
    return cols, pub, [S.lde(c) for c in cols]


def values_of(segments, pub, n):
    return {s: IO.term_values(s, pub, n) for s in segments}


def lies(segments, pub):
    """[(what, segment, lying public inputs)]: one public value changed per claim, in the last instance; the
    range-checked values swapped (or, with one value, its limbs permuted), so that the limb set stays."""
    out = []

    def put(what, seg, key, edit):
        bad = dict(pub)
        bad[key] = [list(v) if isinstance(v, list) else v for v in pub[key]]
        edit(bad[key])
        out.append((what, seg, bad))
    if "pedersen" in segments:
        for c, what in enumerate(("hash x", "hash y", "hash h")):
            put(what, "pedersen", "hashes", lambda h, c=c: h[-1].__setitem__(c, (h[-1][c] + 1) % P))
    if "ecdsa" in segments:
        other = R.private_key_to_ec_point_on_stark_curve(12345)
        for c, what in enumerate(("sig z", "sig r", "sig s")):
            put(what, "ecdsa", "signatures", lambda g, c=c: g[-1].__setitem__(c, g[-1][c] + 1))
        put("sig Q", "ecdsa", "signatures", lambda g: g[-1].__setitem__(slice(3, 5), list(other)))
    if "rc16" in segments:
        def swap(v):
            if len(v) == 1:
                limbs = [(v[0] >> (16 * k)) & 0xFFFF for k in range(8)]
                v[0] = sum(l << (16 * k) for k, l in enumerate(limbs[1:] + limbs[:1]))
            else:
                i = next(i for i in range(1, len(v)) if v[i] != v[0])
                v[0], v[i] = v[i], v[0]
        put("rc values swapped", "rc16", "rc_values", swap)
    return out


def positions(M, seed=0, count=40):
    """Every position where M <= 257, else the edges of builtins_verify_cases and seeded positions."""
    if M <= 257:
        return list(range(M))
    rng = random.Random("builtins-io-pos-%d-%d" % (M, seed))
    return list(dict.fromkeys(BV.edge_positions(M))) + [rng.randrange(M) for _ in range(count)]


def arbitrary_columns(count, size, seed):
    """Columns of seeded felts in which about one value in four is one of EXTREMES."""
    rng = random.Random("builtins-io-arb-%s" % (seed,))
    return [[rng.choice(EXTREMES) if rng.random() < 0.25 else rng.randrange(P) for _ in range(size)] for _ in range(count)]


def arbitrary_pub_lde(segments, M, seed):
    """segment -> its groups' columns, arbitrary."""
    return {s: arbitrary_columns(len(IO.SEG_DESC[s]["rows"]), M, (seed, s)) for s in segments}


def arbitrary_coefficients(segments, n, seed):
    return {s: arbitrary_columns(len(IO.SEG_DESC[s]["rows"]), n // IO.SEG_DESC[s]["period"], (seed, s, "coef"))
            for s in segments}


# sp_boundary_combine_dev: (n_groups, term_groups) - 1 .. 8 terms, groups in order and out of order
COMBINE_SHAPES = ((1, (0,)), (1, (0, 0)), (3, (0, 1, 2)), (2, (1, 0, 1, 0)), (3, (0, 1, 1, 1, 2)), (3, (2, 2, 0, 1, 0, 2)),
                  (4, (0, 0, 0, 1, 2, 3, 3)), (4, (3, 0, 0, 0, 0, 1, 2, 0)))
COMBINE_KS = (1, 2, 4096)


def combine_case(n_groups, term_groups, k):
    """(columns, alphas, expected per group) with extreme values and challenges; columns hold any 256-bit value."""
    cols = arbitrary_columns(len(term_groups), k, ("combine", n_groups, term_groups, k))
    cols[0][k - 1] = 2**256 - 1
    alphas = arbitrary_columns(1, len(term_groups), ("combine-alpha", term_groups, k))[0]
    want = [[0] * k for _ in range(n_groups)]
    for d, col, a in zip(term_groups, cols, alphas):
        want[d] = [(acc + a * x) % P for acc, x in zip(want[d], col)]
    return cols, alphas, want
