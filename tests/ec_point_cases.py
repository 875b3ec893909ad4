"""Inputs and expected answers of the batch point arithmetic on the Stark curve (k P, a G + b P, P +- Q), shared by
tests/test_ec_points_cpu.py (the host build of the per-item code) and tests/test_gpu_ec_points.py (the library).
Everything here is Python integers: multiples come from a small Jacobian double-and-add below, which this module checks
against starkperp.math_utils.ec_mult on a handful of items when it is imported; sums of two points come from
math_utils.ec_add / ec_double directly.

A case is (inputs..., status, result): result is (x, y) for OK and None otherwise."""
import json
import os
import random

from starkperp import math_utils as MU

P = 2**251 + 17 * 2**192 + 1
N = 0x800000000000010FFFFFFFFFFFFFFFFB781126DCAE7B2321E66A241ADC64D2F  # EC_ORDER
BETA = 0x6F21413EFBE40DE150E596D72F7A8C5609AD26C15C915C1F4CDFCB99CEE9E89
GEN = (0x1EF15C18599971B7BECED415A40F0C7DEACFD9B0D1819E03D723D8BC943CFCA,
       0x5668060AA49730B7BE4801DF46EC62DE53ECD11ABE43A32873000C36E8DC1F)
OK, INFINITY, OUT_OF_RANGE, NOT_ON_CURVE = 0, 1, 2, 3  # include/starkperp.h SP_EC_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOO_BIG = [P, P + 1, 2**256 - 1]        # coordinates that are out of range
BAD_SCALARS = [N, N + 1, 2**256 - 1]    # scalars that are out of range


def on_curve(pt):
    x, y = pt
    return (y * y - x * x * x - x - BETA) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


assert on_curve(GEN)


# ---- k * pt in Jacobian coordinates (dbl-2007-bl / add-2007-bl with a = 1), None = infinity ----
def _jdbl(X, Y, Z):
    if Y == 0 or Z == 0:
        return 0, 1, 0
    XX, YY, ZZ = X * X % P, Y * Y % P, Z * Z % P
    S = 4 * X * YY % P
    M = (3 * XX + ZZ * ZZ) % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - 8 * YY * YY) % P, 2 * Y * Z % P


def _jadd_affine(X, Y, Z, pt):
    if Z == 0:
        return pt[0], pt[1], 1
    ZZ = Z * Z % P
    H = (pt[0] * ZZ - X) % P
    R = (pt[1] * ZZ * Z - Y) % P
    if H == 0:
        return _jdbl(X, Y, Z) if R == 0 else (0, 1, 0)
    HH = H * H % P
    HHH, V = H * HH % P, X * HH % P
    X3 = (R * R - HHH - 2 * V) % P
    return X3, (R * (V - X3) - Y * HHH) % P, Z * H % P


def mul(k, pt):
    """k * pt for any integer k >= 0 and an affine pt; None for infinity."""
    k %= N
    acc = (0, 1, 0)
    for bit in bin(k)[2:] if k else "":
        acc = _jdbl(*acc)
        if bit == "1":
            acc = _jadd_affine(*acc, pt)
    X, Y, Z = acc
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


_G_CACHE = {}


def gmul(k):
    """(k mod N) * EC_GEN, cached: the expected value of everything whose base has a known discrete logarithm."""
    k %= N
    if k not in _G_CACHE:
        _G_CACHE[k] = mul(k, GEN)
    return _G_CACHE[k]


def add(p1, p2):
    """p1 + p2 with None as infinity, through math_utils' affine formulas wherever they apply."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        return MU.ec_double(p1, 1, P) if p1[1] == p2[1] else None
    return MU.ec_add(p1, p2, P)


for _k in (1, 2, 3, 30, N - 30, 0x1234567890ABCDEF << 180):
    assert mul(_k, GEN) == MU.ec_mult(_k, GEN, 1, P), hex(_k)
assert mul(N, GEN) is None and mul(N - 1, GEN) == neg(GEN)


# ---- scalars ----
def edge_scalars():
    """Small values and window edges, powers of two and their neighbours, values near the group order (the negation
    path of even scalars, and N - 30 / 30: the one place where the ladder's last addition meets its own operand)."""
    out = [0, 1, 2, 3, 15, 16, 17, 29, 30, 31, 32, 33]
    for j in (4, 8, 128, 248, 251):
        out += [2**j - 1, 2**j, 2**j + 1]
    out += [(N - 1) // 2, (N + 1) // 2, N - 1, N - 2, N - 3, N - 15, N - 16, N - 17, N - 29, N - 30, N - 31, N - 32, N - 33]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    assert all(0 <= k < N for k in uniq)
    return uniq


def random_scalars(n=64, seed=20261019):
    rng = random.Random(seed)
    return [rng.randrange(1, N) for _ in range(n)]


# ---- points with a known discrete logarithm: [(t, (x, y))] with (x, y) = t * EC_GEN ----
def golden_keys(n=12):
    keys = json.load(open(os.path.join(GOLDEN, "g2_keys.json")))["keys"]
    step = len(keys) // n
    return [(int(d, 16), (int(x, 16), int(y, 16))) for d, x, y in keys[::step][:n]]


def known_points():
    pts = [(1, GEN), (N - 1, neg(GEN))] + golden_keys()
    assert all(on_curve(pt) for _, pt in pts)
    return pts


def off_curve_points():
    return [(GEN[0], GEN[1] + 1), (0, 0)]


def _mult_expect(k, t):
    r = gmul(k * t)
    return (OK, r) if r is not None else (INFINITY, None)


def mult_cases():
    """[(k, (px, py), status, result)]: every edge scalar on EC_GEN and on one of the other points in turn, the random
    scalars on the points in turn, then everything that has to be refused - range before curve."""
    pts = known_points()
    cases = []
    for i, k in enumerate(edge_scalars()):
        for t, pt in (pts[0], pts[1 + i % (len(pts) - 1)]):
            cases.append((k, pt) + _mult_expect(k, t))
    for i, k in enumerate(random_scalars()):
        t, pt = pts[i % len(pts)]
        cases.append((k, pt) + _mult_expect(k, t))
    for k in BAD_SCALARS:
        cases.append((k, GEN, OUT_OF_RANGE, None))
    for bad in off_curve_points():
        cases.append((5, bad, NOT_ON_CURVE, None))
        cases.append((0, bad, NOT_ON_CURVE, None))      # checked even when the scalar is 0
        cases.append((N, bad, OUT_OF_RANGE, None))       # range wins over the curve
    for big in TOO_BIG:
        cases.append((5, (big, GEN[1]), OUT_OF_RANGE, None))   # off the curve as well: range wins
        cases.append((5, (GEN[0], big), OUT_OF_RANGE, None))
        cases.append((0, (big, big), OUT_OF_RANGE, None))
    return cases


def lincomb_cases():
    """[(a, b, (px, py), status, result)] on P = t G with t known."""
    pts = known_points()
    rng = random.Random(20261020)
    cases = []

    def put(a, b, t, pt):
        r = gmul(a + b * t)
        cases.append((a % N, b % N, pt, OK if r is not None else INFINITY, r))

    for t, pt in pts[:5]:  # EC_GEN (t = 1: a = N - b, a = b), -EC_GEN, three golden keys
        for b in (rng.randrange(1, N), 30, N - 30, 1, N - 1):
            put(-b * t, b, t, pt)          # b P == -(a G): infinity
            put(b * t, b, t, pt)           # b P == a G: the sum is a doubling
            assert cases[-2][3] == INFINITY and cases[-1][4] == add(gmul(b * t), gmul(b * t))
        b = rng.randrange(1, N)
        put(0, b, t, pt)
        put(b, 0, t, pt)
        put(0, 0, t, pt)
        put(0, 30, t, pt)
        put(30, N - 30, t, pt)
    for i in range(64):
        t, pt = pts[i % len(pts)]
        put(rng.randrange(N), rng.randrange(N), t, pt)
    for k in BAD_SCALARS:
        cases.append((k, 1, GEN, OUT_OF_RANGE, None))
        cases.append((1, k, GEN, OUT_OF_RANGE, None))
    for bad in off_curve_points():
        cases.append((1, 1, bad, NOT_ON_CURVE, None))
        cases.append((0, 0, bad, NOT_ON_CURVE, None))
        cases.append((1, N, bad, OUT_OF_RANGE, None))
    for big in TOO_BIG:
        cases.append((1, 1, (big, GEN[1]), OUT_OF_RANGE, None))
        cases.append((1, 0, (GEN[0], big), OUT_OF_RANGE, None))
    return cases


def add_cases():
    """[((px, py), (qx, qy), subtract, status, result)]"""
    pts = [pt for _, pt in known_points()]
    rng = random.Random(20261021)
    cases = []

    def put(p1, p2, subtract):
        r = add(p1, neg(p2) if subtract else p2)
        cases.append((p1, p2, subtract, OK if r is not None else INFINITY, r))

    for pt in pts:
        put(pt, pt, 0)         # P + P: the doubling
        put(pt, neg(pt), 0)    # P + (-P): infinity
        put(pt, pt, 1)         # P - P: infinity
        put(pt, neg(pt), 1)    # P - (-P): the doubling
    for _ in range(32):
        p1, p2 = rng.sample(pts, 2)
        put(p1, p2, rng.randrange(2))
    for sub in (0, 1):
        for bad in off_curve_points():
            cases.append((GEN, bad, sub, NOT_ON_CURVE, None))
            cases.append((bad, GEN, sub, NOT_ON_CURVE, None))
            cases.append((bad, (P, GEN[1]), sub, OUT_OF_RANGE, None))   # range of Q wins over the curve of P
        for big in TOO_BIG:
            cases.append(((big, GEN[1]), GEN, sub, OUT_OF_RANGE, None))
            cases.append((GEN, (GEN[0], big), sub, OUT_OF_RANGE, None))
    return cases


def pick_mixed(cases, n, seed):
    """n cases drawn with repetition in groups of eight - five OK and one of each other status, shuffled - so that any
    16 consecutive items, wherever a slice starts, mix all four statuses inside one wave."""
    rng = random.Random(seed)
    by_status = {s: [c for c in cases if c[-2] == s] for s in (OK, INFINITY, OUT_OF_RANGE, NOT_ON_CURVE)}
    assert all(by_status.values())
    out = []
    while len(out) < n:
        group = [rng.choice(by_status[s]) for s in (OK, OK, OK, OK, OK, INFINITY, OUT_OF_RANGE, NOT_ON_CURVE)]
        rng.shuffle(group)
        out += group
    return out[:n]
