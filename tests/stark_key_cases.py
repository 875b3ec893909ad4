"""Inputs and expected answers of the square-root / x-only-key batches, shared by tests/test_felt_sqrt_cpu.py (the host
build of the per-item code) and tests/test_gpu_stark_keys.py (the library).  Everything here is Python integers: the
expected roots of the digit sweep come from pow() on the exponent, the status of anything else from Euler's criterion."""
import json
import os
import random

P = 2**251 + 17 * 2**192 + 1
M = 2**59 + 17                # p - 1 = 2^192 * M
G = pow(3, M, P)              # generates the subgroup of order 2^192
W, DIGITS = 8, 24             # the digit width csrc/fp29.hpp chose (SQRT_W, SQRT_DIGITS)
BETA = 0x6F21413EFBE40DE150E596D72F7A8C5609AD26C15C915C1F4CDFCB99CEE9E89
OK, NON_RESIDUE, OUT_OF_RANGE = 0, 1, 2  # include/starkperp.h SP_SQRT_*
MAX_OPS = 3700                # a fifth of the 192 * 193 / 2 = 18 528 squarings of the bit-by-bit method
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

assert pow(G, 2**191, P) == P - 1


def smaller(r):
    return min(r, P - r)


def euler_status(a):
    """The status of a felt by Euler's criterion; 0 counts as a residue (sympy's is_quad_residue)."""
    if a >= P:
        return OUT_OF_RANGE
    return OK if a == 0 or pow(a, (P - 1) // 2, P) == 1 else NON_RESIDUE


def power_case(e):
    """(a, status, root) for a = g^e."""
    a = pow(G, e, P)
    return (a, NON_RESIDUE, None) if e & 1 else (a, OK, smaller(pow(G, e // 2, P)))


def basic_cases():
    """0, 1, 4, p - 1 (root of order 4: only the top digit is set), 3 (a non-residue), g (e = 1)."""
    top = power_case(2**191)
    assert top[0] == P - 1
    return [(0, OK, 0), (1, OK, 1), (4, OK, 2), top, (3, NON_RESIDUE, None), power_case(1)]


def digit_sweep():
    """Every digit value of every window: a = g^(d * 2^(W k)); the odd d of window 0 are the non-residues."""
    return [power_case(d << (W * k)) for k in range(DIGITS) for d in range(1 << W)]


def all_digits_maximal():
    return power_case(2**192 - 2)


def random_squares(n=256, seed=20261019):
    """n seeded squares and their negations (p = 1 mod 4: residues as well, with other roots)."""
    rng = random.Random(seed)
    sq = [pow(rng.randrange(1, P), 2, P) for _ in range(n)]
    return sq + [P - a for a in sq]


def rhs(x):
    return (x * x * x + x + BETA) % P


def golden_keys():
    """[(pub_x, min(pub_y, p - pub_y))] of tests/golden/g2_keys.json (reference output)."""
    keys = json.load(open(os.path.join(GOLDEN, "g2_keys.json")))["keys"]
    return [(int(x, 16), smaller(int(y, 16))) for _, x, y in keys]


def off_curve_key():
    cases = json.load(open(os.path.join(GOLDEN, "g4_verify.json")))["cases"]
    (case,) = [c for c in cases if c["label"] == "off_curve_xonly"]
    return int(case["key"], 16)


def valid_xonly_rows(n=16):
    cases = json.load(open(os.path.join(GOLDEN, "g4_verify.json")))["cases"]
    rows = [c for c in cases if c["label"] == "valid_xonly"][:n]
    assert len(rows) == n
    return [tuple(int(c[k], 16) for k in ("z", "r", "s", "key")) for c in rows]


def mixed_felts(n, seed=7):
    """A seeded mix of residues, non-residues and out-of-range felts (p, 2^256 - 1) for the launch-shape tests."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        kind = rng.randrange(8)
        if kind == 0:
            out.append(P if rng.randrange(2) else 2**256 - 1)
        elif kind < 4:
            out.append(pow(rng.randrange(1, P), 2, P))
        else:
            out.append(rng.randrange(1, P))
    return out


def check_root(a, status, root):
    """status / root of one felt against Euler's criterion and the definition of the smaller root."""
    assert status == euler_status(a), hex(a)
    if status == OK:
        assert root * root % P == a and root <= P - root, hex(a)
