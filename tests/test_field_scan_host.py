"""The product-scanning forms of csrc/fp29.hpp (fe_mul_scan, fe_sqr_scan, fe_mul_sub_mul_scan, fe_mul_add_mul_scan,
fe_mul3_add_scan: a column's multiply-add chain starts from the carry of the column before it) against the column
forms they stand beside, on the host: g++ with SP_CHECK_BOUNDS, so every accumulate step of a scan form is checked
against the 64-bit column budget and an overflow aborts the process.

  * limb for limb equal to the column forms on 120 000 random N-form elements (limbs 0..7 in [0, 2^29), limb 8 in
    [-2^21, 2^21]: value in (-4p, 4p) and a little beyond) and on every 6-tuple of the extreme patterns - all limbs
    2^29 - 1, all 0, limb 8 at both ends of its range over all-zero and all-ones low limbs - that is every pattern in
    every operand position of every form;
  * equal to Python integers modulo p (through fe_canon; a product carries the Montgomery factor 2^-261);
  * the XYZZ additions of csrc/curve.hpp instantiated with both forms give the same limbs: their lazy differences
    are operands the bare forms above never see, and the scan instances of madd / madd_x_only / mmadd run two or
    three multiplications through one interleaved scan (fe_scan with several chains)."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import ref_py as R

HERE = os.path.dirname(os.path.abspath(__file__))
P = R.FIELD_PRIME
NL, LB = 9, 29
MASK = (1 << LB) - 1
RINV = pow(1 << (NL * LB), -1, P)
L8 = 1 << 21  # limb 8 of a value in (-4p, 4p) lies in [-2^21, 2^21]
OPS = ("fe_mul", "fe_sqr", "fe_mul_sub_mul", "fe_mul_add_mul", "fe_mul3_add")


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "host", "field_scan_shim.cpp")
    so = os.path.join(HERE, "host", "field_scan_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    for f in (lib.t_scan_compare, lib.t_scan_compare_xyzz, lib.t_scan_compare_tuples):
        f.restype = ctypes.c_long
    lib.t_scan_compare.argtypes = lib.t_scan_compare_xyzz.argtypes = [ctypes.c_void_p, ctypes.c_long]
    return lib


def patterns():
    ones, zero = [MASK] * 8, [0] * 8
    return [ones + [MASK], zero + [0], zero + [-L8], ones + [-L8], zero + [L8], ones + [L8]]


def random_elements(n, seed):
    rng = random.Random(seed)
    return [[rng.getrandbits(LB) for _ in range(8)] + [rng.randint(-L8, L8)] for _ in range(n)]


def pack(elems):
    return (ctypes.c_int32 * (NL * len(elems)))(*[l for e in elems for l in e])


def value(limbs):
    return sum(l << (LB * i) for i, l in enumerate(limbs))


def expected(op, v):
    a, b, c, d, e, f = v
    t = {"fe_mul": a * b, "fe_sqr": a * a, "fe_mul_sub_mul": a * b - c * d, "fe_mul_add_mul": a * b + c * d,
         "fe_mul3_add": a * b + c * d + e * f}[op]
    return t * RINV % P


def test_scan_forms_equal_column_forms_on_random_elements(shim):
    elems = random_elements(120000, seed=2901)
    bad = shim.t_scan_compare(pack(elems), len(elems))
    assert bad == -1, "item %d, %s" % (bad // 16, OPS[bad % 16])


def test_scan_forms_equal_column_forms_on_extreme_patterns_in_every_position(shim):
    pats = patterns()
    bad = shim.t_scan_compare_tuples(pack(pats), len(pats))
    assert bad == -1, "tuple %d, %s" % (bad // 16, OPS[bad % 16])


def test_scan_forms_equal_python_integers(shim):
    rng = random.Random(2902)
    pats, rnd = patterns(), random_elements(64, seed=2903)
    tuples = [[rng.choice(pats) for _ in range(6)] for _ in range(1500)]
    tuples += [[rng.choice(rnd) for _ in range(6)] for _ in range(1500)]
    tuples += [[rng.choice(pats + rnd) for _ in range(6)] for _ in range(1000)]
    out = (ctypes.c_int32 * (NL * 2 * len(OPS)))()
    canon = (ctypes.c_int32 * NL)()
    for t in tuples:
        shim.t_scan_ops(pack(t), out)
        vals = [value(e) for e in t]
        for k, op in enumerate(OPS):
            col = list(out[NL * 2 * k:NL * (2 * k + 1)])
            scan = list(out[NL * (2 * k + 1):NL * (2 * k + 2)])
            assert scan == col, op
            assert all(0 <= l <= MASK for l in scan[:8])  # N-form
            assert value(scan) % P == expected(op, vals), op
            if abs(scan[8]) < 1 << 28:  # fe_canon's contract; products of the all-ones pattern reach 2^261
                shim.t_canon((ctypes.c_int32 * NL)(*scan), canon)
                assert value(list(canon)) == expected(op, vals), op


def test_group_law_gives_the_same_limbs_with_both_forms(shim):
    # coordinates in (-p, 2p) as the kernels hold them (limb 8 in [-2^19, 2^20]): the formulas' own bound notes
    # (curve.hpp, "B = k") assume outputs of a multiplication, not the 4p of the bare forms above
    rng = random.Random(2904)
    elems = [[rng.getrandbits(LB) for _ in range(8)] + [rng.randint(-(1 << 19), 1 << 20)] for _ in range(20000)]
    ones, zero = [MASK] * 8, [0] * 8
    elems += [rng.choice([ones + [1 << 20], zero + [-(1 << 19)], ones + [-(1 << 19)], zero + [0], ones + [0]])
              for _ in range(4000)]
    bad = shim.t_scan_compare_xyzz(pack(elems), len(elems))
    assert bad == -1, "item %d, formula %d" % (bad // 16, bad % 16)
