"""The per-item code of the batch point arithmetic (csrc/ec_points.hpp: k P, a G + b P, P +- Q with the verifier's
ladder of csrc/ladder.hpp under it) on the host, no GPU: g++ builds tests/host/ec_points_shim.cpp with the bound checks
on.  Inputs and expected answers: tests/ec_point_cases.py (Python integers).  Not covered here: the device's walk over
the EC_GEN window table, which the shim replaces by the host's affine double-and-add."""
import ctypes
import os
import subprocess

import pytest

import ec_point_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 2**256 - 2**128 - 12345


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "host", "ec_points_shim.cpp")
    so = os.path.join(HERE, "host", "ec_points_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.ep_mult.restype = lib.ep_lincomb.restype = lib.ep_add.restype = None
    lib.ep_mult.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t]
    lib.ep_lincomb.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t]
    lib.ep_add.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    return lib


def felts(values):
    return ctypes.create_string_buffer(b"".join(v.to_bytes(32, "little") for v in values), 32 * len(values))


def unpack(buf, n):
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]


def call(fn, inputs, n, subtract=None, want_y=True):
    """(status list, [(x, y) or what the sentinel-filled outputs still hold]) of one shim entry point."""
    rx, ry = felts([SENTINEL] * n), felts([SENTINEL] * n)
    status = (ctypes.c_uint8 * n)(*([0xEE] * n))
    args = [felts(col) for col in inputs]
    if subtract is not None:
        args.append(subtract)
    fn(*args, rx, ry if want_y else None, status, n)
    return list(status), list(zip(unpack(rx, n), unpack(ry, n)))


def check(cases, status, got):
    """status and value of every case; outputs of the items that are not OK untouched."""
    assert len(cases) == len(status)
    for case, st, xy in zip(cases, status, got):
        want_status, want = case[-2], case[-1]
        assert st == want_status, (case, st)
        assert xy == (want if st == C.OK else (SENTINEL, SENTINEL)), (case, xy)


def mult_columns(cases):
    return [[c[0] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases]]


def lincomb_columns(cases):
    return [[c[0] for c in cases], [c[1] for c in cases], [c[2][0] for c in cases], [c[2][1] for c in cases]]


def add_columns(cases):
    return [[c[0][0] for c in cases], [c[0][1] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases]]


def test_mult_case_set(shim):
    cases = C.mult_cases()
    assert {c[2] for c in cases} == {C.OK, C.INFINITY, C.OUT_OF_RANGE, C.NOT_ON_CURVE}
    assert len([c for c in cases if c[2] == C.OK]) <= 300
    status, got = call(shim.ep_mult, mult_columns(cases), len(cases))
    check(cases, status, got)


def test_mult_where_the_ladder_meets_its_own_operand(shim):
    """k = 30 and k = N - 30 on every known point: 16 m = N - 15 = -15 mod N before the last window, whose digit is
    -15 - the ladder's last addition is a doubling there; the neighbours 29, 31, N - 29, N - 31 take the plain path."""
    cases = []
    for t, pt in C.known_points():
        for k in (29, 30, 31, C.N - 29, C.N - 30, C.N - 31):
            cases.append((k, pt, C.OK, C.gmul(k * t)))
    status, got = call(shim.ep_mult, mult_columns(cases), len(cases))
    check(cases, status, got)


def test_mult_by_order_minus_one_is_the_negation(shim):
    pts = [pt for _, pt in C.known_points()]
    cases = [(C.N - 1, pt, C.OK, C.neg(pt)) for pt in pts]
    status, got = call(shim.ep_mult, mult_columns(cases), len(cases))
    check(cases, status, got)


def test_lincomb_case_set(shim):
    cases = C.lincomb_cases()
    assert {c[3] for c in cases} == {C.OK, C.INFINITY, C.OUT_OF_RANGE, C.NOT_ON_CURVE}
    assert sum(1 for c in cases if c[3] == C.INFINITY) >= 30
    status, got = call(shim.ep_lincomb, lincomb_columns(cases), len(cases))
    check(cases, status, got)


def test_add_case_set(shim):
    cases = C.add_cases()
    assert {c[3] for c in cases} == {C.OK, C.INFINITY, C.OUT_OF_RANGE, C.NOT_ON_CURVE}
    for sub in (0, 1):
        part = [c for c in cases if c[2] == sub]
        status, got = call(shim.ep_add, add_columns(part), len(part), subtract=sub)
        check(part, status, got)


def test_order_of_the_checks(shim):
    """Range of everything first, then the curve, then the arithmetic - and the point is checked when its scalar is 0."""
    off = (C.GEN[0], C.GEN[1] + 1)
    status, _ = call(shim.ep_mult, mult_columns([(C.N, off, 0, 0), (0, off, 0, 0), (0, (C.P, 0), 0, 0), (0, C.GEN, 0, 0)]), 4)
    assert status == [C.OUT_OF_RANGE, C.NOT_ON_CURVE, C.OUT_OF_RANGE, C.INFINITY]
    rows = [(0, C.N, off, 0, 0), (C.N, 0, off, 0, 0), (0, 0, off, 0, 0), (0, 0, (0, C.P), 0, 0), (0, 0, C.GEN, 0, 0)]
    status, _ = call(shim.ep_lincomb, lincomb_columns(rows), 5)
    assert status == [C.OUT_OF_RANGE, C.OUT_OF_RANGE, C.NOT_ON_CURVE, C.OUT_OF_RANGE, C.INFINITY]
    rows = [(off, (C.P, 1), 0, 0, 0), ((0, 2**256 - 1), off, 0, 0, 0), (off, C.GEN, 0, 0, 0), (C.GEN, off, 0, 0, 0)]
    status, _ = call(shim.ep_add, add_columns(rows), 4, subtract=0)
    assert status == [C.OUT_OF_RANGE, C.OUT_OF_RANGE, C.NOT_ON_CURVE, C.NOT_ON_CURVE]


def test_x_alone(shim):
    cases = C.mult_cases()[:40]
    status, got = call(shim.ep_mult, mult_columns(cases), len(cases), want_y=False)
    both, full = call(shim.ep_mult, mult_columns(cases), len(cases))
    assert status == both
    assert [xy[0] for xy in got] == [xy[0] for xy in full]
    assert all(xy[1] == SENTINEL for xy in got)
