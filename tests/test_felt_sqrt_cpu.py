"""The fixed-length square root of csrc/fp29.hpp (fe_sqrt) and the per-item code of the x-only-key batches
(csrc/stark_keys.hpp) on the host, no GPU: g++ builds tests/host/felt_sqrt_shim.cpp with the bound checks on and a
counter in fe_mul / fe_sqr.  Inputs and expected answers: tests/stark_key_cases.py."""
import ctypes
import os
import subprocess

import pytest

import stark_key_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "host", "felt_sqrt_shim.cpp")
    so = os.path.join(HERE, "host", "felt_sqrt_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.fs_build.restype = ctypes.c_int
    lib.fs_table_bytes.restype = ctypes.c_size_t
    lib.fs_hash_mult.restype = ctypes.c_uint32
    for name in ("fs_sqrt", "fs_key_y"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t]
    for name in ("fs_is_residue", "fs_key_valid"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t]
    assert lib.fs_build() == 1, "the tables could not be built"
    return lib


SENTINEL = 2**256 - 2**128 - 12345


def run(shim, fn, values):
    """(status list, root list with None where nothing was written, operation counts) of one shim entry point."""
    n = len(values)
    src = ctypes.create_string_buffer(b"".join(v.to_bytes(32, "little") for v in values), 32 * n)
    status = (ctypes.c_uint8 * n)()
    ops = (ctypes.c_long * n)()
    if fn in ("fs_sqrt", "fs_key_y"):
        out = ctypes.create_string_buffer(SENTINEL.to_bytes(32, "little") * n, 32 * n)
        getattr(shim, fn)(src, out, status, ops, n)
        got = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]
        roots = [None if g == SENTINEL else g for g in got]
    else:
        getattr(shim, fn)(src, status, ops, n)
        roots = [None] * n
    return list(status), roots, list(ops)


def check_cases(shim, cases, counts):
    """cases = [(a, status, root or None)] through fs_sqrt; the operation counts of the non-zero ones go to `counts`."""
    status, roots, ops = run(shim, "fs_sqrt", [c[0] for c in cases])
    for (a, want_status, want_root), st, root, k in zip(cases, status, roots, ops):
        assert st == want_status and root == want_root, (hex(a), st, root)
        if a:
            counts.add(k)


@pytest.fixture(scope="module")
def root_ops(shim):
    """The operation count of one root (input 1), which every other non-zero input has to match."""
    (_, _, (k,)) = run(shim, "fs_sqrt", [1])
    return k


def test_tables(shim):
    assert shim.fs_table_bytes() < 500_000
    assert shim.fs_hash_mult() & 1


def test_basic_inputs(shim, root_ops):
    counts = set()
    check_cases(shim, K.basic_cases(), counts)
    assert counts == {root_ops}


def test_every_digit_of_every_window(shim, root_ops):
    cases = K.digit_sweep()
    assert len(cases) == K.DIGITS << K.W == 6144
    assert sum(1 for c in cases if c[1] == K.NON_RESIDUE) == 128
    counts = set()
    check_cases(shim, cases, counts)
    assert counts == {root_ops}


def test_all_digits_maximal(shim, root_ops):
    counts = set()
    check_cases(shim, [K.all_digits_maximal()], counts)
    assert counts == {root_ops}


def test_random_squares_and_their_negations(shim, root_ops):
    from oracle import ref_py as R
    values = K.random_squares()
    status, roots, ops = run(shim, "fs_sqrt", values)
    for a, st, root in zip(values, status, roots):
        K.check_root(a, st, root)
    assert set(ops) == {root_ops}
    for a, root in list(zip(values, roots))[::8]:  # 64 of the 512
        assert root == R.sqrt_mod(a, K.P)


def test_non_residues_and_out_of_range(shim, root_ops):
    values = K.mixed_felts(192)
    status, roots, ops = run(shim, "fs_sqrt", values)
    assert {K.OK, K.NON_RESIDUE, K.OUT_OF_RANGE} == set(status)
    for a, st, root in zip(values, status, roots):
        K.check_root(a, st, root)
        assert (root is None) == (st != K.OK)
    assert {k for a, k in zip(values, ops) if a < K.P} == {root_ops}
    # the status-only entry point (no tables, no root) agrees
    only, _, _ = run(shim, "fs_is_residue", values + [0])
    assert only == status + [K.OK]


def test_keys(shim):
    keys = K.golden_keys()
    assert len(keys) == 256
    xs = [x for x, _ in keys] + [K.off_curve_key()]
    status, ys, ops = run(shim, "fs_key_y", xs)
    assert status == [K.OK] * 256 + [K.NON_RESIDUE]
    assert ys == [y for _, y in keys] + [None]
    assert len(set(ops)) == 1 and ops[0] <= K.MAX_OPS
    valid, _, _ = run(shim, "fs_key_valid", xs)
    assert valid == status


def test_operation_count(shim, root_ops):
    """The same for a residue, a non-residue, the sparse and the dense exponents - and a fifth of the bit-by-bit
    method's at most.  2 338 in fe_sqrt (csrc/fp29.hpp) + 1 for the conversion of the input."""
    values = [1, 4, K.P - 1, 3, K.G, K.all_digits_maximal()[0], K.power_case(2**100)[0], K.power_case(2**100 + 1)[0]]
    _, _, ops = run(shim, "fs_sqrt", values)
    print("field operations per root:", ops)
    assert set(ops) == {root_ops}
    assert root_ops == 2339
    assert root_ops <= K.MAX_OPS
