"""The statement-binding Pedersen proof without a GPU.

First the mathematics of tests/hash_io_ref.py itself, before any kernel is involved: for k = 1 and k = 2 hashes the
composition of an honest trace WITH the three boundary quotients is a polynomial of degree < 3 n, and stops being one
when a single h_i, x_i or y_i of the public list is changed.

Then the per-lane logic of the two kernels (csrc/hash_io.hpp) built by g++ - tests/host/hash_io_shim.cpp replays the
launch plans over host arrays - against that reference in integers."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import hash_io_ref as H
import workloads as wl
from oracle import stark_ref as S

P = S.P
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "hash_io_shim.cpp")


def felts_np(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).copy()


def ints_of(arr):
    raw = np.ascontiguousarray(arr).astype("<u8").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]


@pytest.fixture(scope="module")
def honest():
    """k -> (inputs, trace LDE, periodic LDE, public inputs) of an honest trace, built once."""
    rng = random.Random(2024)
    out = {}
    for k in (1, 2):
        inputs = [(rng.randrange(P), rng.randrange(P)) for _ in range(k)]
        trace = S.pedersen_trace(inputs)
        out[k] = (inputs, [S.lde(c) for c in trace], S.periodic_lde(512 * k), H.public_inputs(inputs, H.hash_outputs(trace)))
    return out


# ---- the reference's own mathematics ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 2))
def test_trace_holds_the_statement_where_the_constraints_say(honest, k):
    inputs, _, _, pub = honest[k]
    trace = S.pedersen_trace(inputs)
    for i, (x, y) in enumerate(inputs):
        assert trace[0][512 * i] == x and trace[0][512 * i + 256] == y
        assert trace[1][512 * i + 511] == S.R.pedersen_hash(x, y) == pub[3 * i + 2]


@pytest.mark.parametrize("k", (1, 2))
def test_honest_composition_is_low_degree_and_a_changed_statement_is_not(honest, k):
    inputs, trace_lde, per, pub = honest[k]
    n = 512 * k
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in range(H.N_ALPHAS)]
    comp = H.composition_io_on_coset(trace_lde, per, H.public_columns_lde(pub, n), n, alphas)
    assert S.poly_degree_bound_check(comp, S.GEN, 3 * n - 1)
    # the boundary term alone is already a polynomial of degree < n
    assert S.poly_degree_bound_check(H.boundary_on_coset(trace_lde, H.public_columns_lde(pub, n), n, alphas[11:]), S.GEN, n - 1)
    for which in range(3):  # x, y, h of the last hash, off by one
        bad = list(pub)
        bad[3 * (k - 1) + which] = (bad[3 * (k - 1) + which] + 1) % P
        extra = H.boundary_on_coset(trace_lde, H.public_columns_lde(bad, n), n, alphas[11:])
        base = S.composition_on_coset(trace_lde, per, n, alphas[:11])
        assert not S.poly_degree_bound_check([(a + b) % P for a, b in zip(base, extra)], S.GEN, 3 * n - 1), which


def test_point_form_of_the_reference_equals_its_dense_form(honest):
    _, trace_lde, _, pub = honest[2]
    n, alphas = 1024, [5, 7, 11]
    dense = H.boundary_on_coset(trace_lde, H.public_columns_lde(pub, n), n, alphas)
    coeffs = H.public_coefficients(pub, n)
    for pos in (0, 1, 2047, 2048, 4095, 1234):
        assert H.boundary_at(n, coeffs, alphas, S.GEN, pos, [c[pos] for c in trace_lde]) == dense[pos]


# ---- the kernels' lane logic on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "hash_io_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.hs_dense.restype = lib.hs_points.restype = ctypes.c_int
    lib.hs_dense.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint] + [ctypes.c_void_p] * 5 + [
        ctypes.c_size_t]
    lib.hs_points.argtypes = [ctypes.c_uint] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [
        ctypes.c_size_t]
    return lib


def run_dense(shim, cols, pub_lde, log_n, alphas, shift, acc=None, alias=False, col_stride=None):
    trace = np.concatenate([felts_np(c) for c in cols])
    pub = np.concatenate([felts_np(c) for c in pub_lde])
    out = np.full((len(cols[0]), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)  # the columns' size, whatever log_n claims
    acc_np = None if acc is None else felts_np(acc)
    if alias:
        out = acc_np
    err = ctypes.create_string_buffer(128)
    rc = shim.hs_dense(trace.ctypes.data, len(cols[0]) if col_stride is None else col_stride, pub.ctypes.data, log_n,
                       felts_np(alphas).ctypes.data, felts_np([shift]).ctypes.data,
                       None if acc_np is None else acc_np.ctypes.data, out.ctypes.data, err, 128)
    return rc, ints_of(out), err.value.decode()


def run_points(shim, log_n, coeffs, alphas, shift, pos, cur):
    n = len(pos)
    out = np.full((max(n, 1), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(128)
    coef = np.concatenate([felts_np(c) for c in coeffs])
    pos_np = np.array(pos, dtype=np.uint64)
    cur_np = felts_np([v for row in cur for v in row]) if n else np.zeros((1, 4), dtype=np.uint64)
    rc = shim.hs_points(log_n, coef.ctypes.data, felts_np(alphas).ctypes.data, felts_np([shift]).ctypes.data, n,
                        pos_np.ctypes.data, cur_np.ctypes.data, out.ctypes.data, status.ctypes.data, err, 128)
    return rc, ints_of(out)[:n], status.tolist()[:n], err.value.decode()


def arbitrary_columns(count, size, seed):
    """Columns of 0, 1, p - 1, the extreme limb patterns (0.85) and random felts, as
    test_prover_kernels_on_extreme_limb_patterns mixes them."""
    rng = random.Random(seed)
    ext = wl.extreme_felts()
    return [[rng.choice(ext) if rng.random() < 0.85 else rng.randrange(P) for _ in range(size)] for _ in range(count)]


def test_host_dense_honest_trace_every_acc_mode_and_shift(shim, honest):
    _, trace_lde, _, pub = honest[1]
    rng = random.Random(3)
    alphas = [rng.randrange(P) for _ in range(3)]
    pub_lde = H.public_columns_lde(pub, 512)
    want = H.boundary_on_coset(trace_lde, pub_lde, 512, alphas)
    rc, got, err = run_dense(shim, trace_lde, pub_lde, 9, alphas, S.GEN)
    assert (rc, err) == (0, "") and got == want
    acc = arbitrary_columns(1, 2048, 8)[0]
    summed = [(a + b) % P for a, b in zip(acc, want)]
    assert run_dense(shim, trace_lde, pub_lde, 9, alphas, S.GEN, acc=acc)[1] == summed
    assert run_dense(shim, trace_lde, pub_lde, 9, alphas, S.GEN, acc=acc, alias=True)[1] == summed


@pytest.mark.parametrize("log_n,shift", ((9, S.GEN), (10, 0x123456789ABCDEF0123456789), (9, P - 2)))
def test_host_dense_arbitrary_columns(shim, log_n, shift):
    M = 4 << log_n
    cols = arbitrary_columns(2, M, log_n)
    pub_lde = arbitrary_columns(3, M, 100 + log_n)
    alphas = arbitrary_columns(1, 3, 200 + log_n)[0]
    rc, got, _ = run_dense(shim, cols, pub_lde, log_n, alphas, shift)
    assert rc == 0 and got == H.boundary_on_coset(cols, pub_lde, 1 << log_n, alphas, shift)


@pytest.mark.parametrize("k", (1, 2))
def test_host_points_equal_the_dense_column(shim, honest, k):
    _, trace_lde, _, pub = honest[k]
    n = 512 * k
    alphas = [3, P - 1, 1 << 250]
    dense = H.boundary_on_coset(trace_lde, H.public_columns_lde(pub, n), n, alphas)
    pos = list(range(0, 4 * n, 7)) + [4 * n - 1]
    rc, got, status, _ = run_points(shim, n.bit_length() - 1, H.public_coefficients(pub, n), alphas, S.GEN, pos,
                                    [[c[p] for c in trace_lde] for p in pos])
    assert rc == 0 and status == [0] * len(pos) and got == [dense[p] for p in pos]


@pytest.mark.parametrize("k", (1, 2, 64, 128, 256, 512, 2048, 1 << 15))
def test_host_points_coefficients_alone(shim, k):
    """Below, at and above one block's stride of 256, against Horner in integers; extreme coefficients."""
    n = 512 * k
    coeffs = arbitrary_columns(3, k, k)
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in range(3)]
    pos = [0, 1, 4 * n - 1, 2 * n] + [rng.randrange(4 * n) for _ in range(4)]
    cur = [[rng.randrange(P) for _ in range(4)] for _ in pos]
    rc, got, status, _ = run_points(shim, n.bit_length() - 1, coeffs, alphas, 5, pos, cur)
    assert rc == 0 and status == [0] * 8
    assert got == [H.boundary_at(n, coeffs, alphas, 5, p, c) for p, c in zip(pos, cur)]


def test_host_points_status_and_neighbours(shim):
    n, k = 1024, 2
    coeffs = arbitrary_columns(3, k, 1)
    alphas = [2, 3, 4]
    pos = [5, 4 * n, 6, (1 << 64) - 1, 7, 8, 9]
    cur = [[1, 2, 3, 4] for _ in pos]
    cur[5] = [1, 2, 3, P]           # a felt of the row that the value does not even use
    cur[6] = [(1 << 256) - 1, 2, 3, 4]
    rc, got, status, _ = run_points(shim, 10, coeffs, alphas, S.GEN, pos, cur)
    assert rc == 0 and status == [0, 1, 0, 1, 0, 1, 1]
    for i in (0, 2, 4):
        assert got[i] == H.boundary_at(n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [got[i] for i in (1, 3, 5, 6)] == [0] * 4


def test_host_argument_rules(shim, honest):
    _, trace_lde, _, pub = honest[1]
    pub_lde = H.public_columns_lde(pub, 512)
    for log_n, shift, stride, word in ((8, 3, None, "log_n"), (25, 3, None, "log_n"), (9, 0, None, "shift"),
                                       (9, 1, None, "shift"), (9, S.root_of_unity(11), None, "shift"),
                                       (9, P, None, "shift"), (9, 3, 2047, "col_stride")):
        rc, got, err = run_dense(shim, trace_lde, pub_lde, log_n, [1, 2, 3], shift, col_stride=stride)
        assert rc == -3 and word in err and set(got) == {int("aa" * 32, 16)}, (log_n, shift)
    coeffs = H.public_coefficients(pub, 512)
    for log_n, shift, word in ((8, 3, "log_n"), (31, 3, "log_n"), (9, 0, "shift"), (9, P - 1, "shift")):
        rc, got, status, err = run_points(shim, log_n, coeffs, [1, 2, 3], shift, [0], [[1, 2, 3, 4]])
        assert rc == -3 and word in err and status == [0xEE] and got == [int("aa" * 32, 16)]
    assert run_points(shim, 9, coeffs, [1, 2, 3], 3, [], [])[0] == 0
