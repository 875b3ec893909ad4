"""Boundary constraints from a descriptor without a GPU.

First the mathematics of tests/boundary_ref.py itself, before any kernel is involved: for k = 1, 2 signatures and
k = 1, 2, 4 range-checked values the boundary term of an honest trace is a polynomial of degree < n, and stops being
one when a single z, r, s, Q or value of the public list is changed; with the pedersen_io descriptor it is the term
of tests/hash_io_ref.py.

Then the per-lane logic of the two kernels (csrc/boundary.hpp) built by g++ - tests/host/boundary_shim.cpp replays
the launch plans over host arrays - against that reference in integers, the argument rules, and the stand-alone form
of the shim under -fsanitize=address,undefined, run directly."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import boundary_ref as B
import hash_io_ref as H
import workloads as wl
from oracle import ref_py as R
from oracle import stark_ref as S

P = S.P
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "boundary_shim.cpp")
FILL = int("aa" * 32, 16)
ECDSA, RANGE, HASHES = (B.DESCRIPTORS[k] for k in ("ecdsa_io", "range_check_io", "pedersen_io"))
# the widest descriptor the calls take, terms out of group order: no AIR of the project, only the argument rules' limit
WIDEST = {"period": 256, "n_cols": 16, "rows": (255, 0, 7, 128),
          "terms": ((15, 3), (0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 2), (6, 0))}
OTHER_SHIFT = 0x123456789ABCDEF0123456789


def felts_np(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).copy()


def ints_of(arr):
    raw = np.ascontiguousarray(arr).astype("<u8").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]


def signatures(k, seed):
    """k signatures the reference accepts, as public inputs [z, r, s, Qx, Qy, ...] and as AIR instances."""
    rng = random.Random(seed)
    pub, insts = [], []
    for _ in range(k):
        z, d = rng.randrange(1, 2**251), rng.randrange(1, R.EC_ORDER)
        r, s = R.sign(z, d)
        q = R.private_key_to_ec_point_on_stark_curve(d)
        insts.append(S.ecdsa_instance(z, r, s, q))
        pub += [z, r, s, q[0], q[1]]
    return pub, insts


@pytest.fixture(scope="module")
def honest():
    """(name, k) -> (trace LDE, public inputs) of an honest trace, built once."""
    out = {}
    for k in (1, 2):
        pub, insts = signatures(k, 70 + k)
        out["ecdsa_io", k] = ([S.lde(c) for c in S.ecdsa_trace(insts)], pub)
    rng = random.Random(5)
    for k in (1, 2, 4):
        pub = [rng.randrange(1 << 128) for _ in range(k)]
        out["range_check_io", k] = ([S.lde(c) for c in S.range_check_trace(pub)], pub)
    return out


def dense_ref(name, trace_lde, pub, n, alphas, shift=S.GEN):
    desc = B.DESCRIPTORS[name]
    return B.boundary_on_coset(desc, trace_lde, B.public_columns_lde(desc, B.term_values(name, pub), n, alphas, shift), n,
                               alphas, shift)


# ---- the reference's own mathematics ------------------------------------------------------------------------------------
CASES = [("ecdsa_io", 1), ("ecdsa_io", 2), ("range_check_io", 1), ("range_check_io", 2), ("range_check_io", 4)]


@pytest.mark.parametrize("name,k", CASES)
def test_trace_holds_the_statement_where_the_descriptor_says(name, k):
    desc = B.DESCRIPTORS[name]
    if name == "ecdsa_io":
        pub, insts = signatures(k, 70 + k)
        trace = S.ecdsa_trace(insts)
    else:
        pub = [random.Random(k).randrange(1 << 128) for _ in range(k)]
        trace = S.range_check_trace(pub)
    for (c, d), v in zip(desc["terms"], B.term_values(name, pub)):
        assert trace[c][desc["rows"][d]::desc["period"]] == v, (c, d)


@pytest.mark.parametrize("name,k", CASES)
def test_honest_boundary_is_low_degree_and_a_changed_statement_is_not(honest, name, k):
    trace_lde, pub = honest[name, k]
    n = B.DESCRIPTORS[name]["period"] * k
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in B.DESCRIPTORS[name]["terms"]]
    assert S.poly_degree_bound_check(dense_ref(name, trace_lde, pub, n, alphas), S.GEN, n - 1)
    if name == "ecdsa_io":
        other = R.private_key_to_ec_point_on_stark_curve(12345)
        lies = [(0, pub[0] + 1), (1, pub[1] + 1), (2, pub[2] + 1), (3, other[0]), (4, other[1])]  # z, r, s, Qx, Qy
    else:
        lies = [(0, (pub[0] + 1) % (1 << 128))]
    for which, value in lies:  # in the last instance
        bad = list(pub)
        bad[len(pub) // k * (k - 1) + which] = value
        assert not S.poly_degree_bound_check(dense_ref(name, trace_lde, bad, n, alphas), S.GEN, n - 1), which


def test_honest_composition_with_the_boundary_term_is_low_degree(honest):
    trace_lde, pub = honest["range_check_io", 2]
    n = 256
    rng = random.Random(9)
    alphas = [rng.randrange(P) for _ in range(B.n_alphas("range_check_io"))]
    comp = B.composition_bound_on_coset("range_check_io", trace_lde, S.periodic_lde(n, S.GEN, "range_check"),
                                        B.term_values("range_check_io", pub), n, alphas)
    assert S.poly_degree_bound_check(comp, S.GEN, 3 * n - 1)


@pytest.mark.parametrize("name,k", (("ecdsa_io", 2), ("range_check_io", 4)))
def test_point_form_of_the_reference_equals_its_dense_form(honest, name, k):
    trace_lde, pub = honest[name, k]
    desc = B.DESCRIPTORS[name]
    n = desc["period"] * k
    alphas = [5, 7, 11, 13, 17][:len(desc["terms"])]
    dense = dense_ref(name, trace_lde, pub, n, alphas)
    coeffs = B.public_coefficients(desc, B.term_values(name, pub), n, alphas)
    for pos in (0, 1, 4 * desc["period"] - 1, 4 * desc["period"], 4 * n - 1, 1234 % (4 * n)):
        assert B.boundary_at(desc, n, coeffs, alphas, S.GEN, pos, [c[pos] for c in trace_lde]) == dense[pos]


def test_the_pedersen_descriptor_is_the_hash_io_statement():
    """Arbitrary columns: B of the pedersen_io descriptor with C_d = a_d X_d is the B of tests/hash_io_ref.py."""
    n, rng = 512, random.Random(4)
    cols = [[rng.randrange(P) for _ in range(4 * n)] for _ in range(4)]
    pub, alphas = [rng.randrange(P) for _ in range(3)], [rng.randrange(P) for _ in range(3)]
    want = H.boundary_on_coset(cols, H.public_columns_lde(pub, n), n, alphas)
    assert dense_ref("pedersen_io", cols, pub, n, alphas) == want
    coeffs = B.public_coefficients(HASHES, B.term_values("pedersen_io", pub), n, alphas)
    assert B.boundary_at(HASHES, n, coeffs, alphas, S.GEN, 77, [c[77] for c in cols]) == want[77]


# ---- the kernels' lane logic on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "boundary_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.bs_dense.restype = lib.bs_points.restype = ctypes.c_int
    desc = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    lib.bs_dense.argtypes = desc + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint] + [
        ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    lib.bs_points.argtypes = desc + [ctypes.c_uint] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [
        ctypes.c_size_t]
    return lib


def desc_args(desc, **over):
    """The seven descriptor arguments; `over` replaces fields (for the argument rules).  The arrays are kept alive by
    the returned list."""
    d = dict(log_period=desc["period"].bit_length() - 1, n_cols=desc["n_cols"], n_groups=len(desc["rows"]),
             group_rows=list(desc["rows"]), n_terms=len(desc["terms"]), term_cols=[c for c, _ in desc["terms"]],
             term_groups=[g for _, g in desc["terms"]])
    d.update(over)
    arr = lambda v: None if v is None else (ctypes.c_uint * max(len(v), 1))(*v)
    return [d["log_period"], d["n_cols"], d["n_groups"], arr(d["group_rows"]), d["n_terms"], arr(d["term_cols"]), arr(d["term_groups"])]


def run_dense(shim, desc, cols, pub_lde, log_n, alphas, shift, acc=None, alias=False, col_stride=None, **over):
    trace = np.concatenate([felts_np(c) for c in cols])
    pub = np.concatenate([felts_np(c) for c in pub_lde])
    out = np.full((len(cols[0]), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)  # the columns' size, whatever log_n claims
    acc_np = None if acc is None else felts_np(acc)
    if alias:
        out = acc_np
    err = ctypes.create_string_buffer(128)
    alphas_np, shift_np = felts_np(alphas), felts_np([shift])  # named: an array must outlive the call that reads it
    rc = shim.bs_dense(*desc_args(desc, **over), trace.ctypes.data, len(cols[0]) if col_stride is None else col_stride,
                       pub.ctypes.data, log_n, alphas_np.ctypes.data, shift_np.ctypes.data,
                       None if acc_np is None else acc_np.ctypes.data, out.ctypes.data, err, 128)
    return rc, ints_of(out), err.value.decode()


def run_points(shim, desc, log_n, coeffs, alphas, shift, pos, cur, **over):
    n = len(pos)
    out = np.full((max(n, 1), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(128)
    coef = np.concatenate([felts_np(c) for c in coeffs])
    pos_np = np.array(pos, dtype=np.uint64)
    cur_np = felts_np([v for row in cur for v in row]) if n else np.zeros((1, 4), dtype=np.uint64)
    alphas_np, shift_np = felts_np(alphas), felts_np([shift])
    rc = shim.bs_points(*desc_args(desc, **over), log_n, coef.ctypes.data, alphas_np.ctypes.data,
                        shift_np.ctypes.data, n, pos_np.ctypes.data, cur_np.ctypes.data, out.ctypes.data,
                        status.ctypes.data, err, 128)
    return rc, ints_of(out)[:n], status.tolist()[:n], err.value.decode()


def arbitrary_columns(count, size, seed):
    """Columns of 0, 1, p - 1, the extreme limb patterns (0.85) and random felts, as
    test_prover_kernels_on_extreme_limb_patterns mixes them."""
    rng = random.Random(seed)
    ext = wl.extreme_felts()
    return [[rng.choice(ext) if rng.random() < 0.85 else rng.randrange(P) for _ in range(size)] for _ in range(count)]


@pytest.mark.parametrize("name,k", (("ecdsa_io", 1), ("range_check_io", 1), ("range_check_io", 4)))
def test_host_dense_honest_trace_every_acc_mode(shim, honest, name, k):
    trace_lde, pub = honest[name, k]
    desc = B.DESCRIPTORS[name]
    n = desc["period"] * k
    rng = random.Random(3)
    alphas = [rng.randrange(P) for _ in desc["terms"]]
    pub_lde = B.public_columns_lde(desc, B.term_values(name, pub), n, alphas)
    want = B.boundary_on_coset(desc, trace_lde, pub_lde, n, alphas)
    log_n = n.bit_length() - 1
    rc, got, err = run_dense(shim, desc, trace_lde, pub_lde, log_n, alphas, S.GEN)
    assert (rc, err) == (0, "") and got == want
    acc = arbitrary_columns(1, 4 * n, 8)[0]
    summed = [(a + b) % P for a, b in zip(acc, want)]
    assert run_dense(shim, desc, trace_lde, pub_lde, log_n, alphas, S.GEN, acc=acc)[1] == summed
    assert run_dense(shim, desc, trace_lde, pub_lde, log_n, alphas, S.GEN, acc=acc, alias=True)[1] == summed


@pytest.mark.parametrize("desc,log_n,shift", ((ECDSA, 10, S.GEN), (ECDSA, 10, OTHER_SHIFT), (RANGE, 7, S.GEN),
                                              (RANGE, 9, OTHER_SHIFT), (RANGE, 8, P - 2), (HASHES, 9, OTHER_SHIFT),
                                              (WIDEST, 8, S.GEN), (WIDEST, 9, OTHER_SHIFT)),
                         ids=lambda v: None if isinstance(v, dict) else "%x" % v)
def test_host_dense_arbitrary_columns(shim, desc, log_n, shift):
    """Extreme limb patterns in the trace columns, the public columns, acc and the challenges; two shifts."""
    M = 4 << log_n
    cols = arbitrary_columns(desc["n_cols"], M, log_n)
    pub_lde = arbitrary_columns(len(desc["rows"]), M, 100 + log_n)
    alphas = arbitrary_columns(1, len(desc["terms"]), 200 + log_n)[0]
    acc = arbitrary_columns(1, M, 300 + log_n)[0]
    want = B.boundary_on_coset(desc, cols, pub_lde, 1 << log_n, alphas, shift)
    rc, got, _ = run_dense(shim, desc, cols, pub_lde, log_n, alphas, shift)
    assert rc == 0 and got == want
    assert run_dense(shim, desc, cols, pub_lde, log_n, alphas, shift, acc=acc)[1] == [(a + b) % P for a, b in zip(acc, want)]


@pytest.mark.parametrize("name,k", (("ecdsa_io", 1), ("ecdsa_io", 2), ("range_check_io", 2)))
def test_host_points_equal_the_dense_column(shim, honest, name, k):
    trace_lde, pub = honest[name, k]
    desc = B.DESCRIPTORS[name]
    n = desc["period"] * k
    alphas = [3, P - 1, 1 << 250, 12345, P - 2][:len(desc["terms"])]
    dense = dense_ref(name, trace_lde, pub, n, alphas)
    pos = list(range(0, 4 * n, 7)) + [4 * n - 1]
    coeffs = B.public_coefficients(desc, B.term_values(name, pub), n, alphas)
    rc, got, status, _ = run_points(shim, desc, n.bit_length() - 1, coeffs, alphas, S.GEN, pos,
                                    [[c[p] for c in trace_lde] for p in pos])
    assert rc == 0 and status == [0] * len(pos) and got == [dense[p] for p in pos]


@pytest.mark.parametrize("desc", (ECDSA, RANGE, WIDEST), ids=("ecdsa", "range", "widest"))
@pytest.mark.parametrize("k", (1, 2, 128, 256, 512, 4096))
def test_host_points_coefficients_alone(shim, desc, k):
    """Below, at and above one block's stride of 256, against Horner in integers; extreme coefficients and rows."""
    n = desc["period"] * k
    coeffs = arbitrary_columns(len(desc["rows"]), k, k)
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in desc["terms"]]
    pos = [0, 1, 4 * n - 1, 2 * n] + [rng.randrange(4 * n) for _ in range(4)]
    cur = arbitrary_columns(8, desc["n_cols"], 7 * k)
    rc, got, status, _ = run_points(shim, desc, n.bit_length() - 1, coeffs, alphas, 5, pos, cur)
    assert rc == 0 and status == [0] * 8
    assert got == [B.boundary_at(desc, n, coeffs, alphas, 5, p, c) for p, c in zip(pos, cur)]


def test_host_points_status_and_neighbours(shim):
    n, k = 2048, 2
    coeffs = arbitrary_columns(3, k, 1)
    alphas = [2, 3, 4, 5, 6]
    pos = [5, 4 * n, 6, (1 << 64) - 1, 7, 8, 9]
    cur = [list(range(1, 11)) for _ in pos]
    cur[5][9] = P               # a felt of the row that the value does not even use
    cur[6][0] = (1 << 256) - 1
    rc, got, status, _ = run_points(shim, ECDSA, 11, coeffs, alphas, S.GEN, pos, cur)
    assert rc == 0 and status == [0, 1, 0, 1, 0, 1, 1]
    for i in (0, 2, 4):
        assert got[i] == B.boundary_at(ECDSA, n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [got[i] for i in (1, 3, 5, 6)] == [0] * 4


DESCRIPTOR_RULES = (({"log_period": 6}, "log_period"), ({"log_period": 11}, "log_period"), ({"n_cols": 0}, "n_cols"),
                    ({"n_cols": 17}, "n_cols"), ({"n_groups": 0}, "n_groups"), ({"n_groups": 5}, "n_groups"),
                    ({"n_terms": 0}, "n_terms"), ({"n_terms": 9}, "n_terms"), ({"group_rows": None}, "group_rows"),
                    ({"term_cols": None}, "term_cols"), ({"term_groups": None}, "term_groups"),
                    ({"group_rows": [0, 256, 1024]}, "group_rows"), ({"group_rows": [0, 256, 256]}, "group_rows"),
                    ({"term_cols": [0, 0, 3, 10, 0]}, "term_cols"), ({"term_groups": [0, 1, 1, 1, 3]}, "term_groups"),
                    ({"term_groups": [0, 1, 1, 1, 1]}, "without a term"))


def test_host_argument_rules(shim, honest):
    trace_lde, pub = honest["ecdsa_io", 1]
    alphas = [1, 2, 3, 4, 5]
    pub_lde = B.public_columns_lde(ECDSA, B.term_values("ecdsa_io", pub), 1024, alphas)
    coeffs = B.public_coefficients(ECDSA, B.term_values("ecdsa_io", pub), 1024, alphas)
    row = [list(range(1, 11))]
    for over, word in DESCRIPTOR_RULES:
        rc, got, err = run_dense(shim, ECDSA, trace_lde, pub_lde, 10, alphas, 3, **over)
        assert rc == -3 and word in err and set(got) == {FILL}, over
        rc, got, status, err = run_points(shim, ECDSA, 10, coeffs, alphas, 3, [0], row, **over)
        assert rc == -3 and word in err and status == [0xEE] and got == [FILL], over
    for log_n, shift, stride, word in ((9, 3, None, "log_n"), (25, 3, None, "log_n"), (10, 0, None, "shift"),
                                       (10, 1, None, "shift"), (10, S.root_of_unity(12), None, "shift"),
                                       (10, P, None, "shift"), (10, 3, 4095, "col_stride")):
        rc, got, err = run_dense(shim, ECDSA, trace_lde, pub_lde, log_n, alphas, shift, col_stride=stride)
        assert rc == -3 and word in err and set(got) == {FILL}, (log_n, shift)
    for log_n, shift, word in ((9, 3, "log_n"), (31, 3, "log_n"), (10, 0, "shift"), (10, P - 1, "shift")):
        rc, got, status, err = run_points(shim, ECDSA, log_n, coeffs, alphas, shift, [0], row)
        assert rc == -3 and word in err and status == [0xEE] and got == [FILL]
    assert run_points(shim, ECDSA, 10, coeffs, alphas, 3, [], [])[0] == 0
    # the range-check descriptor's lower bound is its own period
    assert run_points(shim, RANGE, 6, [[1]], [1], 3, [0], [[1]])[0] == -3
    assert run_points(shim, RANGE, 7, [[1]], [1], 3, [0], [[1]])[0] == 0


def test_shim_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "boundary_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DBOUNDARY_SHIM_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "boundary check passed" in run.stdout, run.stdout + run.stderr


# ---- the binding, the header and the answers decided on the host ---------------------------------------------------
def test_header_and_binding_name_the_calls():
    from starkperp import _lib, stark
    header = open(os.path.join(HERE, "..", "include", "starkperp.h")).read()
    for name in ("sp_boundary_dev", "sp_boundary_points_dev"):
        assert "int %s(" % name in header and name in _lib.declared_symbols()
    for name in ("boundary_public_lde", "boundary", "boundary_coefficients", "boundary_points", "prove_signatures",
                 "verify_signatures", "prove_ranges", "verify_ranges"):
        assert callable(getattr(stark, name))
    for name in ("ecdsa_io", "range_check_io", "pedersen_io"):
        got, want = stark.BOUNDARY_DESCRIPTORS[name], B.DESCRIPTORS[name]
        assert (got["air"], tuple(got["rows"]), tuple(got["terms"])) == (want["air"], want["rows"], want["terms"])
        assert stark.AIRS[got["air"]]["period"] == want["period"] and stark.AIRS[got["air"]]["n_cols"] == want["n_cols"]


def test_verifiers_answer_malformed_before_the_library_is_needed():
    from starkperp import stark
    for verify in (stark.verify_signatures, stark.verify_ranges):
        for case in (None, 7, [], {}, {"air": "ecdsa"}, {"air": "ecdsa_io"}, {"air": "range_check_io"},
                     {"air": "pedersen_io"}):
            assert verify(case) == (False, "malformed")
    assert stark.verify({"air": "ecdsa_io"}) == (False, "malformed")
    assert stark.verify({"air": "range_check_io"}) == (False, "malformed")
