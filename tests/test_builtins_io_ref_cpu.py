"""The builtins proof's boundary constraints without a GPU.

First the mathematics of tests/builtins_io_ref.py itself, before any kernel is involved: for all 7 segment sets, each
at its smallest size and one size larger, the combined trace holds the statement where the descriptors say, the
boundary term of an honest trace is a polynomial of degree < n, it stops being one when a single hash x, y or h, a
signature's z, r, s or Q changes or two range-checked values swap places, and the point form equals the dense form.

Then the per-lane logic of the kernels (csrc/builtins_boundary.hpp) built by g++ -
tests/host/builtins_boundary_shim.cpp replays both launch plans and the combine call over host arrays - against that
reference in integers, every argument rule, and the stand-alone form of the shim under -fsanitize=address,undefined,
run directly."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import boundary_ref as B
import builtins_io_cases as C
import builtins_io_ref as IO
from oracle import stark_ref as S

P = S.P
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "builtins_boundary_shim.cpp")
FILL = int("aa" * 32, 16)
ALL = ("pedersen", "ecdsa", "rc16")


def seeded_alphas(segments, seed):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(IO.n_boundary_alphas(segments))]


def segment_part(seg, segments, trace_lde, pub, n, alphas, shift=S.GEN):
    """B of one segment alone, on the columns and alphas it has inside the set."""
    (_, desc, c0, a0), = [e for e in IO.layout(segments) if e[0] == seg]
    al = alphas[a0: a0 + len(desc["terms"])]
    return B.boundary_on_coset(desc, trace_lde[c0: c0 + desc["n_cols"]],
                               B.public_columns_lde(desc, IO.term_values(seg, pub, n), n, al, shift), n, al, shift)


# ---- the reference's own mathematics ------------------------------------------------------------------------------------
def test_the_descriptors_are_the_single_air_descriptors_and_rc16_is_new():
    assert IO.SEG_DESC["pedersen"] is B.DESCRIPTORS["pedersen_io"] and IO.SEG_DESC["ecdsa"] is B.DESCRIPTORS["ecdsa_io"]
    assert IO.RC16_IO == {"air": "rc16", "period": 8, "n_cols": 3, "rows": (7,), "terms": ((1, 0),)}
    assert [IO.n_boundary_alphas(s) for s in C.SEGMENT_SETS] == [3, 5, 8, 1, 4, 6, 9]
    assert [C.n_groups(s) for s in C.SEGMENT_SETS] == [3, 3, 6, 1, 4, 4, 7]


@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_trace_holds_the_statement_where_the_descriptors_say(segments, log_n):
    cols, pub, _ = C.honest(segments, log_n)
    n = 1 << log_n
    for seg, desc, c0, _ in IO.layout(segments):
        for (c, d), v in zip(desc["terms"], IO.term_values(seg, pub, n)):
            assert cols[c0 + c][desc["rows"][d]::desc["period"]] == v, (seg, c, d)


@pytest.mark.parametrize("n", (16, 64, 256))
def test_rc16_descriptor_honest_low_degree_swapped_not_point_equals_dense(n):
    """The rc16_io descriptor on its own through tests/boundary_ref.py, as the issue checked it."""
    rng = random.Random(n)
    values = C.rc_values_for(n, rng)
    padded = S.rc16_fill(values, n // 8)[0]
    lde = [S.lde(c) for c in S.rc16_trace(padded)]
    alphas = [rng.randrange(P)]
    dense = B.boundary_on_coset(IO.RC16_IO, lde, B.public_columns_lde(IO.RC16_IO, [padded], n, alphas), n, alphas)
    assert S.poly_degree_bound_check(dense, S.GEN, n - 1)
    i = next(i for i in range(1, len(padded)) if padded[i] != padded[0])
    swapped = list(padded)
    swapped[0], swapped[i] = swapped[i], swapped[0]
    bad = B.boundary_on_coset(IO.RC16_IO, lde, B.public_columns_lde(IO.RC16_IO, [swapped], n, alphas), n, alphas)
    assert not S.poly_degree_bound_check(bad, S.GEN, n - 1)
    coeffs = B.public_coefficients(IO.RC16_IO, [padded], n, alphas)
    for pos in C.positions(4 * n):
        assert B.boundary_at(IO.RC16_IO, n, coeffs, alphas, S.GEN, pos, [c[pos] for c in lde]) == dense[pos]


@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_honest_boundary_is_low_degree_and_a_changed_claim_is_not(segments, log_n):
    _, pub, trace_lde = C.honest(segments, log_n)
    n = 1 << log_n
    alphas = seeded_alphas(segments, log_n)
    parts = {s: segment_part(s, segments, trace_lde, pub, n, alphas) for s in segments}
    total = [sum(v) % P for v in zip(*parts.values())]
    assert total == IO.boundary_on_coset(segments, trace_lde, C.values_of(segments, pub, n), n, alphas)
    assert S.poly_degree_bound_check(total, S.GEN, n - 1)
    claims = C.lies(segments, pub)
    assert len(claims) == sum({"pedersen": 3, "ecdsa": 4, "rc16": 1}[s] for s in segments)
    for what, seg, bad in claims:  # B is a sum over segments: only the lying segment's part changes
        lying = segment_part(seg, segments, trace_lde, bad, n, alphas)
        changed = [(t - a + b) % P for t, a, b in zip(total, parts[seg], lying)]
        assert not S.poly_degree_bound_check(changed, S.GEN, n - 1), what


@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_point_form_of_the_reference_equals_its_dense_form(segments, log_n):
    _, pub, trace_lde = C.honest(segments, log_n)
    n = 1 << log_n
    alphas = seeded_alphas(segments, 7 * log_n)
    values = C.values_of(segments, pub, n)
    dense = IO.boundary_on_coset(segments, trace_lde, values, n, alphas)
    coeffs = IO.coefficients(segments, values, n, alphas)
    for pos in C.positions(4 * n):
        assert IO.boundary_at(segments, n, coeffs, alphas, S.GEN, pos, [c[pos] for c in trace_lde]) == dense[pos], pos


def test_honest_composition_with_the_boundary_term_is_low_degree():
    """rc16 alone at n = 16: the AIR's composition with both phases plus B."""
    segments, n = ("rc16",), 16
    cols, pub, trace_lde = C.honest(segments, 4)
    rng = random.Random(2)
    z = rng.randrange(P)
    alphas = [rng.randrange(P) for _ in range(8 + 1)]
    p_lde = S.lde(S.rc16_product_column(cols[0], cols[2], z))
    comp = IO.composition_bound_on_coset(segments, trace_lde, p_lde, C.values_of(segments, pub, n), n, alphas, z,
                                         pub["rc_min"], pub["rc_max"])
    assert S.poly_degree_bound_check(comp, S.GEN, 3 * n - 1)


def test_flat_public_order():
    pub = {"rc_min": 1, "rc_max": 2, "rc_values": [7, 8, 9], "signatures": [[10, 11, 12, 13, 14]], "hashes": [[20, 21, 22]]}
    assert IO.flat_public(list(ALL), pub) == [3, 0, 1, 2, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21, 22]
    assert IO.flat_public(["pedersen", "rc16"], pub) == [2, 0, 2, 1, 2, 3, 7, 8, 9, 20, 21, 22]


# ---- the kernels' lane logic on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "builtins_boundary_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.bbs_combine.restype = lib.bbs_dense.restype = lib.bbs_points.restype = ctypes.c_int
    lib.bbs_combine.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.bbs_dense.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 6 + [
        ctypes.c_size_t]
    lib.bbs_points.argtypes = [ctypes.c_uint, ctypes.c_uint] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [
        ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    return lib


def flat_pub_lde(segments, pub_lde):
    return [col for seg, *_ in IO.layout(segments) for col in pub_lde[seg]]


def run_dense(shim, mask, cols, pub_cols, log_n, alphas, shift, acc=None, alias=False, col_stride=None, null=()):
    trace = np.concatenate([C.felts_np(c) for c in cols])
    pub = np.concatenate([C.felts_np(c) for c in pub_cols])
    out = np.full((len(cols[0]), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)  # the columns' size, whatever log_n claims
    acc_np = None if acc is None else C.felts_np(acc)
    if alias:
        out = acc_np
    err = ctypes.create_string_buffer(160)
    alphas_np, shift_np = C.felts_np(alphas), C.felts_np([shift])  # named: an array must outlive the call that reads it
    a = {"trace": trace.ctypes.data, "pub": pub.ctypes.data, "alphas": alphas_np.ctypes.data, "shift": shift_np.ctypes.data,
         "out": out.ctypes.data}
    a.update({k: None for k in null})
    rc = shim.bbs_dense(mask, log_n, a["trace"], len(cols[0]) if col_stride is None else col_stride, a["pub"], a["alphas"],
                        a["shift"], None if acc_np is None else acc_np.ctypes.data, a["out"], err, 160)
    return rc, C.ints_of(out), err.value.decode()


def run_points(shim, mask, log_n, coef, alphas, shift, pos, cur, null=()):
    n = len(pos)
    out = np.full((max(n, 1), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(160)
    coef_np = C.felts_np(coef)
    pos_np = np.array(pos, dtype=np.uint64)
    cur_np = C.felts_np([v for row in cur for v in row]) if n else np.zeros((1, 4), dtype=np.uint64)
    alphas_np, shift_np = C.felts_np(alphas), C.felts_np([shift])
    a = {"coef": coef_np.ctypes.data, "alphas": alphas_np.ctypes.data, "shift": shift_np.ctypes.data,
         "pos": pos_np.ctypes.data, "cur": cur_np.ctypes.data, "out": out.ctypes.data, "status": status.ctypes.data}
    a.update({k: None for k in null})
    rc = shim.bbs_points(mask, log_n, a["coef"], a["alphas"], a["shift"], n, a["pos"], a["cur"], a["out"], a["status"], err,
                         160)
    return rc, C.ints_of(out)[:n], status.tolist()[:n], err.value.decode()


def run_combine(shim, n_groups, term_groups, cols, alphas, k=None, **over):
    k = len(cols[0]) if k is None else k
    arrays = [C.felts_np(c) for c in cols]
    ptrs = (ctypes.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
    groups = (ctypes.c_uint * max(len(term_groups), 1))(*term_groups)
    out = np.full((max(n_groups, 1) * len(cols[0]), 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    alphas_np = C.felts_np(alphas)
    err = ctypes.create_string_buffer(160)
    a = {"n_groups": n_groups, "n_terms": len(term_groups), "groups": groups, "ptrs": ptrs,
         "alphas_ptr": alphas_np.ctypes.data, "out": out.ctypes.data}
    a.update(over)
    rc = shim.bbs_combine(a["n_groups"], a["n_terms"], a["groups"], a["ptrs"], k, a["alphas_ptr"], a["out"], err, 160)
    return rc, C.ints_of(out), err.value.decode()


@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_host_dense_honest_trace_every_acc_mode(shim, segments, log_n):
    _, pub, trace_lde = C.honest(segments, log_n)
    n, mask = 1 << log_n, C.mask_of(segments)
    alphas = seeded_alphas(segments, 3 * log_n)
    pub_lde = {seg: B.public_columns_lde(desc, IO.term_values(seg, pub, n), n, alphas[a0: a0 + len(desc["terms"])])
               for seg, desc, _, a0 in IO.layout(segments)}
    want = IO.boundary_on_coset(segments, trace_lde, None, n, alphas, pub_lde=pub_lde)
    rc, got, err = run_dense(shim, mask, trace_lde, flat_pub_lde(segments, pub_lde), log_n, alphas, S.GEN)
    assert (rc, err) == (0, "") and got == want
    acc = C.arbitrary_columns(1, 4 * n, "acc")[0]
    summed = [(a + b) % P for a, b in zip(acc, want)]
    pub_cols = flat_pub_lde(segments, pub_lde)
    assert run_dense(shim, mask, trace_lde, pub_cols, log_n, alphas, S.GEN, acc=acc)[1] == summed
    assert run_dense(shim, mask, trace_lde, pub_cols, log_n, alphas, S.GEN, acc=acc, alias=True)[1] == summed


@pytest.mark.parametrize("shift", (S.GEN, C.OTHER_SHIFT), ids=("gen", "other"))
@pytest.mark.parametrize("segments", C.SEGMENT_SETS, ids=C.size_id)
def test_host_dense_arbitrary_columns(shim, segments, shift):
    """Rows of EXTREMES in the trace columns, the public columns, acc and the challenges; two shifts."""
    log_n = C.min_log_n(segments)
    M = 4 << log_n
    cols = C.arbitrary_columns(C.n_cols(segments), M, ("cols", segments))
    pub_lde = C.arbitrary_pub_lde(segments, M, "pub")
    alphas = C.arbitrary_columns(1, IO.n_boundary_alphas(segments), ("alphas", segments))[0]
    acc = C.arbitrary_columns(1, M, "acc2")[0]
    want = IO.boundary_on_coset(segments, cols, None, 1 << log_n, alphas, shift, pub_lde=pub_lde)
    rc, got, _ = run_dense(shim, C.mask_of(segments), cols, flat_pub_lde(segments, pub_lde), log_n, alphas, shift)
    assert rc == 0 and got == want
    assert run_dense(shim, C.mask_of(segments), cols, flat_pub_lde(segments, pub_lde), log_n, alphas, shift, acc=acc,
                     alias=True)[1] == [(a + b) % P for a, b in zip(acc, want)]


@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_host_points_equal_the_dense_column(shim, segments, log_n):
    _, pub, trace_lde = C.honest(segments, log_n)
    n = 1 << log_n
    alphas = ([3, P - 1, 1 << 250, 12345, P - 2] * 2)[:IO.n_boundary_alphas(segments)]
    values = C.values_of(segments, pub, n)
    dense = IO.boundary_on_coset(segments, trace_lde, values, n, alphas)
    coef = IO.flat_coefficients(segments, IO.coefficients(segments, values, n, alphas))
    pos = C.positions(4 * n, seed=1)
    rc, got, status, _ = run_points(shim, C.mask_of(segments), log_n, coef, alphas, S.GEN, pos,
                                    [[c[p] for c in trace_lde] for p in pos])
    assert rc == 0 and status == [0] * len(pos) and got == [dense[p] for p in pos]


@pytest.mark.parametrize("shift", (5, C.OTHER_SHIFT), ids=("five", "other"))
@pytest.mark.parametrize("segments,up", [(s, up) for s in C.SEGMENT_SETS for up in (0, 3)] + [(("rc16",), 9)],
                         ids=C.size_id)
def test_host_points_coefficients_alone(shim, segments, up, shift):
    """Arbitrary coefficients and rows with EXTREMES against Horner in integers; rc16 alone up to k = 512, two
    coefficients per lane of a point's block."""
    log_n = C.min_log_n(segments) + up
    n = 1 << log_n
    coeffs = C.arbitrary_coefficients(segments, n, up)
    alphas = C.arbitrary_columns(1, IO.n_boundary_alphas(segments), ("pa", segments, up))[0]
    rng = random.Random(up)
    pos = [0, 1, 4 * n - 1, 2 * n] + [rng.randrange(4 * n) for _ in range(4)]
    cur = C.arbitrary_columns(8, C.n_cols(segments), ("cur", segments, up))
    rc, got, status, _ = run_points(shim, C.mask_of(segments), log_n, IO.flat_coefficients(segments, coeffs), alphas, shift,
                                    pos, cur)
    assert rc == 0 and status == [0] * 8
    assert got == [IO.boundary_at(segments, n, coeffs, alphas, shift, p, c) for p, c in zip(pos, cur)]


def test_host_points_status_and_neighbours(shim):
    n, log_n = 1024, 10
    coeffs = C.arbitrary_coefficients(ALL, n, "st")
    alphas = list(range(2, 11))
    pos = [5, 4 * n, 6, (1 << 64) - 1, 7, 8, 9, 10]
    cur = [list(range(1, 18)) for _ in pos]
    cur[5][16] = P               # the rc16 segment's s column, which no boundary term reads
    cur[6][0] = (1 << 256) - 1
    cur[7][9] = C.NOT_FELTS[1]   # an ECDSA column no term reads
    rc, got, status, _ = run_points(shim, 7, log_n, IO.flat_coefficients(ALL, coeffs), alphas, S.GEN, pos, cur)
    assert rc == 0 and status == [0, 1, 0, 1, 0, 1, 1, 1]
    for i in (0, 2, 4):
        assert got[i] == IO.boundary_at(ALL, n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [got[i] for i in (1, 3, 5, 6, 7)] == [0] * 5


@pytest.mark.parametrize("k", C.COMBINE_KS)
@pytest.mark.parametrize("n_groups,term_groups", C.COMBINE_SHAPES, ids=lambda v: None if isinstance(v, int) else "".join(map(str, v)))
def test_host_combine_equals_the_integers(shim, n_groups, term_groups, k):
    cols, alphas, want = C.combine_case(n_groups, term_groups, k)
    rc, got, err = run_combine(shim, n_groups, term_groups, cols, alphas)
    assert (rc, err) == (0, "") and got == [v for col in want for v in col]
    desc = {"rows": tuple(range(n_groups)), "terms": tuple((0, d) for d in term_groups)}
    assert want == B.combined_values(desc, cols, alphas)  # the expectation is boundary_ref's


def test_host_argument_rules(shim):
    log_n, n = 10, 1024
    M = 4 * n
    cols = C.arbitrary_columns(17, M, "rules")
    pub_cols = C.arbitrary_columns(7, M, "rules-pub")
    alphas = list(range(1, 10))
    coef = C.arbitrary_columns(1, 3 * 2 + 3 * 1 + 128, "rules-coef")[0]
    row = [list(range(1, 18))]
    assert run_dense(shim, 7, cols, pub_cols, log_n, alphas, 3)[0] == 0
    assert run_points(shim, 7, log_n, coef, alphas, 3, [0], row)[0] == 0
    for mask, ln, shift, stride, null, word in (
            (0, 10, 3, None, (), "segments"), (8, 10, 3, None, (), "segments"), (7, 9, 3, None, (), "log_n"),
            (1, 8, 3, None, (), "log_n"), (5, 8, 3, None, (), "log_n"), (4, 2, 3, None, (), "log_n"),
            (7, 25, 3, None, (), "log_n"), (1, 25, 3, None, (), "log_n"),
            (7, 10, 0, None, (), "shift"), (7, 10, 1, None, (), "shift"), (7, 10, S.root_of_unity(12), None, (), "shift"),
            (7, 10, P, None, (), "shift"), (7, 10, 3, M - 1, (), "col_stride"), (7, 10, 3, None, ("trace",), "trace_lde"),
            (7, 10, 3, None, ("pub",), "pub_lde"), (7, 10, 3, None, ("alphas",), "alphas_host"),
            (7, 10, 3, None, ("shift",), "shift_host"), (7, 10, 3, None, ("out",), "out is NULL")):
        rc, got, err = run_dense(shim, mask, cols, pub_cols, ln, alphas, shift, col_stride=stride, null=null)
        assert rc == -3 and word in err and set(got) == {FILL}, (mask, ln, shift, null)
    for mask, ln, shift, null, word in (
            (0, 10, 3, (), "segments"), (8, 10, 3, (), "segments"), (7, 9, 3, (), "log_n"), (2, 9, 3, (), "log_n"),
            (4, 2, 3, (), "log_n"), (4, 25, 3, (), "log_n"), (7, 25, 3, (), "log_n"), (3, 31, 3, (), "log_n"),
            (7, 10, 0, (), "shift"), (7, 10, P - 1, (), "shift"), (7, 10, 3, ("coef",), "coef"),
            (7, 10, 3, ("alphas",), "alphas_host"), (7, 10, 3, ("shift",), "shift_host"), (7, 10, 3, ("pos",), "pos"),
            (7, 10, 3, ("cur",), "cur"), (7, 10, 3, ("out",), "out is NULL"), (7, 10, 3, ("status",), "status")):
        rc, got, status, err = run_points(shim, mask, ln, coef, alphas, shift, [0], row, null=null)
        assert rc == -3 and word in err and status == [0xEE] and got == [FILL], (mask, ln, shift, null)
    # without rc16 the points call goes up to 30 (refused here only by the NULL that follows the scalar rules)
    assert "coef" in run_points(shim, 3, 30, coef, alphas, 3, [0], row, null=("coef",))[3]
    assert run_points(shim, 7, log_n, coef, alphas, 3, [], [], null=("coef", "alphas", "shift", "pos", "cur"))[0] == 0
    # the combine call
    two = C.arbitrary_columns(2, 4, "rules-combine")
    assert run_combine(shim, 2, (0, 1), two, [1, 2])[0] == 0
    for over, groups, k, word in (({"n_groups": 0}, (0, 1), None, "n_groups"), ({"n_groups": 5}, (0, 1), None, "n_groups"),
                                  ({"n_terms": 0}, (0, 1), None, "n_terms"), ({"n_terms": 9}, (0, 1), None, "n_terms"),
                                  ({"groups": None}, (0, 1), None, "term_groups is NULL"), ({}, (0, 2), None, "at or above"),
                                  ({}, (1, 1), None, "without a term"), ({}, (0, 1), 0, "k out of range"),
                                  ({}, (0, 1), (1 << 30) + 1, "k out of range"), ({"ptrs": None}, (0, 1), None, "values_host"),
                                  ({"ptrs": (ctypes.c_void_p * 2)(None, None)}, (0, 1), None, "NULL column"),
                                  ({"alphas_ptr": None}, (0, 1), None, "alphas_host"), ({"out": None}, (0, 1), None, "out is NULL")):
        over = dict(over)
        rc, got, err = run_combine(shim, over.pop("n_groups", 2), groups, two, [1, 2], k=k, **over)
        assert rc == -3 and word in err and set(got) == {FILL}, (over, groups, k)


def test_shim_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "builtins_boundary_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DBUILTINS_BOUNDARY_SHIM_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "builtins boundary check passed" in run.stdout, run.stdout + run.stderr


# ---- the binding, the header and the answers decided on the host ---------------------------------------------------
def test_header_and_binding_name_the_calls():
    from starkperp import _lib, stark
    header = open(os.path.join(HERE, "..", "include", "starkperp.h")).read()
    for name in ("sp_boundary_combine_dev", "sp_builtins_boundary_dev", "sp_builtins_boundary_points_dev"):
        assert "int %s(" % name in header and name in _lib.declared_symbols()
    for name in ("boundary_combine", "builtins_boundary_public_lde", "builtins_boundary", "builtins_boundary_coefficients",
                 "builtins_boundary_points", "prove_builtin_usage", "verify_builtin_usage", "rc16_fill_tensor"):
        assert callable(getattr(stark, name))
    got = stark.BOUNDARY_DESCRIPTORS["rc16_io"]
    assert (got["air"], tuple(got["rows"]), tuple(got["terms"])) == ("rc16", IO.RC16_IO["rows"], IO.RC16_IO["terms"])
    assert (stark.AIRS["rc16"]["period"], stark.AIRS["rc16"]["n_cols"]) == (IO.RC16_IO["period"], IO.RC16_IO["n_cols"])
    assert stark.BUILTIN_BOUNDARY == {"pedersen": "pedersen_io", "ecdsa": "ecdsa_io", "rc16": "rc16_io"}
    pub = {"rc_min": 1, "rc_max": 2, "rc_values": [7, 8], "signatures": [[10, 11, 12, 13, 14]], "hashes": [[20, 21, 22]]}
    assert stark._builtin_usage_flat(pub, list(ALL)) == IO.flat_public(list(ALL), pub)


def test_rc16_fill_tensor_is_rc16_fill():
    from starkperp import stark
    rng = random.Random(6)
    for total in (1, 2, 16, 128):
        values = C.rc_values_for(8 * total, rng)
        want = stark.rc16_fill(values, total)
        got, lo, hi = stark.rc16_fill_tensor(values, total, "cpu")
        assert (stark.tensor_to_felts(got), lo, hi) == want == S.rc16_fill(values, total)
    with pytest.raises(ValueError):
        stark.rc16_fill_tensor([0, 0xFFFF], 16, "cpu")


def test_verifiers_answer_malformed_before_the_library_is_needed():
    from starkperp import stark
    for case in (None, 7, [], {}, {"air": "builtins"}, {"air": "builtins_io"}, {"air": "pedersen_io"},
                 {"segments": ["rc16"], "n": 8}):
        assert stark.verify_builtin_usage(case) == (False, "malformed")
    for verify in (stark.verify, stark.verify_builtins, stark.verify_hashes, stark.verify_signatures):
        assert verify({"air": "builtins_io"}) == (False, "malformed")
