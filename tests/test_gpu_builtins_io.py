"""The builtins proof bound to its statement, on the GPU: sp_boundary_combine_dev, sp_builtins_boundary_dev and
sp_builtins_boundary_points_dev against the integers of tests/builtins_io_ref.py for all 7 segment sets, against
sp_boundary[_points]_dev where one segment is present, their statuses and argument rules; then
stark.prove_builtin_usage / verify_builtin_usage end to end - round trips, every lying claim, the tamperings of
tests/test_gpu_builtins_verify.py and statements that break a rule, each answer compared as a whole with
builtins_io_ref.verify_builtins_proof_bound on the C oracle's hash - and the proofs of prove_builtins against one
recorded before this statement existed (tests/golden/builtins_proof_parent.json)."""
import copy
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest

import boundary_ref as B
import builtins_io_cases as C
import builtins_io_ref as IO
from oracle import stark_ref as S
from test_gpu_builtins_verify import TAMPERINGS
from test_gpu_verify import SENTINEL, chash, profiled, ptr, to_device

pytestmark = pytest.mark.gpu
P = S.P
ALL = ("pedersen", "ecdsa", "rc16")
SENTINEL_FELT = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "builtins_proof_parent.json")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from starkperp import _lib, stark
    return torch, _lib.ensure_init(), stark


def dev_cols(torch, cols):
    return torch.stack([to_device(torch, C.felts_np(c)) for c in cols])


def felts(t):
    return C.ints_of(t.cpu().numpy().view(np.uint64))


def flat_pub_lde(segments, pub_lde):
    return [col for seg, *_ in IO.layout(segments) for col in pub_lde[seg]]


def term_columns(stark, segments, pub, n):
    return {s: [stark.felts_to_tensor(v) for v in IO.term_values(s, pub, n)] for s in segments}


def seeded_alphas(segments, seed):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(IO.n_boundary_alphas(segments))]


def points_raw(gpu, mask, log_n, coef, alphas, shift, count, pos, cur, extra=3, null=()):
    """The C call on sentinel-filled outputs of count + extra items: (rc, values, statuses, untouched as it must be)."""
    torch, lib, _ = gpu
    from starkperp import _lib
    out = torch.full((count + extra, 4), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.full((count + extra,), 0xEE, dtype=torch.uint8, device="cuda")
    a = {"coef": ptr(coef), "alphas": _lib.pack_felts(alphas), "shift": _lib.pack_felts([shift]), "pos": ptr(pos),
         "cur": ptr(cur), "out": out.data_ptr(), "status": status.data_ptr()}
    a.update({k: None for k in null})
    rc = lib.sp_builtins_boundary_points_dev(mask, log_n, a["coef"], a["alphas"], a["shift"], count, a["pos"], a["cur"],
                                             a["out"], a["status"], None)
    torch.cuda.synchronize()
    vals, st = felts(out), status.cpu().tolist()
    clean = vals[count:] == [SENTINEL_FELT] * extra and st[count:] == [0xEE] * extra
    if rc != 0:
        clean = clean and vals[:count] == [SENTINEL_FELT] * count and st[:count] == [0xEE] * count
    return rc, vals[:count], st[:count], clean


def dense_raw(gpu, mask, log_n, trace, stride, pub, alphas, shift, acc=None, null=()):
    """The C call on a sentinel-filled output of the columns' size: (rc, values, whether a refused call wrote nothing)."""
    torch, lib, _ = gpu
    from starkperp import _lib
    out = torch.full((trace.shape[1], 4), SENTINEL, dtype=torch.int64, device="cuda")
    a = {"trace": ptr(trace), "pub": ptr(pub), "alphas": _lib.pack_felts(alphas), "shift": _lib.pack_felts([shift]),
         "out": out.data_ptr()}
    a.update({k: None for k in null})
    rc = lib.sp_builtins_boundary_dev(mask, log_n, a["trace"], stride, a["pub"], a["alphas"], a["shift"], ptr(acc), a["out"],
                                      None)
    torch.cuda.synchronize()
    return rc, out, bool((out == SENTINEL).all())


# ---- the three calls against the integers -----------------------------------------------------------------------------
@pytest.mark.parametrize("segments,log_n", C.SIZES, ids=C.size_id)
def test_honest_trace_dense_points_and_combine_equal_the_integers(gpu, segments, log_n):
    torch, lib, stark = gpu
    _, pub, trace_lde = C.honest(segments, log_n)
    n, M = 1 << log_n, 4 << log_n
    alphas = seeded_alphas(segments, 5 * log_n)
    values = C.values_of(segments, pub, n)
    want = IO.boundary_on_coset(segments, trace_lde, values, n, alphas)
    trace_t = dev_cols(torch, trace_lde)
    columns = term_columns(stark, segments, pub, n)
    pub_lde = stark.builtins_boundary_public_lde(segments, columns, n, alphas)
    want_pub = [col for seg, desc, _, a0 in IO.layout(segments)
                for col in B.public_columns_lde(desc, values[seg], n, alphas[a0: a0 + len(desc["terms"])])]
    assert felts(pub_lde.reshape(-1, 4)) == [v for col in want_pub for v in col]
    (got, launches, units) = profiled(lib, lambda: stark.builtins_boundary(segments, trace_t, pub_lde, n, alphas))
    assert (launches, units) == (1, M) and felts(got) == want  # ONE bracket entry: the table build and the elementwise launch
    acc = to_device(torch, C.felts_np(C.arbitrary_columns(1, M, "gpu-acc")[0]))
    summed = stark.felt_add(acc, got)
    assert torch.equal(stark.builtins_boundary(segments, trace_t, pub_lde, n, alphas, acc=acc), summed)
    assert torch.equal(stark.builtins_boundary(segments, trace_t, pub_lde, n, alphas, acc=acc, out=acc), summed)
    # the points call at the opened rows: what the dense call wrote
    coef = stark.builtins_boundary_coefficients(segments, columns, n, alphas)
    assert felts(coef) == IO.flat_coefficients(segments, IO.coefficients(segments, values, n, alphas))
    pos = C.positions(M, seed=2)
    idx = torch.tensor(pos, dtype=torch.int64, device="cuda")
    cur = trace_t[:, idx, :].permute(1, 0, 2).contiguous()
    ((out, st), launches, units) = profiled(lib, lambda: stark.builtins_boundary_points(segments, n, coef, alphas, S.GEN, idx, cur))
    assert (launches, units) == (1, len(pos)) and st.cpu().tolist() == [0] * len(pos)
    assert felts(out) == [want[p] for p in pos]


@pytest.mark.parametrize("shift", (S.GEN, C.OTHER_SHIFT), ids=("gen", "other"))
@pytest.mark.parametrize("segments", C.SEGMENT_SETS, ids=C.size_id)
def test_arbitrary_columns_with_extremes(gpu, segments, shift):
    torch, lib, stark = gpu
    log_n = C.min_log_n(segments)
    n, M, mask = 1 << log_n, 4 << log_n, C.mask_of(segments)
    cols = C.arbitrary_columns(C.n_cols(segments), M, ("cols", segments))
    pub_lde = C.arbitrary_pub_lde(segments, M, "pub")
    alphas = C.arbitrary_columns(1, IO.n_boundary_alphas(segments), ("alphas", segments))[0]
    want = IO.boundary_on_coset(segments, cols, None, n, alphas, shift, pub_lde=pub_lde)
    rc, out, _ = dense_raw(gpu, mask, log_n, dev_cols(torch, cols), M, dev_cols(torch, flat_pub_lde(segments, pub_lde)),
                           alphas, shift)
    assert rc == 0 and felts(out) == want
    coeffs = C.arbitrary_coefficients(segments, n, "gpu")
    rng = random.Random(log_n)
    pos = [0, 1, M - 1, M // 2] + [rng.randrange(M) for _ in range(4)]
    cur = C.arbitrary_columns(8, C.n_cols(segments), ("cur", segments))
    rc, vals, st, clean = points_raw(gpu, mask, log_n, to_device(torch, C.felts_np(IO.flat_coefficients(segments, coeffs))),
                                     alphas, shift, 8, to_device(torch, np.array(pos, dtype=np.uint64)),
                                     to_device(torch, C.felts_np([v for row in cur for v in row])))
    assert rc == 0 and clean and st == [0] * 8
    assert vals == [IO.boundary_at(segments, n, coeffs, alphas, shift, p, c) for p, c in zip(pos, cur)]


def test_rc16_points_with_two_coefficients_per_lane(gpu):
    """k = 512: above one block's stride of 256."""
    torch, lib, stark = gpu
    segments, log_n = ("rc16",), 12
    n, M = 1 << log_n, 4 << log_n
    coeffs = C.arbitrary_coefficients(segments, n, "k512")
    pos = [0, M - 1, 12345, 7]
    cur = C.arbitrary_columns(4, 3, "k512-cur")
    rc, vals, st, clean = points_raw(gpu, 4, log_n, to_device(torch, C.felts_np(coeffs["rc16"][0])), [P - 3], 5, 4,
                                     to_device(torch, np.array(pos, dtype=np.uint64)),
                                     to_device(torch, C.felts_np([v for row in cur for v in row])))
    assert rc == 0 and clean and st == [0] * 4
    assert vals == [IO.boundary_at(segments, n, coeffs, [P - 3], 5, p, c) for p, c in zip(pos, cur)]


# ---- against the single-AIR calls -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole_case():
    """Arbitrary columns for all three segments at n = 1024, on the device: (trace [17, M, 4], pub [7, M, 4], alphas,
    coefficients by segment, their device arrays by segment)."""
    import torch
    M = 4096
    trace = dev_cols(torch, C.arbitrary_columns(17, M, "whole"))
    pub = dev_cols(torch, C.arbitrary_columns(7, M, "whole-pub"))
    coeffs = C.arbitrary_coefficients(ALL, 1024, "whole")
    coef_t = {s: to_device(torch, C.felts_np([c for g in coeffs[s] for c in g])) for s in ALL}
    return trace, pub, seeded_alphas(ALL, "whole"), coeffs, coef_t


SLICES = {"pedersen": (slice(0, 4), slice(0, 3), slice(0, 3)), "ecdsa": (slice(4, 14), slice(3, 6), slice(3, 8)),
          "rc16": (slice(14, 17), slice(6, 7), slice(8, 9))}  # columns, groups, alphas of a segment inside the whole


def test_one_segment_is_the_single_air_call_and_three_are_their_sum(gpu):
    torch, lib, stark = gpu
    trace, pub, alphas, coeffs, coef_t = whole_case()
    n, M = 1024, 4096
    idx = torch.arange(M, dtype=torch.int64, device="cuda")  # every index
    rows = trace.permute(1, 0, 2).contiguous()
    dense, points = {}, {}
    for seg in ALL:
        cs, gs, as_ = SLICES[seg]
        dense[seg] = stark.builtins_boundary((seg,), trace[cs], pub[gs].contiguous(), n, alphas[as_])
        points[seg], st = stark.builtins_boundary_points((seg,), n, coef_t[seg], alphas[as_], S.GEN, idx, rows[:, cs].contiguous())
        assert not st.any()
    for seg, name in (("pedersen", "pedersen_io"), ("ecdsa", "ecdsa_io")):
        cs, gs, as_ = SLICES[seg]
        assert torch.equal(dense[seg], stark.boundary(name, trace[cs], pub[gs].contiguous(), n, alphas[as_]))
        k = n // stark.AIRS[seg]["period"]
        single, st = stark.boundary_points(name, n, coef_t[seg].reshape(3, k, 4), alphas[as_], S.GEN, idx,
                                           rows[:, cs].contiguous())
        assert not st.any() and torch.equal(points[seg], single)
    whole = stark.builtins_boundary(ALL, trace, pub, n, alphas)
    assert torch.equal(whole, stark.felt_add(stark.felt_add(dense["pedersen"], dense["ecdsa"]), dense["rc16"]))
    whole_pts, st = stark.builtins_boundary_points(ALL, n, torch.cat([coef_t[s] for s in ALL]), alphas, S.GEN, idx, rows)
    assert not st.any()
    assert torch.equal(whole_pts, stark.felt_add(stark.felt_add(points["pedersen"], points["ecdsa"]), points["rc16"]))
    want = [IO.boundary_at(ALL, n, coeffs, alphas, S.GEN, p, felts(rows[p])) for p in (0, 1, 2047, 4095)]
    assert [felts(whole_pts[p:p + 1])[0] for p in (0, 1, 2047, 4095)] == want


# ---- statuses and argument edges --------------------------------------------------------------------------------------
def test_points_status_with_good_neighbours_between_bad_items(gpu):
    torch, lib, stark = gpu
    trace, pub, alphas, coeffs, coef_t = whole_case()
    n = 1024
    pos = [5, 4 * n, 6, (1 << 64) - 1, 7, 8, 9, 10, 11]
    cur = [list(range(1, 18)) for _ in pos]
    cur[5][16] = P               # the rc16 segment's s column, which no boundary term reads
    cur[6][0] = (1 << 256) - 1
    cur[7][9] = C.NOT_FELTS[1]   # an ECDSA column no term reads
    rc, vals, st, clean = points_raw(gpu, 7, 10, torch.cat([coef_t[s] for s in ALL]), alphas, S.GEN, len(pos),
                                     to_device(torch, np.array(pos, dtype=np.uint64)),
                                     to_device(torch, C.felts_np([v for row in cur for v in row])))
    assert rc == 0 and clean and st == [0, 1, 0, 1, 0, 1, 1, 1, 0]
    for i in (0, 2, 4, 8):
        assert vals[i] == IO.boundary_at(ALL, n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [vals[i] for i in (1, 3, 5, 6, 7)] == [0] * 5


def test_argument_edges_leave_prefilled_outputs_untouched(gpu):
    torch, lib, stark = gpu
    from starkperp import _lib
    trace, pub, alphas, coeffs, coef_t = whole_case()
    coef = torch.cat([coef_t[s] for s in ALL])
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    cur = trace.permute(1, 0, 2).contiguous()[:1]

    def refused(call):
        (res, launches, _) = profiled(lib, call)
        assert res[0] == -3 and res[-1] and launches == 0
        return _lib.last_error()
    assert dense_raw(gpu, 7, 10, trace, 4096, pub, alphas, 3)[0] == 0
    for mask, ln, shift, stride, null, word in (
            (0, 10, 3, 4096, (), "segments"), (8, 10, 3, 4096, (), "segments"), (7, 9, 3, 4096, (), "log_n"),
            (1, 8, 3, 4096, (), "log_n"), (4, 2, 3, 4096, (), "log_n"), (7, 25, 3, 1 << 27, (), "log_n"),
            (7, 10, 0, 4096, (), "shift"), (7, 10, 1, 4096, (), "shift"), (7, 10, S.root_of_unity(12), 4096, (), "shift"),
            (7, 10, P, 4096, (), "shift"), (7, 10, 3, 4095, (), "col_stride"), (7, 10, 3, 4096, ("trace",), "trace_lde"),
            (7, 10, 3, 4096, ("pub",), "pub_lde"), (7, 10, 3, 4096, ("alphas",), "alphas_host"),
            (7, 10, 3, 4096, ("shift",), "shift_host")):
        err = refused(lambda: dense_raw(gpu, mask, ln, trace, stride, pub, alphas, shift, null=null))
        assert word in err and "sp_builtins_boundary_dev" in err, (mask, ln, shift, null)
    assert "out is NULL" in refused(lambda: dense_raw(gpu, 7, 10, trace, 4096, pub, alphas, 3, null=("out",)))
    assert points_raw(gpu, 7, 10, coef, alphas, 3, 1, pos, cur)[0] == 0
    for mask, ln, shift, null, word in (
            (0, 10, 3, (), "segments"), (8, 10, 3, (), "segments"), (7, 9, 3, (), "log_n"), (2, 9, 3, (), "log_n"),
            (4, 2, 3, (), "log_n"), (4, 25, 3, (), "log_n"), (3, 31, 3, (), "log_n"), (7, 10, 0, (), "shift"),
            (7, 10, P - 1, (), "shift"), (7, 10, 3, ("coef",), "coef"), (7, 10, 3, ("alphas",), "alphas_host"),
            (7, 10, 3, ("shift",), "shift_host"), (7, 10, 3, ("pos",), "pos"), (7, 10, 3, ("cur",), "cur"),
            (7, 10, 3, ("out",), "out is NULL"), (7, 10, 3, ("status",), "status")):
        err = refused(lambda: points_raw(gpu, mask, ln, coef, alphas, shift, 1, pos, cur, null=null))
        assert word in err and "sp_builtins_boundary_points_dev" in err, (mask, ln, shift, null)
    # a count of 0 is SP_OK without a launch, NULL arrays allowed; above 2^30 points is refused from the count alone
    (res, launches, _) = profiled(lib, lambda: points_raw(gpu, 7, 10, None, alphas, 3, 0, None, None))
    assert res[0] == 0 and res[3] and launches == 0
    small = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    st8 = torch.full((8,), 0xEE, dtype=torch.uint8, device="cuda")
    (rc, launches, _) = profiled(lib, lambda: lib.sp_builtins_boundary_points_dev(
        7, 10, ptr(coef), _lib.pack_felts(alphas), _lib.pack_felts([3]), (1 << 30) + 1, ptr(pos), ptr(cur), small.data_ptr(),
        st8.data_ptr(), None))
    assert rc == -3 and launches == 0 and "2^30" in _lib.last_error()
    # the combine call
    cols = [to_device(torch, C.felts_np(c)) for c in C.arbitrary_columns(2, 4, "edge-combine")]
    out = torch.full((2, 4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    ptrs = (ctypes.c_void_p * 2)(*[c.data_ptr() for c in cols])
    grp = lambda *g: (ctypes.c_uint * len(g))(*g)
    a12 = _lib.pack_felts([1, 2])
    combine = lambda ng, nt, g, v, k, al, o: lib.sp_boundary_combine_dev(ng, nt, g, v, k, al, o, None)
    for args, word in (((0, 2, grp(0, 1), ptrs, 4, a12, out.data_ptr()), "n_groups"),
                       ((5, 2, grp(0, 1), ptrs, 4, a12, out.data_ptr()), "n_groups"),
                       ((2, 0, grp(0, 1), ptrs, 4, a12, out.data_ptr()), "n_terms"),
                       ((2, 9, grp(0, 1), ptrs, 4, a12, out.data_ptr()), "n_terms"),
                       ((2, 2, None, ptrs, 4, a12, out.data_ptr()), "term_groups is NULL"),
                       ((2, 2, grp(0, 2), ptrs, 4, a12, out.data_ptr()), "at or above"),
                       ((2, 2, grp(1, 1), ptrs, 4, a12, out.data_ptr()), "without a term"),
                       ((2, 2, grp(0, 1), ptrs, 0, a12, out.data_ptr()), "k out of range"),
                       ((2, 2, grp(0, 1), ptrs, (1 << 30) + 1, a12, out.data_ptr()), "k out of range"),
                       ((2, 2, grp(0, 1), None, 4, a12, out.data_ptr()), "values_host"),
                       ((2, 2, grp(0, 1), (ctypes.c_void_p * 2)(cols[0].data_ptr(), None), 4, a12, out.data_ptr()), "NULL column"),
                       ((2, 2, grp(0, 1), ptrs, 4, None, out.data_ptr()), "alphas_host"),
                       ((2, 2, grp(0, 1), ptrs, 4, a12, None), "out is NULL")):
        (rc, launches, _) = profiled(lib, lambda: combine(*args))
        assert rc == -3 and launches == 0 and word in _lib.last_error() and "sp_boundary_combine_dev" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((small == SENTINEL).all()) and st8.cpu().tolist() == [0xEE] * 8


@pytest.mark.parametrize("k", C.COMBINE_KS)
@pytest.mark.parametrize("n_groups,term_groups", C.COMBINE_SHAPES, ids=lambda v: None if isinstance(v, int) else "".join(map(str, v)))
def test_combine_equals_boundary_combined(gpu, n_groups, term_groups, k):
    torch, lib, stark = gpu
    cols, alphas, want = C.combine_case(n_groups, term_groups, k)
    tensors = [to_device(torch, C.felts_np(c)) for c in cols]
    (got, launches, units) = profiled(lib, lambda: stark.boundary_combine(list(term_groups), n_groups, tensors, alphas))
    assert (launches, units) == (1, k)
    desc = {"rows": tuple(range(n_groups)), "terms": tuple((0, d) for d in term_groups)}
    assert torch.equal(got, stark._boundary_combined(desc, cols, alphas, "cuda"))
    assert felts(got.reshape(-1, 4)) == [v for col in want for v in col]


# ---- end to end -------------------------------------------------------------------------------------------------------
ROUND_TRIPS = ((ALL, 10), (ALL, 11), (("rc16",), 3), (("rc16",), 6), (("pedersen", "rc16"), 9))


def final_log_of(log_n):
    return min(6, log_n + 2 - 3)  # at least three layers


@functools.lru_cache(maxsize=None)
def proof_of(segments, log_n, n_queries, claim=None):
    """prove_builtin_usage on the instances of the case; `claim` names one of C.lies."""
    from starkperp import stark
    hashes, sigs, values = C.instances(segments, log_n)
    claims = None
    if claim is not None:
        (key, bad), = [({"pedersen": "hashes", "ecdsa": "signatures", "rc16": "rc_values"}[seg], bad)
                       for what, seg, bad in C.lies(segments, C.honest(segments, log_n)[1]) if what == claim]
        claims = {key: bad[key]}
    return stark.prove_builtin_usage(hashes or None, sigs or None, values or None, n_queries=n_queries, seed=3,
                                     final_log=final_log_of(log_n), log_rows=log_n, claims=claims)


@pytest.mark.parametrize("segments,log_n", ROUND_TRIPS, ids=C.size_id)
def test_round_trip_is_accepted_by_both_verifiers(gpu, segments, log_n):
    torch, lib, stark = gpu
    proof = proof_of(segments, log_n, 8)
    fl = final_log_of(log_n)
    assert (proof["air"], proof["n"], tuple(proof["segments"]), len(proof["queries"])) == ("builtins_io", 1 << log_n, segments, 8)
    assert proof["public_inputs"] == C.honest(segments, log_n)[1]  # h, rc_min and rc_max are the integers' own
    assert stark.verify_builtin_usage(proof, final_log=fl) == (True, "ok")
    assert stark.verify_builtin_usage(proof, final_log=fl, n_queries=8) == (True, "ok")
    assert stark.verify_builtin_usage(proof, final_log=fl, n_queries=7) == (False, "shape")
    assert IO.verify_builtins_proof_bound(proof, hash2=chash, final_log=fl) == (True, "ok")
    for other in (stark.verify, stark.verify_builtins):
        assert other(proof, final_log=fl) == (False, "malformed")
    assert stark.verify_builtin_usage(dict(proof, air="builtins"), final_log=fl) == (False, "malformed")


LIES = [(segs, log_n, what) for segs, log_n in ((ALL, 10), (("rc16",), 3), (("pedersen", "rc16"), 9))
        for what, _, _ in C.lies(segs, {"hashes": [[0, 0, 0]], "signatures": [[1, 1, 1, 1, 1]], "rc_values": [1, 2]})]


@pytest.mark.parametrize("segments,log_n,what", LIES, ids=C.size_id)
def test_a_lying_claim_is_rejected_by_both_verifiers(gpu, segments, log_n, what):
    torch, lib, stark = gpu
    proof = proof_of(segments, log_n, 2, what)
    fl = final_log_of(log_n)
    honest = C.honest(segments, log_n)[1]
    assert proof["public_inputs"] != honest and {k: len(v) if isinstance(v, list) else v for k, v in proof["public_inputs"].items()} \
        == {k: len(v) if isinstance(v, list) else v for k, v in honest.items()}
    assert stark.verify_builtin_usage(proof, final_log=fl) == (False, "final layer degree")
    assert IO.verify_builtins_proof_bound(proof, hash2=chash, final_log=fl) == (False, "final layer degree")


def _edit(path, fn):
    def f(p):
        o = p
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = fn(o[path[-1]])
    return f


# statements that break a rule, or say something else than what was proved: all on the proof of the three segments
STATEMENTS = {
    "a hash triple dropped": _edit(("public_inputs", "hashes"), lambda v: v[:-1]),
    "a hash triple too many": _edit(("public_inputs", "hashes"), lambda v: v + [v[0]]),
    "a hash x that is no felt": _edit(("public_inputs", "hashes", 0, 0), lambda v: P),
    "a hash h that is no felt": _edit(("public_inputs", "hashes", 1, 2), lambda v: 2**256 - 1),
    "a signature dropped": _edit(("public_inputs", "signatures"), lambda v: []),
    "a signature's s = 0": _edit(("public_inputs", "signatures", 0, 2), lambda v: 0),
    "a key off the curve": _edit(("public_inputs", "signatures", 0, 4), lambda v: v ^ 1),
    "an rc value of 2^128": _edit(("public_inputs", "rc_values", 3), lambda v: 1 << 128),
    "no rc value": _edit(("public_inputs", "rc_values"), lambda v: []),
    "rc values whose fill does not fit": _edit(("public_inputs", "rc_values", 0), lambda v: 0xFFFF),
    "rc_min + 1": _edit(("public_inputs", "rc_min"), lambda v: v + 1),
    "rc_max + 1": _edit(("public_inputs", "rc_max"), lambda v: v + 1),
    "a changed hash x": _edit(("public_inputs", "hashes", 0, 0), lambda v: v ^ 1),
    "a changed hash h": _edit(("public_inputs", "hashes", 1, 2), lambda v: v ^ 1),
    "a changed message hash": _edit(("public_inputs", "signatures", 0, 0), lambda v: v ^ 1),
    "two rc values swapped": _edit(("public_inputs", "rc_values"), lambda v: [v[1], v[0]] + v[2:]),
    "an rc value appended that is already there": _edit(("public_inputs", "rc_values"), lambda v: v + [v[0]]),
}
E2E = sorted(TAMPERINGS) + sorted(STATEMENTS)


@pytest.mark.parametrize("what", E2E)
def test_verify_builtin_usage_agrees_with_the_integer_verifier(gpu, what):
    torch, lib, stark = gpu
    proof = copy.deepcopy(proof_of(ALL, 10, 3))
    (TAMPERINGS[what][1] if what in TAMPERINGS else STATEMENTS[what])(proof)
    want = IO.verify_builtins_proof_bound(proof, hash2=chash, final_log=6)
    assert stark.verify_builtin_usage(proof, final_log=6) == want, what
    assert want == (True, "ok") if what == "nothing" else not want[0]
    if what in STATEMENTS and not what.startswith(("a changed", "two rc", "an rc value appended")):
        assert want == (False, "public inputs")


def test_malformed_statements(gpu):
    torch, lib, stark = gpu
    proof = proof_of(ALL, 10, 3)
    for path, value in ((("public_inputs", "hashes"), None), (("public_inputs", "hashes", 0), [1, 2]),
                        (("public_inputs", "hashes", 0, 1), 1 << 256), (("public_inputs", "hashes", 0, 1), "7"),
                        (("public_inputs", "rc_values"), None), (("public_inputs", "rc_values", 0), -1),
                        (("public_inputs", "rc_values", 0), 1.0), (("air",), "builtins")):
        bad = copy.deepcopy(proof)
        _edit(path, lambda v: value)(bad)
        assert stark.verify_builtin_usage(bad) == (False, "malformed"), path
    bad = copy.deepcopy(proof)
    del bad["air"]
    assert stark.verify_builtin_usage(bad) == (False, "malformed")


# ---- the unbound proof is what it was ----------------------------------------------------------------------------------
def test_prove_builtins_proof_is_the_recorded_one(gpu):
    """prove_builtins on the three-segment case at n = 1024, 2 queries, seed 5, against the dict recorded from the
    commit before _commit_builtins took a statement hook."""
    torch, lib, stark = gpu
    hashes, sigs, values = C.instances(ALL, 10)
    proof = stark.prove_builtins(hashes, sigs, values, n_queries=2, seed=5)
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert proof == recorded
    assert stark.verify_builtins(proof) == (True, "ok")
