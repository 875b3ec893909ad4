"""Batch point arithmetic on the Stark curve on the GPU (csrc/ec_points.hip): sp_ec_mult_batch, sp_ec_lincomb_batch,
sp_ec_add_batch, their _dev forms and the Python layers, against the cases of tests/ec_point_cases.py (Python integers,
the reference's golden keys), against sp_public_key_batch on batches too large for Python, and against the reference's
pinned verification vectors.  The kernels run 256 lanes per block (EC_TPB), one item per lane."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

import ec_point_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256  # csrc/ec_points.hip EC_TPB
SENTINEL = 2**256 - 2**128 - 12345
BAD_ARGUMENT = -3
ALL_STATUSES = {C.OK, C.INFINITY, C.OUT_OF_RANGE, C.NOT_ON_CURVE}


@pytest.fixture(scope="module")
def lib():
    from starkperp import _lib
    return _lib.ensure_init()


def felts(values):
    from starkperp import batch_np as bn
    return bn.felts_from_ints(values)


def ints(arr):
    from starkperp import batch_np as bn
    return bn.ints_from_felts(arr)


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def columns(op, cases):
    """The input arrays of one entry point, as lists of ints, in the order of its arguments."""
    if op == "mult":
        return [[c[0] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases]]
    if op == "lincomb":
        return [[c[0] for c in cases], [c[1] for c in cases], [c[2][0] for c in cases], [c[2][1] for c in cases]]
    return [[c[0][0] for c in cases], [c[0][1] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases]]


def call(lib, op, cols, subtract=0, want_y=True):
    """One host-pointer call on lists of ints: (status list, [(x, y)], sentinels where nothing was written)."""
    from starkperp import _lib
    n = len(cols[0])
    arrays = [felts(col) for col in cols]
    rx, ry = felts([SENTINEL] * n), felts([SENTINEL] * n)
    st = np.full(n, 77, dtype=np.uint8)
    fn = "sp_ec_%s_batch" % op
    extra = [subtract] if op == "add" else []
    _lib.check(getattr(lib, fn)(*[ptr(a) for a in arrays], *extra, ptr(rx), ptr(ry) if want_y else None, ptr(st), n), fn)
    return st.tolist(), list(zip(ints(rx), ints(ry)))


def check(cases, status, got):
    """status and value of every case; the sentinel still in the outputs of the items that are not OK, and every
    status byte written."""
    assert len(cases) == len(status)
    for case, st, xy in zip(cases, status, got):
        assert st == case[-2], (case, st)
        assert xy == (case[-1] if st == C.OK else (SENTINEL, SENTINEL)), (case, xy)


@pytest.fixture(scope="module")
def case_sets():
    """Computed once: {op: cases}; "add" holds P + Q, "sub" P - Q."""
    adds = C.add_cases()
    return {"mult": C.mult_cases(), "lincomb": C.lincomb_cases(), "add": [c for c in adds if c[2] == 0],
            "sub": [c for c in adds if c[2] == 1]}


def run_cases(lib, name, cases, **kw):
    op = "add" if name == "sub" else name
    return call(lib, op, columns(op, cases), subtract=1 if name == "sub" else 0, **kw)


@pytest.mark.parametrize("name", ["mult", "lincomb", "add", "sub"])
def test_case_set_in_one_call(lib, case_sets, name):
    cases = case_sets[name]
    assert {c[-2] for c in cases} == ALL_STATUSES
    status, got = run_cases(lib, name, cases)
    check(cases, status, got)


@pytest.fixture(scope="module")
def one_by_one(lib, case_sets):
    """For each call a seeded mix of all four statuses, BLOCK + 9 items, each item in a call of its own."""
    out = {}
    for i, name in enumerate(("mult", "lincomb", "add", "sub")):
        mixed = C.pick_mixed(case_sets[name], BLOCK + 9, seed=11 + i)
        singles = [run_cases(lib, name, [c]) for c in mixed]
        status, got = [s[0][0] for s in singles], [s[1][0] for s in singles]
        check(mixed, status, got)
        out[name] = (mixed, status, got)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_launch_shape_edges(lib, one_by_one, n):
    for name, (mixed, single_status, single_got) in one_by_one.items():
        for at in (0, len(mixed) - n):  # the same items at two lane offsets
            part = mixed[at:at + n]
            status, got = run_cases(lib, name, part)
            check(part, status, got)
            assert status == single_status[at:at + n] and got == single_got[at:at + n]
            if n >= 63:
                assert set(status[:64]) == ALL_STATUSES  # all four inside the first wave


def test_argument_edges(lib, case_sets):
    for name in ("mult", "lincomb", "add", "sub"):
        op = "add" if name == "sub" else name
        extra = [1 if name == "sub" else 0] if op == "add" else []
        cases = C.pick_mixed(case_sets[name], 70, seed=5)
        n = len(cases)
        fn = getattr(lib, "sp_ec_%s_batch" % op)
        full_status, full = run_cases(lib, name, cases)
        x_status, x_only = run_cases(lib, name, cases, want_y=False)  # ry == NULL: the same rx, ry never touched
        assert x_status == full_status and [xy[0] for xy in x_only] == [xy[0] for xy in full]
        assert all(xy[1] == SENTINEL for xy in x_only)
        arrays = [felts(col) for col in columns(op, cases)]
        before = [a.copy() for a in arrays]
        rx, ry = felts([SENTINEL] * n), felts([SENTINEL] * n)
        st = np.full(n, 77, dtype=np.uint8)
        ins = [ptr(a) for a in arrays]
        assert fn(*ins, *extra, ptr(rx), ptr(ry), None, n) == BAD_ARGUMENT   # status is required
        assert fn(*ins, *extra, None, ptr(ry), ptr(st), n) == BAD_ARGUMENT    # rx is required
        for i in range(len(arrays)):  # an output equal to an input, or overlapping it
            assert fn(*ins, *extra, ins[i], ptr(ry), ptr(st), n) == BAD_ARGUMENT
            assert fn(*ins, *extra, ptr(rx), ins[i], ptr(st), n) == BAD_ARGUMENT
            assert fn(*ins, *extra, ptr(arrays[i][1:]), ptr(ry), ptr(st), n - 1) == BAD_ARGUMENT
        missing = list(ins)
        missing[-1] = None
        assert fn(*missing, *extra, ptr(rx), ptr(ry), ptr(st), n) == BAD_ARGUMENT
        assert all((a == b).all() for a, b in zip(arrays, before))
        assert ints(rx) == [SENTINEL] * n and ints(ry) == [SENTINEL] * n and (st == 77).all()
        assert fn(*ins, *extra, ins[0], ins[0], None, 0) == 0  # n == 0 is legal, whatever the pointers are
        assert fn(*[None] * len(ins), *extra, None, None, None, 0) == 0


def test_dev_calls_on_streams(lib, case_sets):
    """Device tensors on a torch stream of its own; the same batch on two streams at once (each stream has its own
    ladder scratch); the bytes of the host-pointer call."""
    import torch
    from starkperp import _lib
    for name in ("mult", "lincomb", "add", "sub"):
        op = "add" if name == "sub" else name
        extra = [1 if name == "sub" else 0] if op == "add" else []
        cases = C.pick_mixed(case_sets[name], 2 * BLOCK + 3, seed=21)
        n = len(cases)
        want = run_cases(lib, name, cases)
        ins = [torch.from_numpy(felts(col).view(np.int64)).cuda() for col in columns(op, cases)]
        fn = getattr(lib, "sp_ec_%s_batch_dev" % op)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for side in streams:
            rx = torch.from_numpy(felts([SENTINEL] * n).view(np.int64)).cuda()
            ry = torch.from_numpy(felts([SENTINEL] * n).view(np.int64)).cuda()
            st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
            outs.append((rx, ry, st))
        torch.cuda.synchronize()
        for side, (rx, ry, st) in zip(streams, outs):  # both enqueued before either is waited for
            _lib.check(fn(*[a.data_ptr() for a in ins], *extra, rx.data_ptr(), ry.data_ptr(), st.data_ptr(), n,
                          side.cuda_stream), "sp_ec_%s_batch_dev" % op)
        for side in streams:
            side.synchronize()
        for rx, ry, st in outs:
            got = list(zip(ints(rx.cpu().numpy().view(np.uint64)), ints(ry.cpu().numpy().view(np.uint64))))
            assert (st.cpu().tolist(), got) == want
        # x alone on a stream
        rx, ry, st = outs[0]
        ry.copy_(torch.from_numpy(felts([SENTINEL] * n).view(np.int64)))
        torch.cuda.synchronize()
        _lib.check(fn(*[a.data_ptr() for a in ins], *extra, rx.data_ptr(), None, st.data_ptr(), n,
                      streams[0].cuda_stream), "sp_ec_%s_batch_dev" % op)
        streams[0].synchronize()
        assert ints(rx.cpu().numpy().view(np.uint64)) == [xy[0] for xy in want[1]]
        assert ints(ry.cpu().numpy().view(np.uint64)) == [SENTINEL] * n


def public_keys(lib, scalars):
    """[d G] through sp_public_key_batch, None where d = 0 mod N (which that call refuses)."""
    from starkperp import _lib
    n = len(scalars)
    d = felts([k % C.N or 1 for k in scalars])
    qx, qy = felts([0] * n), felts([0] * n)
    st = np.zeros(n, dtype=np.uint8)
    _lib.check(lib.sp_public_key_batch(ptr(d), ptr(qx), ptr(qy), ptr(st), n), "sp_public_key_batch")
    assert not st.any()
    return [xy if k % C.N else None for k, xy in zip(scalars, zip(ints(qx), ints(qy)))]


def as_cases(points):
    """(status, result) per expected point, None being infinity."""
    return [(C.OK, pt) if pt is not None else (C.INFINITY, None) for pt in points]


def test_identities_on_a_large_batch(lib):
    """4096 + 1 items each, no Python curve arithmetic: the expected points are d G from sp_public_key_batch."""
    n = 4097
    rng = random.Random(4097)
    d = [rng.randrange(1, C.N) for _ in range(n)]
    d2 = [rng.randrange(1, C.N) for _ in range(n)]
    k = [rng.randrange(1, C.N) for _ in range(n)]
    b = [rng.randrange(C.N) for _ in range(n)]
    a = [rng.randrange(C.N) for _ in range(n)]
    for i in range(0, n, 257):   # the sum is infinity
        a[i] = -b[i] * d[i] % C.N
    for i in range(100, n, 257):  # the sum is a doubling
        a[i] = b[i] * d[i] % C.N
    d2[7], d2[300] = C.N - d[7], d[300]  # P + (-P), P + P
    keys = public_keys(lib, d)
    keys2 = public_keys(lib, d2)
    px, py = [pt[0] for pt in keys], [pt[1] for pt in keys]
    # k (d G) == (k d) G
    status, got = call(lib, "mult", [k, px, py])
    check(as_cases(public_keys(lib, [x * y for x, y in zip(k, d)])), status, got)
    # a G + b (d G) == (a + b d) G, infinity exactly where that scalar is 0
    want = public_keys(lib, [x + y * z for x, y, z in zip(a, b, d)])
    assert sum(1 for pt in want if pt is None) == len(range(0, n, 257))
    status, got = call(lib, "lincomb", [a, b, px, py])
    check(as_cases(want), status, got)
    # d1 G + d2 G == (d1 + d2) G,  d1 G - d2 G == (d1 - d2) G
    for sub, sign in ((0, 1), (1, -1)):
        want = public_keys(lib, [x + sign * y for x, y in zip(d, d2)])
        status, got = call(lib, "add", [px, py, [pt[0] for pt in keys2], [pt[1] for pt in keys2]], subtract=sub)
        check(as_cases(want), status, got)
        assert status.count(C.INFINITY) == 1
    # (N - 1) P == -P
    status, got = call(lib, "mult", [[C.N - 1] * n, px, py])
    check([(C.OK, C.neg(pt)) for pt in keys], status, got)


def test_tie_to_the_verification_goldens(lib):
    """The reference's pinned vectors: with w = 1 / s mod N, the x of (z w) G + (r w) Q is r for the valid signatures
    with point keys, and is not r where the golden is False because of a wrong r."""
    rows = json.load(open(os.path.join(C.GOLDEN, "g4_verify.json")))["cases"]
    valid = [c for c in rows if c["label"] == "valid_point" and c["expect"] == "true"]
    wrong = [c for c in rows if c["label"] == "wrong_r" and isinstance(c["key"], list)]
    assert len(valid) >= 15 and len(wrong) >= 16
    picked = valid + wrong
    z, r, s = ([int(c[f], 16) for c in picked] for f in ("z", "r", "s"))
    w = [pow(v, -1, C.N) for v in s]
    qx, qy = [int(c["key"][0], 16) for c in picked], [int(c["key"][1], 16) for c in picked]
    status, got = call(lib, "lincomb", [[x * y % C.N for x, y in zip(z, w)], [x * y % C.N for x, y in zip(r, w)], qx, qy])
    assert status == [C.OK] * len(picked)
    same = [xy[0] == ri for xy, ri in zip(got, r)]
    assert same == [True] * len(valid) + [False] * len(wrong)


def test_python_layers(case_sets):
    from starkperp import batch, batch_np as bn
    fine = {name: [c for c in cases if c[-2] in (C.OK, C.INFINITY)] for name, cases in case_sets.items()}
    m, l, a, s = fine["mult"], fine["lincomb"], fine["add"], fine["sub"]
    assert None in [c[-1] for c in m] and None in [c[-1] for c in l] and None in [c[-1] for c in a]
    assert batch.ec_mult_many([c[0] for c in m], [c[1] for c in m]) == [c[-1] for c in m]
    assert batch.ec_lincomb_many([c[0] for c in l], [c[1] for c in l], [c[2] for c in l]) == [c[-1] for c in l]
    assert batch.ec_add_many([c[0] for c in a], [c[1] for c in a]) == [c[-1] for c in a]
    assert batch.ec_sub_many([c[0] for c in s], [c[1] for c in s]) == [c[-1] for c in s]
    assert batch.ec_mult_many([], []) == [] and batch.ec_add_many([], []) == []
    off = C.off_curve_points()[0]
    for bad in (lambda: batch.ec_mult_many([C.N], [C.GEN]), lambda: batch.ec_mult_many([-1], [C.GEN]),
                lambda: batch.ec_mult_many([1], [(C.P, C.GEN[1])]), lambda: batch.ec_mult_many([0], [off]),
                lambda: batch.ec_lincomb_many([1], [2**256 - 1], [C.GEN]), lambda: batch.ec_lincomb_many([1], [1], [(0, 0)]),
                lambda: batch.ec_add_many([C.GEN], [off]), lambda: batch.ec_sub_many([(C.GEN[0], C.P + 1)], [C.GEN])):
        with pytest.raises(AssertionError):
            bad()
    # the NumPy layer passes everything through and reports it; rows that are not OK are zero
    for name, op in (("mult", "mult"), ("lincomb", "lincomb"), ("add", "add"), ("sub", "add")):
        cases = case_sets[name]
        cols = [bn.felts_from_ints(col) for col in columns(op, cases)]
        if op == "add":
            rx, ry, st = bn.ec_add(*cols, subtract=name == "sub")
        else:
            rx, ry, st = getattr(bn, "ec_" + op)(*cols)
        assert st.tolist() == [c[-2] for c in cases]
        assert list(zip(ints(rx), ints(ry))) == [c[-1] if c[-2] == C.OK else (0, 0) for c in cases]
    rx, ry, st = bn.ec_mult(np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64))
    assert rx.shape == (0, 4) and st.shape == (0,)


def test_plain_c_caller():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_points")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_points.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.splitlines() == ["cabi_points ok"]
