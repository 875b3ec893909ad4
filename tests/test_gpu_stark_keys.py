"""Batch square roots mod p and x-only Stark keys on the GPU (csrc/keys.hip): sp_felt_sqrt_batch / sp_stark_key_y_batch,
their _dev forms and the *_many layer, against the cases of tests/stark_key_cases.py (Python integers, the reference's
golden keys).  The kernels run 128 lanes per block (KEYS_TPB), one item per lane."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import stark_key_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 128  # csrc/keys.hip KEYS_TPB
SENTINEL = 2**256 - 2**128 - 12345
BAD_ARGUMENT = -3


@pytest.fixture(scope="module")
def lib():
    from starkperp import _lib
    return _lib.ensure_init()


def felts(values):
    from starkperp import batch_np as bn
    return bn.felts_from_ints(values)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def call(lib, fn, values, want_root=True):
    """One host-pointer call: (status list, [root, or None where the sentinel is still there])."""
    from starkperp import _lib, batch_np as bn
    n = len(values)
    a = felts(values)
    out = felts([SENTINEL] * n) if want_root else None
    st = np.full(n, 77, dtype=np.uint8)
    _lib.check(getattr(lib, fn)(ptr(a), None if out is None else ptr(out), ptr(st), n), fn)
    roots = [None if r == SENTINEL else r for r in bn.ints_from_felts(out)] if want_root else None
    return st.tolist(), roots


def test_cpu_cases_in_one_call_each(lib):
    """Everything tests/test_felt_sqrt_cpu.py checks on the host build; the 6 144-item digit sweep is one launch."""
    cases = K.basic_cases() + K.digit_sweep() + [K.all_digits_maximal()]
    squares = K.random_squares()
    status, roots = call(lib, "sp_felt_sqrt_batch", [c[0] for c in cases] + squares)
    for (a, want_status, want_root), st, root in zip(cases, status, roots):
        assert st == want_status and root == want_root, (hex(a), st, root)
    for a, st, root in zip(squares, status[len(cases):], roots[len(cases):]):
        K.check_root(a, st, root)
    keys = K.golden_keys()
    status, ys = call(lib, "sp_stark_key_y_batch", [x for x, _ in keys] + [K.off_curve_key()])
    assert status == [K.OK] * 256 + [K.NON_RESIDUE]
    assert ys == [y for _, y in keys] + [None]


@pytest.fixture(scope="module")
def one_by_one(lib):
    """The seeded mix of residues, non-residues and out-of-range felts, each item in a call of its own."""
    mixed = K.mixed_felts(BLOCK + 1)
    singles = [call(lib, "sp_felt_sqrt_batch", [a]) for a in mixed]
    return mixed, [s[0][0] for s in singles], [s[1][0] for s in singles]


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK, BLOCK + 1])
def test_launch_shape_edges(lib, one_by_one, n):
    mixed, single_status, single_root = one_by_one
    assert {K.OK, K.NON_RESIDUE, K.OUT_OF_RANGE} == set(single_status)
    for at in sorted({0, len(mixed) - n}):  # the same items at other lane positions
        values = mixed[at:at + n]
        status, roots = call(lib, "sp_felt_sqrt_batch", values)
        for a, st, root in zip(values, status, roots):
            K.check_root(a, st, root)
            assert (root is None) == (st != K.OK)  # the sentinel is still there
        assert status == single_status[at:at + n] and roots == single_root[at:at + n]


def test_status_only_and_argument_edges(lib):
    mixed = K.mixed_felts(BLOCK + 1, seed=8) + [0]
    for fn in ("sp_felt_sqrt_batch", "sp_stark_key_y_batch"):
        full, _ = call(lib, fn, mixed)
        only, _ = call(lib, fn, mixed, want_root=False)
        assert only == full and {K.OK, K.NON_RESIDUE, K.OUT_OF_RANGE} == set(only)
        a = felts(mixed)
        st = np.full(len(mixed), 77, dtype=np.uint8)
        before = a.copy()
        assert getattr(lib, fn)(ptr(a), ptr(a), ptr(st), len(mixed)) == BAD_ARGUMENT  # the same array in and out
        assert getattr(lib, fn)(ptr(a), ptr(a[1:]), ptr(st), len(mixed) - 1) == BAD_ARGUMENT  # overlapping
        assert getattr(lib, fn)(ptr(a), None, None, len(mixed)) == BAD_ARGUMENT  # status is required
        assert (a == before).all() and (st == 77).all()
        assert getattr(lib, fn)(ptr(a), ptr(a), ptr(st), 0) == 0  # n == 0 is legal
        assert getattr(lib, fn)(None, None, None, 0) == 0
    # the felt's own status against Euler's criterion, the key's against the curve equation's
    only, _ = call(lib, "sp_stark_key_y_batch", mixed, want_root=False)
    assert only == [K.OUT_OF_RANGE if x >= K.P else K.euler_status(K.rhs(x)) for x in mixed]


def test_dev_calls_on_a_stream(lib):
    """Device tensors on a torch stream: the bytes of the host-pointer calls; once more after sp_shutdown and a fresh
    sp_init - the tables are built again by the first call that needs them."""
    import torch
    from starkperp import _lib
    mixed = K.mixed_felts(BLOCK + 1, seed=9) + [x for x, _ in K.golden_keys()[:32]]
    n = len(mixed)
    want = {fn: call(lib, fn, mixed) for fn in ("sp_felt_sqrt_batch", "sp_stark_key_y_batch")}

    def dev(fn, want_root=True):
        a = torch.from_numpy(felts(mixed).view(np.int64)).cuda()
        out = torch.from_numpy(felts([SENTINEL] * n).view(np.int64)).cuda()
        st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _lib.check(getattr(lib, fn + "_dev")(a.data_ptr(), out.data_ptr() if want_root else None, st.data_ptr(), n,
                                                 side.cuda_stream), fn + "_dev")
        side.synchronize()
        from starkperp import batch_np as bn
        got = bn.ints_from_felts(out.cpu().numpy().view(np.uint64))
        return st.cpu().tolist(), [None if r == SENTINEL else r for r in got]

    for fn in want:
        assert dev(fn) == want[fn]
        status, untouched = dev(fn, want_root=False)
        assert status == want[fn][0] and untouched == [None] * n
    lib.sp_shutdown()
    assert lib.sp_is_initialised() == 0
    _lib.ensure_init()
    for fn in want:
        assert dev(fn) == want[fn]


def test_python_layer():
    from starkperp import batch, batch_np as bn, signature as S
    keys = K.golden_keys()[:32]
    xs = [x for x, _ in keys]
    assert batch.get_y_coordinates_many(xs) == [S.get_y_coordinate(x) for x in xs] == [y for _, y in keys]
    bad = K.off_curve_key()
    with pytest.raises(S.InvalidPublicKeyError):
        S.get_y_coordinate(bad)
    with pytest.raises(S.InvalidPublicKeyError):
        batch.get_y_coordinates_many(xs[:3] + [bad])
    assert batch.get_y_coordinates_many(xs[:3] + [bad] + xs[3:5], strict=False) == [y for _, y in keys[:3]] + [None] + [
        y for _, y in keys[3:5]]
    assert batch.get_y_coordinates_many([]) == [] and batch.is_valid_stark_key_many([]) == []
    rng = random.Random(64)
    seeded = [rng.randrange(K.P) for _ in range(64)]
    valid = batch.is_valid_stark_key_many(seeded)
    assert valid == [S.is_valid_stark_key(x) for x in seeded] and True in valid and False in valid
    # integers outside [0, p) are reduced, as the scalar functions reduce them
    wide = [xs[0] + K.P, xs[1] - K.P, -xs[2], K.P, 2**256 + 5, -1]
    assert batch.is_valid_stark_key_many(wide) == [S.is_valid_stark_key(x) for x in wide]
    want = []
    for x in wide:
        try:
            want.append(S.get_y_coordinate(x))
        except S.InvalidPublicKeyError:
            want.append(None)
    assert batch.get_y_coordinates_many(wide, strict=False) == want
    values = [0, 1, 4, 3, K.P + 4, -3, 9 - 2 * K.P]
    want = [S.sqrt_mod(v, K.P) if S.is_quad_residue(v, K.P) else None for v in values]
    assert batch.sqrt_mod_many(values) == want and want[:5] == [0, 1, 2, None, 2]
    # the NumPy layer passes felts through and reports the ones that are not below p
    roots, st = bn.felt_sqrt(bn.felts_from_ints([4, 3, K.P, 2**256 - 1]))
    assert st.tolist() == [bn.SQRT_OK, bn.SQRT_NON_RESIDUE, bn.SQRT_OUT_OF_RANGE, bn.SQRT_OUT_OF_RANGE]
    assert bn.ints_from_felts(roots) == [2, 0, 0, 0]
    qy, st = bn.stark_key_y(bn.felts_from_ints(xs[:2] + [bad, K.P + xs[0]]))
    assert st.tolist() == [0, 0, bn.SQRT_NON_RESIDUE, bn.SQRT_OUT_OF_RANGE]
    assert bn.ints_from_felts(qy) == [keys[0][1], keys[1][1], 0, 0]
    none, st2 = bn.stark_key_y(bn.felts_from_ints(xs[:2] + [bad, K.P + xs[0]]), want_y=False)
    assert none is None and st2.tolist() == st.tolist()


def test_consistent_with_verify(lib):
    """16 x-only rows of the reference's verify goldens: the x-only verdict is TRUE, and the point key (x, y) with the
    new call's y or with its negation verifies as well."""
    from starkperp import batch_np as bn
    rows = K.valid_xonly_rows(16)
    z, r, s, x = (felts([row[i] for row in rows]) for i in range(4))
    status, ys = call(lib, "sp_stark_key_y_batch", [row[3] for row in rows])
    assert status == [K.OK] * 16
    assert bn.verify_codes(z, r, s, x).tolist() == [1] * 16
    plus = bn.verify_codes(z, r, s, x, felts(ys)).tolist()
    minus = bn.verify_codes(z, r, s, x, felts([K.P - y for y in ys])).tolist()
    assert all(a == 1 or b == 1 for a, b in zip(plus, minus)), (plus, minus)
    assert set(plus) | set(minus) <= {0, 1}  # both candidates are on the curve


def test_plain_c_caller():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_keys")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_keys.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.splitlines() == ["cabi_keys ok"]
