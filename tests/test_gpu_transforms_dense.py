"""Dense parity of the prover's transforms - sp_ntt_dev, sp_lde_dev, sp_interpolate_dev, sp_coset_eval_dev,
sp_fri_fold_dev - with the C reference (oracle/starkref.c cref_ntt ..., itself pinned by tests/test_transform_ref_cpu.py)
at every pass plan and argument edge of tests/transform_cases.py.  Every comparison is np.array_equal on the uint64 words
of whole arrays: no sampling, no round trips, no tolerance."""
import random

import numpy as np
import pytest

import transform_cases as cases
from oracle import cref, stark_ref as S

pytestmark = pytest.mark.gpu
P = S.P
SP_ERR_BAD_ARGUMENT = -3


@pytest.fixture(scope="module")
def stark():
    from starkperp import stark as st
    return st


def to_dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().contiguous().numpy().view(np.uint64)


def first_mismatch(got, want):
    """Where two felt arrays first differ - for the assertion message only."""
    bad = np.flatnonzero((got != want).reshape(-1, 4).any(axis=1))
    return "equal" if bad.size == 0 else "%d of %d felts differ, first at flat index %d" % (bad.size, got.size // 4, bad[0])


def column(kind, n, seed):
    return cases.random_column(n, seed) if kind == "random" else cases.extreme_column(n, seed)


def interpolate(stark, cols):
    """sp_interpolate_dev on [ncols, n, 4]."""
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    out = torch.empty_like(cols)
    _lib.check(lib.sp_interpolate_dev(cols.data_ptr(), out.data_ptr(), cols.shape[0], cols.shape[1].bit_length() - 1,
                                      stark._stream()), "sp_interpolate_dev")
    return out


def coset_eval(stark, coef, shift):
    """sp_coset_eval_dev on [ncols, n, 4]."""
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    out = torch.empty_like(coef)
    _lib.check(lib.sp_coset_eval_dev(coef.data_ptr(), out.data_ptr(), coef.shape[0], coef.shape[1].bit_length() - 1,
                                     _lib.pack_felts([shift]), stark._stream()), "sp_coset_eval_dev")
    return out


# ---- f. FRI fold (first in the file: a process that starts here has no inverse twiddle table cached yet) -----------------
def test_fri_fold_does_not_depend_on_the_cached_twiddle_table(stark):
    """fri_twiddles strides through the LARGEST inverse twiddle table the process has built.  Fold a 2^9 layer, make the
    library cache a larger inverse table (an inverse NTT of 2^15 points), fold the same layer again: both are the
    oracle's fold.  In a process that ran larger inverse transforms before, both folds stride through that larger table."""
    rng = random.Random(909)
    layer = cases.ints_from_felts(cases.extreme_column(1 << 9, 909))
    beta, shift = rng.randrange(P), rng.randrange(1, P)
    want = S.fri_fold(layer, beta, shift)
    t = stark.felts_to_tensor(layer)
    assert stark.tensor_to_felts(stark.fri_fold(t, beta, shift)) == want
    col = cases.random_column(1 << 15, 915)
    assert np.array_equal(to_host(stark.ntt(to_dev(col), inverse=True)), cref.ntt_dense(col, inverse=True))
    assert stark.tensor_to_felts(stark.fri_fold(t, beta, shift)) == want


@pytest.mark.parametrize("kind", ("random", "extreme"))
@pytest.mark.parametrize("log_m", cases.FOLD_SIZES)
def test_fri_fold_matches_oracle(stark, log_m, kind):
    m = 1 << log_m
    rng = random.Random(1000 + log_m)
    layer_arr = column(kind, m, 1100 + log_m)
    layer = cases.ints_from_felts(layer_arr)
    t = to_dev(layer_arr)
    for beta in (0, 1, P - 1, rng.randrange(P)):
        for shift in (3, P - 1, rng.randrange(1, P)):
            got = to_host(stark.fri_fold(t, beta, shift))
            want = cases.felts_from_ints(S.fri_fold(layer, beta, shift))
            assert np.array_equal(got, want), (log_m, kind, beta, shift, first_mismatch(got, want))


# ---- a. NTT, dense, per plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "extreme"))
@pytest.mark.parametrize("log_n", cases.NTT_DENSE)
def test_ntt_dense_per_plan(stark, log_n, kind):
    """Forward and inverse sp_ntt_dev, whole output against the C reference, at every plan of transform_cases.PLAN_CLASSES
    from 11 to 21 and at 23, the smallest size no test had run.  Sizes 24 and 25 are left out for time (the reference
    takes tens of seconds there): they stay without any dense check, 22 and 26 keep the sparse checks of
    test_gpu_stark.py."""
    col = column(kind, 1 << log_n, 2000 + log_n)
    t = to_dev(col)
    for inverse in (False, True):
        got = to_host(stark.ntt(t, inverse=inverse))
        want = cref.ntt_dense(col, inverse=inverse)
        assert np.array_equal(got, want), (log_n, kind, inverse, first_mismatch(got, want))


# ---- b. structured columns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", cases.V_VALUES, ids=("full_limbs", "2p251m1", "pm1"))
@pytest.mark.parametrize("log_n", cases.STRUCTURED)
def test_interpolate_structured_columns(stark, log_n, v):
    """sp_interpolate_dev (the DIF plan, lazy stores between its passes) on constant(v) and every square(v, k) in ONE
    launch of log_n + 1 columns: the largest sum or difference at every stage depth, the all-sum element doubling through
    every stage, and every column stride of grid.y."""
    cols = cases.structured_columns(log_n, v)
    got = to_host(interpolate(stark, to_dev(cols)))
    for c in range(cols.shape[0]):
        want = cref.interpolate_dense(cols[c])
        assert np.array_equal(got[c], want), (log_n, hex(v), "column %d" % c, first_mismatch(got[c], want))


# ---- c. LDE, dense: the DIT plan and the fused padding --------------------------------------------------------------------
def lde_columns(log_n):
    n = 1 << log_n
    return np.stack([cases.random_column(n, 3000 + log_n), cases.extreme_column(n, 3100 + log_n),
                     cases.constant_column(n, 2**232 - 1)])


def check_lde(stark, cols, log_blowup, shift):
    got = to_host(stark.lde(to_dev(cols), blowup_log=log_blowup, shift=shift))
    want = cref.lde_dense(cols, log_blowup, shift)
    assert got.shape == want.shape
    for c in range(cols.shape[0]):
        assert np.array_equal(got[c], want[c]), (cols.shape[1], log_blowup, hex(shift), "column %d" % c,
                                                 first_mismatch(got[c], want[c]))


@pytest.mark.parametrize("log_n,log_blowup", cases.LDE_DENSE)
def test_lde_dense(stark, log_n, log_blowup):
    check_lde(stark, lde_columns(log_n), log_blowup, 3)


@pytest.mark.parametrize("which", ("random", "minus_one"))
def test_lde_dense_other_shifts(stark, which):
    log_n, log_blowup = cases.LDE_SHIFTS_AT
    shift = P - 1 if which == "minus_one" else random.Random(172).randrange(2, P - 1)
    check_lde(stark, lde_columns(log_n), log_blowup, shift)


# ---- d. LDE argument edges ---------------------------------------------------------------------------------------------
def tiny_columns(log_n, seed):
    n = 1 << log_n
    return np.stack([cases.random_column(n, seed), cases.extreme_column(n, seed + 50)])


@pytest.mark.parametrize("log_blowup", cases.LDE_TINY_BLOWUPS)
@pytest.mark.parametrize("log_n", cases.LDE_TINY_LOG_N)
def test_lde_tiny_sizes_every_blowup(stark, log_n, log_blowup):
    """Where sp_lde_dev's host logic branches: no blowup, the fused padding up to its limit (11), and the unfused path
    above it.  Blowups 12 and 13 returned SP_OK with n transformed felts and m - n uninitialised ones before the unfused
    path existed (smallest case: log_n = 0, log_blowup = 12, one column)."""
    import torch
    cols = tiny_columns(log_n, 4000 + 16 * log_n + log_blowup)
    ints = [cases.ints_from_felts(c) for c in cols]
    t = torch.stack([stark.felts_to_tensor(c) for c in ints])
    got = stark.lde(t, blowup_log=log_blowup, shift=3)
    if log_n + log_blowup <= 12:
        for c in range(2):
            assert stark.tensor_to_felts(got[c]) == S.lde(ints[c], 1 << log_blowup, 3), (log_n, log_blowup, c)
    else:
        want = cref.lde_dense(cols, log_blowup, 3)
        assert np.array_equal(to_host(got), want), (log_n, log_blowup, first_mismatch(to_host(got), want))


@pytest.mark.parametrize("col", (0, 1))
@pytest.mark.parametrize("log_n,log_blowup", cases.LDE_EDGES)
def test_lde_padding_edges(stark, log_n, log_blowup, col):
    """(4, 10), (7, 11): the zero padding fills the contiguous pass exactly (no stage left in it) and strided passes
    follow; (14, 12): the largest shape at a blowup above the tile, 2^26 points per column through the unfused path.
    Both columns go through one launch; one of them is compared per case (the reference of 2^26 points takes its time)."""
    cols = tiny_columns(log_n, 5000 + log_n)
    got = to_host(stark.lde(to_dev(cols), blowup_log=log_blowup, shift=3)[col])
    want = cref.lde_dense(cols[col:col + 1], log_blowup, 3)[0]
    assert np.array_equal(got, want), (log_n, log_blowup, "column %d" % col, first_mismatch(got, want))


@pytest.mark.parametrize("log_n,log_blowup", ((14, 13), (13, 14), (26, 1), (0, 27)))
def test_lde_rejects_sizes_above_the_abi_limit(stark, log_n, log_blowup):
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    buf = torch.zeros((2, 4), dtype=torch.int64, device="cuda")  # never touched: the size check comes first
    rc = lib.sp_lde_dev(buf.data_ptr(), buf.data_ptr(), 1, log_n, log_blowup, _lib.pack_felts([3]), stark._stream())
    assert rc == SP_ERR_BAD_ARGUMENT
    assert not buf.any().item()


# ---- e. interpolate + coset evaluation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", cases.COSET_SIZES)
def test_interpolate_then_coset_eval(stark, log_n):
    """The four cosets 3 w^c of the blowup-4 domain, three columns per launch: each equals the C coset evaluation, and
    interleaved they are sp_lde_dev's output."""
    n = 1 << log_n
    cols = np.stack([cases.random_column(n, 6000 + log_n), cases.extreme_column(n, 6100 + log_n),
                     cases.constant_column(n, P - 1)])
    t = to_dev(cols)
    coef = interpolate(stark, t)
    coef_ref = [cref.interpolate_dense(c) for c in cols]
    got_coef = to_host(coef)
    for c in range(3):
        assert np.array_equal(got_coef[c], coef_ref[c]), (log_n, "coefficients", c)
    ext = to_host(stark.lde(t, blowup_log=2, shift=3))
    w_big = S.root_of_unity(log_n + 2)
    for k in range(4):
        shift = 3 * pow(w_big, k, P) % P
        got = to_host(coset_eval(stark, coef, shift))
        for c in range(3):
            want = cref.coset_eval_dense(coef_ref[c], shift)
            assert np.array_equal(got[c], want), (log_n, "coset %d" % k, "column %d" % c, first_mismatch(got[c], want))
            assert np.array_equal(got[c], ext[c, k::4]), (log_n, "coset %d against the LDE" % k, "column %d" % c)


# ---- g. streams and the work buffer ---------------------------------------------------------------------------------------
def test_lde_back_to_back_on_fresh_streams(stark):
    """Two LDEs on a non-default stream with no synchronisation between them, the second one large enough to make the
    stream's work buffer grow while the first may be in flight; then the same on a second stream.  All four results are
    those of the default stream with a synchronise between the calls, which are the C reference's."""
    import torch
    small, large = tiny_columns(10, 7010), tiny_columns(14, 7014)
    ts, tl = to_dev(small), to_dev(large)
    want_small = stark.lde(ts, blowup_log=2)
    torch.cuda.synchronize()
    want_large = stark.lde(tl, blowup_log=2)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(want_small), cref.lde_dense(small, 2, 3))
    assert np.array_equal(to_host(want_large), cref.lde_dense(large, 2, 3))
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            got_small = stark.lde(ts, blowup_log=2)
            got_large = stark.lde(tl, blowup_log=2)
        stream.synchronize()
        assert torch.equal(got_small, want_small)
        assert torch.equal(got_large, want_large)
