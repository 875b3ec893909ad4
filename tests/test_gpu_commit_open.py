"""Opening committed tables on the GPU (sp_commit_open_dev, sp_commit_open, stark.open_rows): the cases of
tests/commit_open_cases.py against their NumPy answers through both calls, a round trip on real commitments into the
Merkle path verifier, table offsets above 2^32 bytes, the two provers' proofs against the slice-by-slice assembly
they replaced, and a plain-C consumer."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import commit_open_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from starkperp import _lib
    return torch, _lib.ensure_init()


def c_sizes(vals):
    return (ctypes.c_size_t * max(len(vals), 1))(*vals)


def c_ptrs(vals):
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


def to_device(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def profiled(lib, fn):
    """(fn(), launches, units) with the library's launch bracket around fn"""
    from starkperp import _lib
    _lib.check(lib.sp_profile_begin(8), "sp_profile_begin")
    result = fn()
    ms, launches, units = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(lib.sp_profile_end(ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(units)), "sp_profile_end")
    return result, launches.value, units.value


class DeviceOutputs:
    """commit_open_cases.Outputs on the device: the same sentinel fill; the offset arrays stay on the host."""

    def __init__(self, torch, host):
        self.host = host
        self.values, self.leaves, self.siblings = (to_device(torch, a) for a in (host.values, host.leaves, host.siblings))
        self.val_off, self.off = host.val_off, host.off

    def download(self):
        for name in ("values", "leaves", "siblings"):
            getattr(self.host, name)[:] = getattr(self, name).cpu().numpy().view(np.uint64)
        return self.host


def call(lib, a, out, stream=None):
    """sp_commit_open_dev on `stream` (out: DeviceOutputs) or sp_commit_open (out: Outputs, stream None) on an argument
    dict of commit_open_cases.  The host argument arrays are COPIES that are scribbled over as soon as the call returns:
    it must have consumed them by then."""
    dev = stream is not None
    ptr = lambda name: None if name in a["null"] else (
        getattr(out, name).data_ptr() if dev and name in ("values", "leaves", "siblings") else getattr(out, name).ctypes.data)
    cols, levels = c_ptrs(a["cols"]), c_ptrs(a["levels"])
    stride, n_rows, n_cols = c_sizes(a["col_stride"]), c_sizes(a["n_rows"]), c_sizes(a["n_cols"])
    small = a["n_open"] <= 1 << 20  # (the 2^27 zero pages of a refused case are passed as they are)
    table_of, rows = (a["table_of"].copy(), a["rows"].copy()) if small else (a["table_of"], a["rows"])
    args = [a["n_tables"], cols, stride, n_rows, n_cols, levels, a["n_open"], table_of.ctypes.data, rows.ctypes.data,
            ptr("values"), ptr("val_off"), ptr("leaves"), ptr("siblings"), ptr("off")]
    rc = lib.sp_commit_open_dev(*args, stream) if dev else lib.sp_commit_open(*args)
    for arr in (cols, levels, stride, n_rows, n_cols):
        ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
    if small:
        table_of[:] = 0xFFFFFFFF
        rows[:] = 0xFFFFFFFFFFFFFFFF
    return rc


def device_case_args(torch, case):
    tensors = [(to_device(torch, c), to_device(torch, lv)) for c, lv in case.arrays]
    a = {"n_tables": len(case.tables), "cols": [c.data_ptr() for c, _ in tensors],
         "levels": [lv.data_ptr() for _, lv in tensors], "col_stride": [s for _, _, s in case.tables],
         "n_rows": [r for r, _, _ in case.tables], "n_cols": [c for _, c, _ in case.tables], "n_open": case.n_open,
         "table_of": case.table_of, "rows": case.rows, "null": set()}
    return a, tensors


def assert_outputs(case, out, want, want_leaves=True):
    values, val_off, leaves, siblings, off = want
    assert np.array_equal(out.val_off, val_off) and np.array_equal(out.off, off)
    assert np.array_equal(out.values[: len(values)], values)
    assert np.array_equal(out.siblings[: len(siblings)], siblings)
    if want_leaves:
        assert np.array_equal(out.leaves[: case.n_open], leaves)
    else:
        assert C.all_sentinel(out.leaves)
    assert C.all_sentinel(out.values[len(values):]) and C.all_sentinel(out.siblings[len(siblings):])


# ---- 1. the shared cases through both calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c.name)
def test_case_through_both_calls(gpu, case):
    torch, lib = gpu
    want = case.expected()
    a, tensors = device_case_args(torch, case)
    torch.cuda.synchronize()  # the tables are in place before a side stream or a host lane reads them
    side = torch.cuda.Stream()
    out = DeviceOutputs(torch, C.Outputs(case.n_open, len(want[0]) + 2, len(want[3]) + 2))
    torch.cuda.synchronize()
    rc, launches, units = profiled(lib, lambda: call(lib, a, out, side.cuda_stream))
    assert rc == C.SP_OK
    assert (launches, units) == (C.slices_of(case.n_open), case.n_open)  # ONE launch up to the largest class
    assert np.array_equal(out.val_off, want[1]) and np.array_equal(out.off, want[4])  # filled when the call returns
    side.synchronize()
    assert_outputs(case, out.download(), want)
    # the host call, with and without leaves
    for want_leaves in (True, False):
        host = C.Outputs(case.n_open, len(want[0]) + 2, len(want[3]) + 2)
        if not want_leaves:
            a["null"].add("leaves")
        rc, launches, _ = profiled(lib, lambda: call(lib, a, host))
        assert rc == C.SP_OK and launches == C.slices_of(case.n_open)
        assert_outputs(case, host, want, want_leaves)


def test_slice_class_is_the_headers(gpu):
    """commit_open_cases.SLICE_MAX is what the tests plan with: it must be OPEN_SLICE_MAX of the shared header, which
    the host shim reports."""
    src = os.path.join(ROOT, "tests", "host", "commit_open_shim.cpp")
    so = os.path.join(ROOT, "tests", "host", "commit_open_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    shim = ctypes.CDLL(so)
    shim.co_slice_max.restype = ctypes.c_size_t
    assert shim.co_slice_max() == C.SLICE_MAX


@pytest.mark.parametrize("bad", C.BAD, ids=lambda b: b[0])
def test_bad_argument_is_refused_before_anything_is_written(gpu, bad):
    from starkperp import _lib
    torch, lib = gpu
    name, patch, word = bad
    tensors = [(to_device(torch, c), to_device(torch, lv))
               for c, lv in (C.table_arrays(t, *shape) for t, shape in enumerate(C.BASE_TABLES))]
    torch.cuda.synchronize()
    fresh = lambda: C.base_args([c.data_ptr() for c, _ in tensors], [lv.data_ptr() for _, lv in tensors])
    assert call(lib, fresh(), C.Outputs(len(C.BASE_PICKS), 16, 16)) == C.SP_OK  # the base call is good
    for who in ("sp_commit_open_dev", "sp_commit_open"):
        a = fresh()
        patch(a)
        host = C.Outputs(len(C.BASE_PICKS), 16, 16)
        if who == "sp_commit_open_dev":
            out = DeviceOutputs(torch, host)
            torch.cuda.synchronize()
            (rc, launches, _) = profiled(lib, lambda: call(lib, a, out, torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            out.download()
        else:
            (rc, launches, _) = profiled(lib, lambda: call(lib, a, host))
        assert rc == C.SP_ERR_BAD_ARGUMENT and launches == 0
        text = _lib.last_error()
        assert text.startswith(who + ":") and word in text, text
        assert host.untouched()


# ---- 2. round trip on real commitments ------------------------------------------------------------------------------
def open_arrays(lib, tables, picks):
    """sp_commit_open of stark-style tables [(cols [n_cols, n_rows, 4], levels)]: NumPy outputs."""
    from starkperp import _lib
    shapes = [(c.shape[1], c.shape[0]) for c, _ in tables]
    n = len(picks)
    table_of = np.array([t for t, _ in picks], dtype=np.uint32)
    rows = np.array([r for _, r in picks], dtype=np.uint64)
    n_rows, n_cols = c_sizes([s[0] for s in shapes]), c_sizes([s[1] for s in shapes])
    nv, ns = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.sp_commit_open_size(len(tables), n_rows, n_cols, n, table_of.ctypes.data, ctypes.byref(nv),
                                       ctypes.byref(ns)), "sp_commit_open_size")
    values, leaves = np.zeros((nv.value, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    siblings = np.zeros((max(ns.value, 1), 4), dtype=np.uint64)
    val_off, off = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    _lib.check(lib.sp_commit_open(len(tables), c_ptrs([c.data_ptr() for c, _ in tables]), n_rows, n_rows, n_cols,
                                  c_ptrs([lv.data_ptr() for _, lv in tables]), n, table_of.ctypes.data, rows.ctypes.data,
                                  values.ctypes.data, val_off.ctypes.data, leaves.ctypes.data, siblings.ctypes.data,
                                  off.ctypes.data), "sp_commit_open")
    return values, val_off, leaves, siblings[: ns.value], off, rows


def test_round_trip_on_real_commitments(gpu):
    from starkperp import batch_np, stark
    torch, lib = gpu
    rng = random.Random(71)
    P = stark.FIELD_PRIME
    wide = stark.felts_to_tensor([rng.randrange(P) for _ in range(3 * 16)]).reshape(3, 16, 4).contiguous()
    narrow = stark.felts_to_tensor([rng.randrange(P) for _ in range(8)]).reshape(1, 8, 4).contiguous()
    tables = [(wide, stark.commit_rows(wide)), (narrow, stark.commit_rows(narrow))]
    roots = [batch_np.felts_from_ints([stark.root_of(lv)])[0] for _, lv in tables]
    torch.cuda.synchronize()
    picks = [(0, r) for r in range(16)] + [(1, r) for r in range(8)]
    values, val_off, leaves, siblings, off, rows = open_arrays(lib, tables, picks)
    assert list(val_off) == [3 * i for i in range(17)] + [48 + i for i in range(1, 9)]
    assert list(off) == [4 * i for i in range(17)] + [64 + 3 * i for i in range(1, 9)]
    hashed, status = batch_np.pedersen_chains_ragged(values, val_off)
    assert not status.any() and np.array_equal(hashed, leaves)
    assert np.array_equal(leaves[16:], values[48:])  # one column: the leaf is the value itself
    expected = np.stack([roots[t] for t, _ in picks])
    verdict, status = batch_np.merkle_verify_paths(leaves, siblings, rows, expected, offsets=off)
    assert verdict.all() and not status.any()
    for item, level in ((5, 2), (20, 0)):
        bent = siblings.copy()
        bent[off[item] + level, 1] ^= np.uint64(1)
        verdict, _ = batch_np.merkle_verify_paths(leaves, bent, rows, expected, offsets=off)
        assert [i for i, v in enumerate(verdict) if not v] == [item]


# ---- 3. offsets above 2^32 bytes ------------------------------------------------------------------------------------
def test_table_offsets_above_4_gib(gpu):
    """One column of 2^27 rows: 4 GiB of values, 8 GiB of levels, neither initialised except for the ~30 felts the
    three openings read, which carry tags.  A 32-bit felt or byte offset anywhere would read an untagged felt."""
    torch, lib = gpu
    n_rows = 1 << 27
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory")
    col = torch.empty((1, n_rows, 4), dtype=torch.int64, device="cuda")
    levels = torch.empty((2 * n_rows - 1, 4), dtype=torch.int64, device="cuda")
    rows = [n_rows - 1, 0, 0x5A5A5A5 % n_rows]
    tag = lambda kind, index: [kind, index, index >> 5, 0x7777]
    level_idx = sorted({i for r in rows for i in [r] + C.path_indices(n_rows, r)})
    # byte offsets: the levels pass 2^32, the last row of the column is the last felt below it (past a signed 2^31)
    assert max(level_idx) * 32 > 1 << 32 and (1 << 31) < max(rows) * 32 == (1 << 32) - 32
    col[0, torch.tensor(rows, device="cuda")] = torch.tensor([tag(C.VALUE_TAG, r) for r in rows], device="cuda")
    levels[torch.tensor(level_idx, device="cuda")] = torch.tensor([tag(C.LEVEL_TAG, i) for i in level_idx], device="cuda")
    torch.cuda.synchronize()
    try:
        values, val_off, leaves, siblings, off, _ = open_arrays(lib, [(col, levels)], [(0, r) for r in rows])
    finally:
        del col, levels
        torch.cuda.empty_cache()  # 12 GiB go back to the device for the tests that follow
    assert list(val_off) == [0, 1, 2, 3] and list(off) == [0, 27, 54, 81]
    assert values.tolist() == [tag(C.VALUE_TAG, r) for r in rows]
    assert leaves.tolist() == [tag(C.LEVEL_TAG, r) for r in rows]
    assert siblings.tolist() == [tag(C.LEVEL_TAG, i) for r in rows for i in C.path_indices(n_rows, r)]


# ---- 4. proof identity ----------------------------------------------------------------------------------------------
def c_hash(a, b):
    from oracle import cref
    return cref.pedersen_hash_many([a], [b])[0][0]


def test_prove_equals_the_slice_by_slice_assembly(gpu):
    from oracle import stark_ref as S
    from starkperp import stark
    torch, lib = gpu
    rng = random.Random(17)
    inputs = [(rng.randrange(S.P), rng.randrange(S.P)) for _ in range(2)]
    xs = stark.felts_to_tensor([a for a, _ in inputs])
    ys = stark.felts_to_tensor([b for _, b in inputs])
    state = stark._commit_trace(stark.pedersen_trace(xs, ys), "pedersen", 7, 6, stark.FIELD_GEN, ())
    torch.cuda.synchronize()
    proof, launches, units = profiled(lib, lambda: stark._query_trace(state, 3))
    n_layers = len(proof["layer_roots"])
    assert proof["n"] == 1024 and (launches, units) == (1, 3 * (4 + 2 * n_layers))  # the whole query phase: one launch
    assert proof == stark._query_trace(state, 3, stark._open_by_slices)
    assert proof == stark.prove(xs, ys, n_queries=3, seed=7)
    assert proof == stark._query_trace(state, 3, lambda t, p: stark.open_rows(t, p, host_call=True))
    ok, why = S.verify_proof(proof)
    assert ok, why
    checks = stark.check_merkle_openings(proof)
    assert len(checks) == units and all(good for _, good in checks)


def test_prove_builtins_equals_the_slice_by_slice_assembly(gpu):
    from oracle import ref_py as R
    from oracle import stark_ref as S
    from starkperp import batch, stark
    torch, lib = gpu
    rng = random.Random(18)
    hashes = [(rng.randrange(S.P), rng.randrange(S.P)) for _ in range(2)]
    key, z = rng.randrange(1, R.EC_ORDER), rng.randrange(1, 2**251)
    (r, s), q = batch.sign_many([z], [key])[0], batch.public_keys_many([key])[0]
    values = [sum(rng.randrange(300, 420) << (16 * k) for k in range(8)) for _ in range(16)]
    state = stark._commit_builtins(hashes, [(z, r, s, q)], values, 1, 6, stark.FIELD_GEN, None)
    torch.cuda.synchronize()
    proof, launches, units = profiled(lib, lambda: stark._query_builtins(state, 2))
    n_layers = len(proof["layer_roots"])
    assert proof["segments"] == ["pedersen", "ecdsa", "rc16"] and proof["n"] == 1024
    assert (launches, units) == (1, 2 * (8 + 2 * n_layers))
    assert proof == stark._query_builtins(state, 2, stark._open_by_slices)
    assert proof == stark.prove_builtins(hashes, [(z, r, s, q)], values, n_queries=2, seed=1)
    ok, why = S.verify_builtins_proof(proof, hash2=c_hash)
    assert ok, why


# ---- 5. a plain-C consumer --------------------------------------------------------------------------------------------
def test_c_consumer_opens_and_verifies(gpu):
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_open")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_open.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-ldl", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "cabi_open ok" in out.stdout
