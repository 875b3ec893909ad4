"""The index and plan logic of the opening call (csrc/commit_open.hpp: validation, base_l, the sibling index, the two
offset arrays, the slice plan, the gather of one opening) on the host, no GPU: g++ builds
tests/host/commit_open_shim.cpp, which replays the kernel's launch plan lane by lane over host arrays of tags; the
expected arrays are NumPy indexing (tests/commit_open_cases.py).  Also the stand-alone form of the shim under
-fsanitize=address,undefined, run directly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import commit_open_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "commit_open_shim.cpp")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "commit_open_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.co_slice_max.restype = lib.co_slice_count.restype = ctypes.c_size_t
    lib.co_slice_count.argtypes = [ctypes.c_size_t]
    lib.co_slice.restype = None
    lib.co_slice.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.co_blocks.restype = ctypes.c_uint
    lib.co_blocks.argtypes = [ctypes.c_size_t]
    lib.co_level_base.restype = lib.co_sibling_index.restype = ctypes.c_uint64
    lib.co_level_base.argtypes = [ctypes.c_uint64, ctypes.c_uint]
    lib.co_sibling_index.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint]
    lib.co_size.restype = lib.co_open.restype = ctypes.c_int
    lib.co_size.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4 + [
        ctypes.c_size_t]
    lib.co_open.argtypes = [ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 9 + [
        ctypes.c_size_t]
    return lib


def c_sizes(vals):
    return (ctypes.c_size_t * max(len(vals), 1))(*vals)


def c_ptrs(vals):
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


def call_open(shim, a, out):
    """co_open on an argument dict of commit_open_cases (base_args / a Case's): (rc, launches, error text)."""
    err = ctypes.create_string_buffer(128)
    launches = ctypes.c_uint64(0)
    ptr = lambda name: None if name in a["null"] else getattr(out, name).ctypes.data
    rc = shim.co_open(a["n_tables"], c_ptrs(a["cols"]), c_sizes(a["col_stride"]), c_sizes(a["n_rows"]),
                      c_sizes(a["n_cols"]), c_ptrs(a["levels"]), a["n_open"], a["table_of"].ctypes.data,
                      a["rows"].ctypes.data, ptr("values"), ptr("val_off"), ptr("leaves"), ptr("siblings"), ptr("off"),
                      ctypes.byref(launches), err, 128)
    return rc, launches.value, err.value.decode()


def case_args(case):
    return {"n_tables": len(case.tables), "cols": [c.ctypes.data for c, _ in case.arrays],
            "levels": [lv.ctypes.data for _, lv in case.arrays], "col_stride": [s for _, _, s in case.tables],
            "n_rows": [r for r, _, _ in case.tables], "n_cols": [c for _, c, _ in case.tables], "n_open": case.n_open,
            "table_of": case.table_of, "rows": case.rows, "null": set()}


def test_slice_plan_and_closed_forms(shim):
    S = shim.co_slice_max()
    assert S == C.SLICE_MAX
    for n in (0, 1, S - 1, S, S + 1, 3 * S, 3 * S + 5):
        k = shim.co_slice_count(n)
        assert k == C.slices_of(n)
        at = 0
        for j in range(k):
            first, count = ctypes.c_size_t(), ctypes.c_size_t()
            shim.co_slice(n, j, ctypes.byref(first), ctypes.byref(count))
            assert first.value == at and 1 <= count.value <= S
            at += count.value
        assert at == n
    assert [shim.co_blocks(c) for c in (1, 4, 5, S)] == [1, 1, 2, S // 4]
    # base_l is the running offset of _path_indices, the sibling index its entry - up to tables of 2^32 rows
    for n_rows in (1, 2, 4, 64, 128, 1 << 26, 1 << 32):
        at, width, level = 0, n_rows, 0
        while width >= 1:
            assert shim.co_level_base(n_rows, level) == at
            at, width, level = at + width, width >> 1, level + 1
        for r in {0, n_rows - 1, n_rows // 2, n_rows // 3}:
            want = C.path_indices(n_rows, r)
            assert [shim.co_sibling_index(n_rows, r, l) for l in range(len(want))] == want


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c.name)
def test_case_against_numpy(shim, case):
    values, val_off, leaves, siblings, off = case.expected()
    # the totals from the shapes alone
    nv, ns = ctypes.c_size_t(99), ctypes.c_size_t(99)
    err = ctypes.create_string_buffer(128)
    rc = shim.co_size(len(case.tables), c_sizes([r for r, _, _ in case.tables]), c_sizes([c for _, c, _ in case.tables]),
                      case.n_open, case.table_of.ctypes.data, ctypes.byref(nv), ctypes.byref(ns), err, 128)
    assert (rc, nv.value, ns.value) == (C.SP_OK, len(values), len(siblings)), err.value
    for want_leaves in (True, False):
        out = C.Outputs(case.n_open, len(values) + 2, len(siblings) + 2)
        a = case_args(case)
        if not want_leaves:
            a["null"].add("leaves")
        rc, launches, text = call_open(shim, a, out)
        assert rc == C.SP_OK, text
        assert launches == C.slices_of(case.n_open)
        assert np.array_equal(out.val_off, val_off) and np.array_equal(out.off, off)
        assert np.array_equal(out.values[: len(values)], values)
        assert np.array_equal(out.siblings[: len(siblings)], siblings)
        if want_leaves:
            assert np.array_equal(out.leaves[: case.n_open], leaves)
        else:
            assert C.all_sentinel(out.leaves)
        # nothing past the totals is written, and no padding row was read (a pad tag in an output)
        assert C.all_sentinel(out.values[len(values):]) and C.all_sentinel(out.siblings[len(siblings):])
        assert not np.isin(out.values[:, 0], [C.PAD_TAG + t for t in range(len(case.tables))]).any()


@pytest.mark.parametrize("bad", C.BAD, ids=lambda b: b[0])
def test_bad_argument_is_refused_before_anything_is_written(shim, bad):
    name, patch, word = bad
    arrays = [C.table_arrays(t, *shape) for t, shape in enumerate(C.BASE_TABLES)]
    good = C.base_args([c.ctypes.data for c, _ in arrays], [lv.ctypes.data for _, lv in arrays])
    out = C.Outputs(len(C.BASE_PICKS), 16, 16)
    rc, _, text = call_open(shim, good, out)
    assert rc == C.SP_OK, text  # the base call is good: what follows fails for the patched argument alone
    a = C.base_args([c.ctypes.data for c, _ in arrays], [lv.ctypes.data for _, lv in arrays])
    patch(a)
    out = C.Outputs(len(C.BASE_PICKS), 16, 16)
    rc, _, text = call_open(shim, a, out)
    assert rc == C.SP_ERR_BAD_ARGUMENT
    assert word in text, text
    assert out.untouched()


def test_size_call_refuses_bad_shapes(shim):
    err = ctypes.create_string_buffer(128)
    nv, ns = ctypes.c_size_t(7), ctypes.c_size_t(7)
    one = np.zeros(1, dtype=np.uint32)
    for n_rows, n_cols, n_tables, table, word in ((3, 1, 1, 0, "n_rows"), (4, 0, 1, 0, "n_cols"), (4, 1, 0, 0, "n_tables"),
                                                  (4, 1, 1, 1, "table_of")):
        one[0] = table
        rc = shim.co_size(n_tables, c_sizes([n_rows]), c_sizes([n_cols]), 1, one.ctypes.data, ctypes.byref(nv),
                          ctypes.byref(ns), err, 128)
        assert rc == C.SP_ERR_BAD_ARGUMENT and word in err.value.decode()
        assert (nv.value, ns.value) == (7, 7)


def test_standalone_program_under_sanitizers(tmp_path):
    """The same shim source with its own main, built with AddressSanitizer + UndefinedBehaviorSanitizer and run
    directly: exactly-sized tables, every row of every table, two slices, refused calls."""
    exe = str(tmp_path / "commit_open_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DCOMMIT_OPEN_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    assert "commit_open check passed" in run.stdout
