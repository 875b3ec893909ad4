"""GPU parity of every launch plan of the Pedersen dispatcher (enqueue_pedersen_impl and, in front of it,
ped_top_kernel in sp_merkle_forest_dev): results AND per-item status at every size-class edge, through
sp_pedersen_batch itself - below the Python-side range assertion of starkperp.batch / batch_np, which keeps an
out-of-range operand from ever reaching a kernel.  Inputs, expectations and the size tables with the plan each size
takes: tests/pedersen_plan_cases.py (checked against the oracle without a GPU by tests/test_pedersen_plan_cases_cpu.py).
All comparisons are exact; `out` of a flagged row is unspecified (include/starkperp.h) and not compared."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pedersen_plan_cases as cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    from starkperp import _lib
    return _lib.ensure_init()


# ---- 1. results and per-item status of a direct batch ----
@pytest.mark.parametrize("n", cases.SMALL)
def test_small_batches(lib, n):
    """Quad kernels (8, 4, 2 quads per hash) and the fused lane-split kernels (4, 2, 1 lanes), both sides of every
    threshold."""
    cases.check_batch(lib, n)


@pytest.mark.parametrize("n", cases.MIXED)
def test_mixed_batches(lib, n):
    """One round of the bulk body plus a remainder: the three remainder lane counts of ped_accumulate_mixed_kernel, a
    remainder of one hash, and the plain bulk kernel with a ragged and with a whole last round."""
    cases.check_batch(lib, n)


@pytest.mark.parametrize("n", cases.LARGE)
def test_large_batches(lib, n):
    """The three finish kernels at the sizes where one takes over from the other (8 | 9 and 16 | 17 elements per
    thread) and the cap of 32 elements per thread."""
    cases.check_batch(lib, n)


# one size per class: 8 / 4 / 2 quads, 4 / 2 / 1 lanes fused, mixed with 8 / 4 / 2 lanes, bulk ragged, bulk whole
@pytest.mark.parametrize("n", [3, 4096, 8192, 16384, 32768, 65535, 65537, 81920, 98304, 131071, 131072])
def test_batch_np_raises_for_a_row_the_device_flagged(n):
    from starkperp import batch_np
    x, y, expected = cases.inputs(n, seed=n + 1)
    assert (batch_np.pedersen_hash_many(x, y) == expected).all()
    xi, yi, _, _ = cases.inject(n, x, y, expected)
    with pytest.raises(AssertionError):
        batch_np.pedersen_hash_many(xi, yi)


# ---- 2. forests ----
def run_forest(lib, leaves, n_trees, height):
    """sp_merkle_forest_dev on a torch buffer, on the current stream.  Returns (every node uint64[rows, 4], status byte)."""
    import torch
    from starkperp import _lib
    _, rows = cases.forest_offsets(n_trees, height)
    buf = torch.zeros((rows, 4), dtype=torch.int64, device="cuda")
    buf[: leaves.shape[0]] = torch.from_numpy(np.array(leaves).view(np.int64)).cuda()  # a writable copy
    status = (ctypes.c_uint8 * 1)(0xEE)
    _lib.check(lib.sp_merkle_forest_dev(buf.data_ptr(), n_trees, height, status,
                                        torch.cuda.current_stream().cuda_stream), "sp_merkle_forest_dev")
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint64), status[0]


def wrong_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1))


@pytest.mark.parametrize("n_trees,height", cases.FOREST_SHAPES)
def test_forest_every_node(lib, n_trees, height):
    leaves, want = cases.forest(n_trees, height)
    got, status = run_forest(lib, leaves, n_trees, height)
    assert status == 0
    bad = wrong_rows(got, want)
    assert bad.size == 0, "%d wrong nodes, first rows %s (level offsets %s)" % (
        bad.size, bad[:8].tolist(), cases.forest_offsets(n_trees, height)[0])


@pytest.mark.parametrize("n_trees,height,tree,leaf", cases.FOREST_BAD_LEAF)
def test_forest_status_byte_and_its_reset(lib, n_trees, height, tree, leaf):
    """One leaf = p: the status byte says so, every node that is not above that leaf is still the oracle's (the bad
    leaf's own path is unspecified), and a clean call on the same stream straight afterwards reports 0 again."""
    leaves, want = cases.forest(n_trees, height)
    spoiled = leaves.copy()
    spoiled[(tree << height) + leaf] = cases.felts_from_ints([cases.P])[0]
    got, status = run_forest(lib, spoiled, n_trees, height)
    assert status == cases.HASH_OUT_OF_RANGE
    path = cases.path_rows(n_trees, height, tree, leaf)
    offs, rows = cases.forest_offsets(n_trees, height)
    keep = np.ones(rows, dtype=bool)
    keep[path] = False
    keep[(tree << height) + leaf] = False  # the leaf itself stays as given
    assert (got[(tree << height) + leaf] == spoiled[(tree << height) + leaf]).all()
    bad = wrong_rows(got[keep], want[keep])
    assert bad.size == 0, "%d nodes off the bad leaf's path are wrong" % bad.size
    roots = [t for t in range(n_trees) if t != tree]
    assert (got[offs[height] + np.array(roots)] == want[offs[height] + np.array(roots)]).all()
    got, status = run_forest(lib, leaves, n_trees, height)
    assert status == 0
    assert wrong_rows(got, want).size == 0


# ---- 3. plans only the A/B switches reach, in fresh child processes ----
SWITCHES = {
    # no quad kernels, no fused inversion: ped_accumulate_split_kernel<3 | 2 | 1, false> and ped_finish_kernel with 64
    # and with 256 threads per block, one element per thread
    "no_quad_no_fuse": {"STARKPERP_NO_QUAD": "1", "STARKPERP_NO_FUSE": "1"},
    # a level is never cut into bulk + remainder, the finish kernel keeps its prefix products in HBM
    "no_level_split_no_finish_lds": {"STARKPERP_NO_LEVEL_SPLIT": "1", "STARKPERP_NO_FINISH_LDS": "1"},
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_only_plans_in_a_child_process(name):
    """The size ladder of pedersen_plan_cases.main (results and injected status, 1 .. 70 000 hashes) under the A/B
    switches the project's measurements compare against, with 16-bit windows (tables of 0.2 GiB, built in the child)."""
    env = dict(os.environ, STARKPERP_WINDOW_BITS="16", **SWITCHES[name])
    done = subprocess.run([sys.executable, os.path.join(HERE, "pedersen_plan_cases.py")], env=env, timeout=300,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "pedersen_plan child ok" in done.stdout, done.stdout[-2000:]
