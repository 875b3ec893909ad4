"""GPU parity of the Merkle path calls (sp_merkle_fold_paths[_dev], sp_merkle_verify_paths, the path form of
ped_fold_ragged_kernel and its per-step fallback) against the C oracle: size classes and slice edges, side bits, ragged lengths inside one block,
the sp_tree_prove round trip, per-item verdicts and status, bad arguments, the fallback switches in a child process,
both window plans, the prover's Merkle openings and a plain-C consumer."""
import copy
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import merkle_path_cases as cases
from test_gpu_window_plans import window_bits  # noqa: F401  (the fixture that re-initialises under 21 and 26 bits)
from witness_replay import oracle_hash, oracle_hash_many

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = cases.P
BAD_ARGUMENT = -3


@pytest.fixture(scope="module")
def batch_np():
    from starkperp import batch_np as b
    return b


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def fold_dev(leaves, sib, off, height, keys, with_status=True):
    """sp_merkle_fold_paths_dev on a side stream with torch tensors; the host arrays are scribbled over as soon as
    the call returns."""
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    n = leaves.shape[0]
    side = torch.cuda.Stream()
    d_leaves = torch.from_numpy(leaves.view(np.int64)).cuda()
    d_sib = torch.from_numpy(np.ascontiguousarray(sib).view(np.int64).reshape(-1, 4)).cuda()
    if d_sib.shape[0] == 0:
        d_sib = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    d_roots = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host_keys = keys.copy()
    host_off = None if off is None else off.copy()
    with torch.cuda.stream(side):
        _lib.check(lib.sp_merkle_fold_paths_dev(d_leaves.data_ptr(), d_sib.data_ptr(),
                                                None if off is None else ptr(host_off), height, ptr(host_keys), n,
                                                d_roots.data_ptr(), d_st.data_ptr() if with_status else None,
                                                side.cuda_stream), "sp_merkle_fold_paths_dev")
        host_keys[:] = 0xFFFFFFFFFFFFFFFF  # keys and offsets were copied before the call returned
        if host_off is not None:
            host_off[:] = 0
    side.synchronize()
    return d_roots.cpu().numpy().view(np.uint64), d_st.cpu().numpy()


# ---- 1. size classes and slice edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 65, 2048, 2049, 4096, 4097, 8192, 8193])
def test_size_classes_and_slice_edges(batch_np, n):
    pool = cases.pool(3)
    want31 = batch_np.felts_from_ints(cases.oracle_roots(pool))
    leaves31, sib31, _, keys31 = cases.arrays(pool)
    idx = np.arange(n) % cases.POOL
    leaves, sib, keys = leaves31[idx], sib31.reshape(cases.POOL, 3, 4)[idx], keys31[idx]
    want = want31[idx]
    roots, st = batch_np.merkle_fold_paths(leaves, sib, keys, height=3)
    assert not st.any() and (roots == want).all(), np.flatnonzero((roots != want).any(axis=1))[:8]
    verdict, st = batch_np.merkle_verify_paths(leaves, sib, keys, want, height=3)
    assert verdict.all() and not st.any()
    roots, st = fold_dev(leaves, sib, None, 3, keys)
    assert not st.any() and (roots == want).all(), np.flatnonzero((roots != want).any(axis=1))[:8]
    # the ragged form of the same batch
    roots, st = fold_dev(leaves, sib, batch_np.uniform_path_offsets(n, 3), 0, keys, with_status=False)
    assert (roots == want).all() and (st == 0xEE).all()


# ---- 2. side bits --------------------------------------------------------------------------------------------------
def test_side_bits(batch_np):
    rng = random.Random(64)
    keys = [0, 2**64 - 1, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 1, 2**63] + [rng.randrange(2**64) for _ in range(27)]
    items = [(k, rng.randrange(P), [rng.randrange(P) for _ in range(64)]) for k in keys]
    assert len(items) == 33
    cases.check_batch(batch_np, items)
    leaves, sib, off, key_arr = cases.arrays(items)
    roots, st = batch_np.merkle_fold_paths(leaves, sib.reshape(33, 64, 4), key_arr, height=64)
    assert not st.any() and batch_np.ints_from_felts(roots) == cases.oracle_roots(items)
    # a swapped side changes every one of these roots: the all-left and the all-right fold of one path differ
    same = [(0, items[0][1], items[0][2]), (2**64 - 1, items[0][1], items[0][2])]
    a, b = cases.oracle_roots(same)
    assert a != b
    low = [(0, 11, [22]), (1, 11, [22])]
    assert cases.oracle_roots(low) == [oracle_hash(11, 22), oracle_hash(22, 11)]
    cases.check_batch(batch_np, low)


def test_list_api_and_proof_roots_many(batch_np):
    from starkperp import batch, state
    items = cases.batch_of(cases.ragged_lengths(40))
    want = cases.oracle_roots(items)
    keys, proofs = [k for k, _, _ in items], [(leaf, s) for _, leaf, s in items]
    assert batch.merkle_fold_paths(keys, proofs) == want
    assert state.proof_roots_many(keys, proofs) == want


# ---- 3. ragged lengths in one block --------------------------------------------------------------------------------
def test_ragged_lengths_in_one_block(batch_np):
    cases.check_batch(batch_np, cases.batch_of(cases.ragged_lengths(300)))
    cases.check_batch(batch_np, cases.batch_of([0] * 300))  # root = leaf
    cases.check_batch(batch_np, cases.batch_of([0] * 150 + [64] + [0] * 149))
    items = cases.batch_of(cases.ragged_lengths(300))
    leaves, sib, off, keys = cases.arrays(items)
    roots, st = fold_dev(leaves, sib, off, 0, keys)
    assert not st.any() and batch_np.ints_from_felts(roots) == cases.oracle_roots(items)


# ---- 4. sp_tree_prove round trip -----------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [64, 1, 3, 16])
def test_tree_prove_round_trip(batch_np, height):
    from starkperp import state
    rng = random.Random(400 + height)
    size = 1 << height
    written = rng.sample(range(size), min(300, size)) if height <= 16 else [rng.randrange(size) for _ in range(300)]
    leaves = {k: rng.randrange(1, P) for k in written}
    tree = state.LibrarySparseTree(height)
    twin = state.SparseMerkleTree(height, 0, hash_many=oracle_hash_many)
    tree.update(leaves)
    twin.update(leaves)
    assert tree.root == twin.root
    known = sorted(leaves)
    touched = known[:5]
    keys = touched + [rng.choice(known) for _ in range(195)]  # repeats included
    fresh = [k for k in (rng.randrange(size) for _ in range(50)) if k not in leaves]
    keys += fresh + fresh[:3]
    proofs = tree.prove(keys)
    assert tree.verify(keys, proofs) == [True] * len(keys)
    assert state.proof_roots_many(keys, proofs) == [twin.root] * len(keys)
    # sp_tree_prove's arrays are sp_merkle_verify_paths' arguments as they come
    karr = np.array(keys, dtype=np.uint64)
    lv, sib = batch_np.tree_prove(tree, karr)
    verdict, st = batch_np.merkle_verify_paths(lv, sib, karr, batch_np.felts_from_ints([twin.root]), height=height)
    assert verdict.all() and not st.any()
    # one more update: the old proofs of the touched keys no longer verify against the new root
    tree.update({k: leaves[k] ^ 1 for k in touched})
    verdicts = tree.verify(keys, proofs)
    assert not any(verdicts[:len(touched)]) and all(not v for k, v in zip(keys, verdicts) if k in touched)
    assert tree.verify(touched, tree.prove(touched)) == [True] * len(touched)
    old = [(leaves[k], p[1]) for k, p in zip(touched, tree.prove(touched))]
    assert tree.verify(touched, old) == [False] * len(touched)
    # malformed proofs are False, not an error
    leaf, sibs = tree.prove(touched[:1])[0]
    assert tree.verify([touched[0]] * 3 + [size], [(leaf, sibs[:-1]), (P, sibs), (leaf, sibs), (leaf, sibs)]) == \
        [False, False, True, False]
    tree.close()


# ---- 5. verdicts and status are per item ---------------------------------------------------------------------------
@pytest.mark.parametrize("shared_root", [True, False], ids=["one_root", "per_item_roots"])
def test_verdicts_and_status_are_per_item(batch_np, shared_root):
    cases.check_verdict_case(batch_np, shared_root)


# ---- 6. bad arguments write nothing --------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(batch_np):
    from starkperp import _lib
    lib = _lib.ensure_init()
    items = cases.batch_of([2, 0, 5])
    leaves, sib, off, keys = cases.arrays(items)
    expected = batch_np.felts_from_ints(cases.oracle_roots(items))
    PAT = 0xA5A5A5A5A5A5A5A5
    roots = np.full((3, 4), PAT, dtype=np.uint64)
    verdict = np.full(3, 0xEE, dtype=np.uint8)
    st = np.full(3, 0xEE, dtype=np.uint8)
    u32 = lambda v: np.array(v, dtype=np.uint32)
    u64 = lambda v: np.array(v, dtype=np.uint64)
    wide = np.zeros((3 * 65, 4), dtype=np.uint64)
    # (off, height, keys, n, n_expected)
    bad = {
        "off[0] != 0": (u32([1, 2, 2, 7]), 0, keys, 3, 3),
        "a decreasing offset": (u32([0, 2, 1, 7]), 0, keys, 3, 3),
        "a path longer than 64": (u32([0, 65, 65, 70]), 0, u64([0, 0, 0]), 3, 3),
        "height > 64": (None, 65, u64([0, 0, 0]), 3, 3),
        "key bit at its path's length": (off, 0, u64([4, 0, 0]), 3, 3),
        "key bit in a path of no siblings": (off, 0, u64([0, 1, 0]), 3, 3),
        "key bit above a uniform height": (None, 2, u64([0, 0, 1 << 63]), 3, 3),
        "more than 2^32 - 1 sibling felts": (None, 64, keys, (1 << 26) + 1, (1 << 26) + 1),
    }
    for name, (o, height, k, n, n_exp) in bad.items():
        o_ptr = None if o is None else ptr(o)
        s = wide if name.startswith("a path longer") else sib
        assert lib.sp_merkle_fold_paths(ptr(leaves), ptr(s), o_ptr, height, ptr(k), n, ptr(roots), ptr(st)) == BAD_ARGUMENT, name
        assert b"merkle paths" in lib.sp_last_error(), name
        assert lib.sp_merkle_verify_paths(ptr(leaves), ptr(s), o_ptr, height, ptr(k), n, ptr(expected), n_exp, ptr(verdict),
                                          ptr(st)) == BAD_ARGUMENT, name
        assert len(lib.sp_last_error()) > 0, name
        assert (roots == PAT).all() and (verdict == 0xEE).all() and (st == 0xEE).all(), name
    for n_exp in (0, 2, 4):
        assert lib.sp_merkle_verify_paths(ptr(leaves), ptr(sib), ptr(off), 0, ptr(keys), 3, ptr(expected), n_exp,
                                          ptr(verdict), ptr(st)) == BAD_ARGUMENT
        assert b"n_expected" in lib.sp_last_error()
        assert (verdict == 0xEE).all() and (st == 0xEE).all()
    # the _dev call validates the same way, before anything is enqueued
    import torch
    d_leaves = torch.from_numpy(leaves.view(np.int64)).cuda()
    d_sib = torch.from_numpy(sib.view(np.int64)).cuda()
    d_roots = torch.full((3, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_st = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for name in ("off[0] != 0", "a decreasing offset", "height > 64", "key bit at its path's length"):
        o, height, k, n, _ = bad[name]
        assert lib.sp_merkle_fold_paths_dev(d_leaves.data_ptr(), d_sib.data_ptr(), None if o is None else ptr(o), height,
                                            ptr(k), n, d_roots.data_ptr(), d_st.data_ptr(), stream) == BAD_ARGUMENT, name
        assert len(lib.sp_last_error()) > 0
    torch.cuda.synchronize()
    assert (d_roots.cpu().numpy() == 0x5A5A5A5A).all() and (d_st.cpu().numpy() == 0xEE).all()
    # n == 0 is SP_OK and writes nothing
    assert lib.sp_merkle_fold_paths(None, None, None, 64, None, 0, None, None) == 0
    assert lib.sp_merkle_verify_paths(None, None, None, 64, None, 0, None, 1, None, None) == 0
    assert lib.sp_merkle_fold_paths_dev(None, None, None, 64, None, 0, None, None, None) == 0
    assert lib.sp_merkle_fold_paths(ptr(leaves), ptr(sib), ptr(off), 0, ptr(keys), 0, ptr(roots), ptr(st)) == 0
    assert (roots == PAT).all() and (st == 0xEE).all()
    # and the good call still works afterwards
    assert lib.sp_merkle_fold_paths(ptr(leaves), ptr(sib), ptr(off), 0, ptr(keys), 3, ptr(roots), None) == 0
    assert (roots == expected).all()


# ---- 7. the fallback in a fresh child process ----------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["STARKPERP_NO_QUAD", "STARKPERP_NO_CHAIN_RAGGED", "STARKPERP_NO_PATH_FOLD"])
def test_fallback_in_a_child_process(switch):
    """No fused kernel (the quad kernels switched off, the switch of the ragged launches, the switch of this launch):
    one gathered launch per level over the paths still running, the index pair swapped where the side bit is set; 300
    ragged paths and the verdict case against the oracle, in a fresh interpreter."""
    env = dict(os.environ)
    env[switch] = "1"
    done = subprocess.run([sys.executable, os.path.join(HERE, "merkle_path_cases.py")], env=env, timeout=120,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "merkle_paths child ok" in done.stdout, done.stdout[-2000:]


# ---- 8. window plans -----------------------------------------------------------------------------------------------
def test_ragged_batch_under_both_window_plans(window_bits, batch_np):  # noqa: F811
    cases.check_batch(batch_np, cases.batch_of(cases.ragged_lengths(300)))


# ---- 9. the prover's Merkle openings -------------------------------------------------------------------------------
def test_prover_openings():
    from oracle import stark_ref as S
    from starkperp import stark
    rng = random.Random(21)  # the inputs of test_gpu_stark.test_prove_then_verify_small
    inputs = [(rng.randrange(P), rng.randrange(P)) for _ in range(2)]
    xs = stark.felts_to_tensor([a for a, _ in inputs])
    ys = stark.felts_to_tensor([b for _, b in inputs])
    proof = stark.prove(xs, ys, n_queries=3, seed=7)
    ok, why = S.verify_proof(proof, hash2=oracle_hash)
    assert ok, why
    got = stark.check_merkle_openings(proof)
    n_layers = len(proof["layer_roots"])
    assert len(got) == 3 * (4 + 2 * n_layers) and len({label for label, _ in got}) == len(got)
    assert all(v for _, v in got), [label for label, v in got if not v]
    q0, q2 = proof["queries"][0], proof["queries"][2]
    assert got[0][0] == "q0/trace/row %d" % q0["trace"][0]["row"]
    assert got[4][0] == "q0/layer 0/pos %d" % q0["layers"][0][0]["pos"]
    bad = copy.deepcopy(proof)
    bad["queries"][2]["layers"][3][1]["path"][2] ^= 1
    bad["queries"][1]["trace"][2]["values"][3] ^= 1
    want_false = {"q2/layer 3/pos %d" % q2["layers"][3][1]["pos"], "q1/trace/row %d" % proof["queries"][1]["trace"][2]["row"]}
    got_bad = stark.check_merkle_openings(bad)
    assert [label for label, _ in got_bad] == [label for label, _ in got]
    assert {label for label, v in got_bad if not v} == want_false
    assert not S.verify_proof(bad, hash2=oracle_hash)[0]
    # a value that is no field element fails its own opening only
    bad = copy.deepcopy(proof)
    bad["queries"][0]["layers"][1][0]["value"] = P
    bad["queries"][0]["trace"][1]["values"][0] = 2**256
    assert [i for i, (_, v) in enumerate(stark.check_merkle_openings(bad)) if not v] == [1, 6]


# ---- 10. a plain-C consumer ----------------------------------------------------------------------------------------
def test_c_consumer_of_the_path_calls_runs():
    libdir = os.path.join(ROOT, "stark-perpetual_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cabi", "cabi_paths")
    subprocess.check_call(["gcc", "-O1", os.path.join(ROOT, "tests", "cabi", "cabi_paths.c"), "-o", exe,
                           "-L" + libdir, "-lstarkperp", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "cabi_paths ok" in out.stdout
