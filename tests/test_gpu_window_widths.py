"""Parity at every window width sp_init accepts, 4 .. 27 bits (tests/window_width_cases.py; proven without a GPU by
tests/test_window_width_cases_cpu.py).  The width fixes the Pedersen window plan (18 .. 101 windows, window 0 of 1 .. 28
bits) and the EC_GEN table (4 .. 22 bits, 12 .. 63 windows, the top one partial unless the width divides 252); every
hash kernel receives w0, log2e and nwin at run time and cuts its windows out of x || y with code of its own (pop_bits,
window_from_memory, gen_mul_gathered), and the host dispatcher changes shape with nwin.  One module-scoped fixture per
width: sp_shutdown, sp_init(0, width), the tests, and back to the environment's plan.  Everything expected is independent
of the width except the crafted operand pairs (one oracle call of about 400 hashes per width) and the generator scalars;
all of it is cached at module level, so the oracle runs once per session.  Every comparison is exact.

What a width changes, read from the dispatcher (pedersen.hip), not traced:
  4, 5, 6      nwin = 101, 84, 72 > 64: quad_class_max is 0 for every class, enqueue_pedersen_top declines ped_tail_kernel
               and ped_top_kernel, the chain and path fusions decline - EVERY size here, every forest level, chain step and
               tree level runs the lane-split kernels (ped_accumulate_split_kernel<3 | 2 | 1 | 0, fused>), the bulk body
               or the mixed kernel, one level at a time.  The nodes must be the same all the same.
  7 .. 14      33 <= nwin <= 63: the quad kernels with their further-window loop (from a quad's fifth window)
  15 .. 27     nwin <= 32: at most four windows per quad with eight quads
  5, 6, 8, 11, 13, 17, 20, 27   no window straddles string bit 252 (constant_window_counts, ped_partial_kernel and the
               SPARSE forms of ped_quad_kernel / ped_path_kernel see whole windows on both sides)
  27           window 0 is 28 bits wide; nwin = 18, two above the least the quad, top and tail kernels take
  23 .. 27     the EC_GEN table is the 22-bit one: the generator walk is tested at 4 .. 22 only

Widths above 22 need 14 .. 155 GiB of tables and are skipped when the device has less free memory than the plan's
sp_table_bytes plus an eighth.

REDUCED widths: inside this suite sp_init takes 0.02 .. 0.04 s up to 23 bits (0.03 s at the default, 21) and 1.1, 1.8, 2.4
and 3.7 s at 24, 25, 26 and 27 (profiles/window_widths.txt) - more than ten times the default width's in the same run,
the bound the work on this file set itself for a width's share of the suite.  Those four run the crafted batch, one
forest shape with its bad-leaf case and the height-3 tree only (their EC_GEN table is the 22-bit one); the other tests
skip there with that reason.  26 bits has its full parity in tests/test_gpu_window_plans.py."""
import functools
import random
import time

import numpy as np
import pytest

import chains_ragged_cases as CR
import ec_point_cases as E
import pedersen_plan_cases as PC
import sign_cases as SC
import test_gpu_tail_fusion as TF
import window_width_cases as W

pytestmark = pytest.mark.gpu

P, N = W.P, W.N
TILED_SIZES = (1500, 3000, 6000, 12000, 24000, 50000, 65536 + 5000, 65536 + 40000)  # one inside every class of SMALL / MIXED
PLAN_FORESTS = ((3, 5), (5, 10), (5, 13), (17, 13))   # pedersen_plan_cases.FOREST_SHAPES
TAIL_FORESTS = ((1, 13), (20, 13))                    # test_gpu_tail_fusion.SHAPES
SMALL_TREE_SIZES = (1, 3, 8, 5)                       # updates of the height-3 tree
EMPTY_LEAVES = (0, 0x1234567890ABCDEF1234567890ABCDEF)
INIT_SECONDS = {}
REDUCED = (24, 25, 26, 27)                                   # see the docstring
REDUCED_FOREST = (17, 13)


def full_only(width):
    if width in REDUCED:
        pytest.skip("reduced width: sp_init takes more than ten times the default width's (profiles/window_widths.txt)")


def margin(need):
    return max(need // 8, 2 << 30)


@pytest.fixture(scope="module", params=list(W.WIDTHS), ids=["w%d" % w for w in W.WIDTHS])
def width(request):
    import torch
    from starkperp import _lib
    w = request.param
    lib = _lib.load()
    torch.cuda.synchronize()
    if w > 22:
        torch.cuda.empty_cache()
        free, _total = torch.cuda.mem_get_info(0)
        have = lib.sp_table_bytes() if lib.sp_is_initialised() else 0
        need = W.table_bytes(w)
        if free + have < need + margin(need):
            pytest.skip("%d-bit tables need %.0f GiB of HBM; %.0f GiB free" % (w, need / 2**30, (free + have) / 2**30))
    lib.sp_shutdown()
    t0 = time.perf_counter()
    _lib.check(lib.sp_init(0, w), "sp_init")
    INIT_SECONDS[w] = time.perf_counter() - t0
    assert lib.sp_window_bits() == w
    assert W.table_bytes(w) <= lib.sp_table_bytes() <= W.table_bytes(w) + 63 * 16 * 64  # + the masked walk's table
    print("window_widths: width %d nwin %d w0 %d table_bytes %d init_s %.3f" % (
        w, len(W.plan(w)), W.plan(w)[0][1], lib.sp_table_bytes(), INIT_SECONDS[w]))
    yield w
    torch.cuda.synchronize()
    lib.sp_shutdown()
    _lib.ensure_init()  # back to the environment's plan for whatever runs next


@pytest.fixture(scope="module")
def lib(width):
    from starkperp import _lib
    return _lib.ensure_init()


def wrong_rows(got, want):
    return np.flatnonzero((got != want).any(axis=1))


# ---- 1. batches ---------------------------------------------------------------------------------------------------
def test_ladder_batches(lib, width):
    """pedersen_plan_cases.check_batch at its ladder sizes: clean, and with injected out-of-range rows."""
    full_only(width)
    for n in PC.LADDER:
        PC.check_batch(lib, n)


def test_tiled_batches(lib, width):
    """The crafted pairs of this width scattered over table rows, at one size inside every class of the dispatcher: every
    row and every status byte; then the same batch with injected rows."""
    full_only(width)
    for n in TILED_SIZES:
        x, y, expected = W.tiled(width, n)
        rc, out, status = PC.run_batch(lib, x, y)
        assert rc == 0 and not status.any(), (n, rc, PC._first(status != 0))
        bad = wrong_rows(out, expected)
        assert bad.size == 0, "n = %d: %d wrong rows, first %s" % (n, bad.size, bad[:8].tolist())
        xi, yi, ei, si = PC.inject(n, x, y, expected)
        rc, out, status = PC.run_batch(lib, xi, yi)
        assert rc == 0 and (status == si).all(), (n, rc, PC._first(status != si))
        bad = np.flatnonzero((out != ei).any(axis=1) & (si == 0))
        assert bad.size == 0, "n = %d, injected: %d wrong rows, first %s" % (n, bad.size, bad[:8].tolist())


def test_crafted_pairs_alone_and_as_points(lib, width):
    """The crafted pairs as one small batch (eight quads, or eight lanes at widths 4 .. 6) and through
    sp_pedersen_point_batch (ped_point_kernel: pop_bits with this w0): x is the hash, (x, y) is on the curve, and eight
    points equal the Python oracle's."""
    from oracle import ref_py as R
    from starkperp import batch
    records = W.crafted(width)[0]
    x, y, expected = W.crafted_arrays(width)
    rc, out, status = PC.run_batch(lib, x, y)
    assert rc == 0 and not status.any()
    bad = wrong_rows(out, expected)
    assert bad.size == 0, "wrong: %s" % [records[i][4] for i in bad[:8]]
    pairs = W.crafted_pairs(width)
    points = batch.pedersen_points_many([p[0] for p in pairs], [p[1] for p in pairs])
    want = W.crafted_expected(width)
    for i, (px, py) in enumerate(points):
        assert px == want[i] and E.on_curve((px, py)), records[i][4]
    for i in random.Random(width).sample(range(len(pairs)), 8):
        assert points[i] == tuple(R.pedersen_hash_as_point(*pairs[i])), records[i][4]


# ---- 2. dense forests ---------------------------------------------------------------------------------------------
def check_forest(lib, module, n_trees, height):
    leaves, want = module.forest(n_trees, height)
    got, status = TF.run_forest(lib, leaves, n_trees, height)
    assert status == 0
    bad = wrong_rows(got, want)
    assert bad.size == 0, "(%d, %d): %s" % (n_trees, height, TF.describe(bad, n_trees, height))


def check_bad_leaf(lib, module, n_trees, height, tree, leaf):
    """One leaf = p: the status byte says so, every node that is not above that leaf is the oracle's, and a clean call
    straight afterwards reports 0 again."""
    leaves, want = module.forest(n_trees, height)
    spoiled = np.array(leaves)
    spoiled[(tree << height) + leaf] = PC.felts_from_ints([P])[0]
    got, status = TF.run_forest(lib, spoiled, n_trees, height)
    assert status == PC.HASH_OUT_OF_RANGE
    keep = np.ones(want.shape[0], dtype=bool)
    keep[TF.path_rows(n_trees, height, tree, leaf)] = False
    keep[(tree << height) + leaf] = False
    assert wrong_rows(got[keep], want[keep]).size == 0
    got, status = TF.run_forest(lib, leaves, n_trees, height)
    assert status == 0 and wrong_rows(got, want).size == 0


def test_plan_forests(lib, width):
    for n_trees, height in ((REDUCED_FOREST,) if width in REDUCED else PLAN_FORESTS):
        check_forest(lib, PC, n_trees, height)
    shape = REDUCED_FOREST if width in REDUCED else (5, 13)
    check_bad_leaf(lib, PC, *[c for c in PC.FOREST_BAD_LEAF if c[:2] == shape][0])


def test_tail_forests(lib, width):
    full_only(width)
    for n_trees, height in TAIL_FORESTS:
        check_forest(lib, TF, n_trees, height)
    check_bad_leaf(lib, TF, *[c for c in TF.BAD_LEAF if c[:2] == (20, 13)][0])


# ---- 3. sparse trees ----------------------------------------------------------------------------------------------
def replay(height, empty_leaf, sizes):
    """The fixed history on a LibrarySparseTree against the host twin on the C oracle: the root pair of every update; the
    last update with its witnesses before and after; then get_many, sp_tree_prove folded by sp_merkle_verify_paths, and
    sp_merkle_verify_update on the sp_tree_witness records."""
    from starkperp import batch_np, state
    history, roots, twin = W.sparse_expected(height, empty_leaf, sizes)
    tree = state.LibrarySparseTree(height, empty_leaf)
    try:
        assert tree.root == twin.empties[height]
        for mods, want in zip(history[:-1], roots[:-1]):
            assert tree.update(mods) == want, len(mods)
        last = history[-1]
        keys = np.array(sorted(last), dtype=np.uint64)
        prev = tree.get_many(keys.tolist())
        new = batch_np.felts_from_ints([last[int(k)] for k in keys])
        before = batch_np.tree_witness(tree, keys)
        prev_root, new_root = tree.update_arrays(keys, new)
        assert (prev_root, new_root) == roots[-1]
        after = batch_np.tree_witness(tree, keys)
        sample = random.Random(height).sample(sorted(set().union(*history)), min(200, 1 << height))
        sample += [k for k in (0, (1 << height) - 1) if k not in sample]
        assert tree.get_many(sample) == twin.get_many(sample)
        # inclusion proofs of every key of the last batch against the expected root
        leaves, sib = batch_np.tree_prove(tree, keys)
        assert batch_np.ints_from_felts(leaves) == [last[int(k)] for k in keys]
        root = batch_np.felts_from_ints([roots[-1][1]])
        verdict, st = batch_np.merkle_verify_paths(leaves, sib, keys, root, height=height)
        assert verdict.all() and not st.any()
        spoiled = sib.copy()
        i, level = len(keys) // 2, height // 2
        spoiled[i, level, 0] ^= np.uint64(1)
        verdict, st = batch_np.merkle_verify_paths(leaves, spoiled, keys, root, height=height)
        assert not verdict[i] and verdict.sum() == len(keys) - 1 and not st.any()
        # the update, verified from its witnesses
        args = (height, keys, batch_np.felts_from_ints(prev), new, prev_root, new_root)
        verdict, status = batch_np.merkle_verify_update(*args, before, after)
        assert verdict is True and not status.any()
        after[2][after[2].shape[0] // 3, 0] ^= np.uint64(1)
        verdict, status = batch_np.merkle_verify_update(*args, before, after)
        assert verdict is False and status[1].any() and not status[0].any()
    finally:
        tree.close()


@pytest.mark.parametrize("empty_leaf", EMPTY_LEAVES, ids=["empty_0", "empty_nonzero"])
def test_sparse_tree_height_64(lib, width, empty_leaf):
    """Updates of 1, 40, 600, 5000 and 3000 keys: levels of 1 .. 2048, 2049 .. 4096 and 4097 .. 8192 hashes - the
    eight-quad kernel and the sparse four- and two-quad forms, the fused path launches below them (the lane-split kernels
    level by level at widths 4 .. 6)."""
    full_only(width)
    replay(64, empty_leaf, W.SPARSE_BATCHES)


def test_sparse_tree_height_3(lib, width):
    replay(3, EMPTY_LEAVES[1], SMALL_TREE_SIZES)


# ---- 4. chains ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(n, depth):
    chains = CR.random_chains([depth] * n, seed=1000 * depth + n)
    words = np.stack([PC.felts_from_ints([c[j] for c in chains]) for j in range(depth)])
    return words, PC.felts_from_ints(CR.oracle_fold(chains))


@functools.lru_cache(maxsize=None)
def ragged_case():
    chains = CR.random_chains(CR.random_lengths(500, 7, seed=500), seed=501)  # 1 .. 7 words: 0 .. 6 hashes
    return CR.csr(chains), PC.felts_from_ints(CR.oracle_fold(chains))


def test_chains(lib, width):
    """sp_pedersen_chains at 300 x 5 (the chain fusion where the plan allows it) and 9000 x 3 (one launch per step),
    sp_pedersen_chains_ragged on 500 chains of 1 .. 7 words, and the ragged status case."""
    full_only(width)
    from starkperp import batch_np
    for n, depth in ((300, 5), (9000, 3)):
        words, want = chain_case(n, depth)
        bad = wrong_rows(batch_np.pedersen_chains(words), want)
        assert bad.size == 0, "%d x %d: %d wrong chains, first %s" % (n, depth, bad.size, bad[:8].tolist())
    (words, off), want = ragged_case()
    out, st = batch_np.pedersen_chains_ragged(words, off)
    assert not st.any() and wrong_rows(out, want).size == 0
    CR.check_status_case(batch_np)


# ---- 5. the EC_GEN walk -------------------------------------------------------------------------------------------
@pytest.fixture
def wbits(width):
    if width > 22:
        pytest.skip("the EC_GEN table of widths above 22 is the 22-bit one, tested at width 22")
    return width


def test_public_keys_of_the_generator_scalars(lib, wbits):
    from starkperp import _lib, batch
    ks = list(W.gen_scalars(wbits))
    got = batch.public_keys_many(ks)
    want = W.gen_points(wbits)
    bad = [i for i in range(len(ks)) if got[i] != want[i]]
    assert not bad, "first wrong scalars: %s" % [hex(ks[i]) for i in bad[:4]]
    dd = ks[:5] + [0, N] + ks[5:9]
    qx, qy, st = _lib.new_felts(len(dd)), _lib.new_felts(len(dd)), _lib.new_bytes(len(dd))
    _lib.check(lib.sp_public_key_batch(_lib.pack_felts(dd), qx, qy, st, len(dd)), "sp_public_key_batch")
    assert list(bytes(st)[:len(dd)]) == [SC.OK] * 5 + [SC.BAD_INPUT] * 2 + [SC.OK] * 4
    pts = list(zip(_lib.unpack_felts(qx, len(dd)), _lib.unpack_felts(qy, len(dd))))
    assert pts[:5] == want[:5] and pts[7:] == want[5:9]


def test_sign_attempts_with_the_generator_scalars_as_nonces(lib, wbits):
    from starkperp import batch
    items = W.sign_items(wbits)
    want = [SC.attempt(*it) for it in items]
    rs, ss, st = batch.sign_attempt_many([it[0] for it in items], [it[1] for it in items], [it[2] for it in items])
    bad = [i for i in range(len(items)) if (st[i], rs[i], ss[i]) != want[i]]
    assert not bad, "first wrong items: %s" % bad[:4]
    assert st.count(SC.RETRY) >= 8 and st.count(SC.BAD_INPUT) == 2


@functools.lru_cache(maxsize=None)
def golden_verify_cases():
    import json
    import os
    cases = json.load(open(os.path.join(E.GOLDEN, "g4_verify.json")))["cases"]
    cases = [c for c in cases if not isinstance(c["key"], list)]
    return cases


def test_verify_with_u1_on_the_generator_scalars(lib, wbits):
    """The g4 golden cases, and signatures whose u1 = z / s is each generator scalar: the valid ones and their r + 1
    twins.  Verdict codes of all of them from the C oracle's three-ladder verify, of a sample of four from oracle.ref_py
    (whose verification takes 20 ms); with point keys and x-only keys, on the per-signature ladder."""
    from oracle import ref_py as R
    from starkperp import batch
    import test_gpu_ecdsa as TE
    h = TE.h
    cases = golden_verify_cases()
    codes = batch.verify_codes([h(c["z"]) for c in cases], [h(c["r"]) for c in cases], [h(c["s"]) for c in cases],
                               [TE._key(c) for c in cases])
    for c, code in zip(cases, codes):
        if c["expect"] in ("true", "false"):
            assert code == (1 if c["expect"] == "true" else 0), c["label"]
        else:
            assert code >= 2, c["label"]
    sigs, q = W.verify_items(wbits)
    zs, rs, ss = [s[0] for s in sigs], [s[1] for s in sigs], [s[2] for s in sigs]
    want = verify_expected(wbits)
    assert want.count(1) == len(W.gen_scalars(wbits)) and want.count(0) == len(want) - want.count(1)
    assert batch.verify_codes(zs, rs, ss, [q] * len(sigs), key_tables=False) == want
    assert batch.verify_codes(zs, rs, ss, [q[0]] * len(sigs), key_tables=False) == want
    for i in random.Random(wbits).sample(range(len(sigs)), 4):
        assert want[i] == int(R.verify(zs[i], rs[i], ss[i], q)), i


@functools.lru_cache(maxsize=None)
def verify_expected(wbits):
    from oracle import cref
    sigs, q = W.verify_items(wbits)
    return list(cref.verify_codes([s[0] for s in sigs], [s[1] for s in sigs], [s[2] for s in sigs], [q] * len(sigs)))


def test_lincomb_with_the_generator_scalars(lib, wbits):
    from starkperp import batch
    items = W.lincomb_items(wbits)
    got = batch.ec_lincomb_many([it[0] for it in items], [it[1] for it in items], [it[2] for it in items])
    bad = [i for i in range(len(items)) if got[i] != items[i][3]]
    assert not bad, "first wrong items: %s" % [(hex(items[i][0]), items[i][1]) for i in bad[:4]]


# ---- 6. argument edges (once, not per width) ---------------------------------------------------------------------------
def test_widths_outside_the_range_are_refused():
    """sp_init(0, w) for w outside [4, 27]: refused, sp_last_error names the range, the library stays uninitialised; a
    following sp_init(0, 4) succeeds and hashes the goldens."""
    import torch
    from starkperp import _lib, batch
    import test_gpu_pedersen as TP
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.sp_shutdown()
    try:
        for w in (-1, 1, 3, 28, 64):
            assert lib.sp_init(0, w) != 0, w
            assert b"[4, 27]" in lib.sp_last_error(), (w, lib.sp_last_error())
            assert lib.sp_is_initialised() == 0, w
        _lib.check(lib.sp_init(0, 4), "sp_init")
        assert lib.sp_is_initialised() == 1 and lib.sp_window_bits() == 4
        TP.test_g1_full_batch(batch)
        TP.test_edges_and_kats(batch)
    finally:
        torch.cuda.synchronize()
        lib.sp_shutdown()
        _lib.ensure_init()
