"""The verifier on the GPU: sp_air_eval_points_dev against the dense composition kernels bit for bit and against the
integers of tests/verify_cases.py, sp_fri_check_queries_dev against layers folded by sp_fri_fold_dev and against the
cases' statuses, the argument rules and the one-launch promise of both calls, and stark.verify end to end - proofs of
all four AIRs, the tamperings of test_prove_then_verify_small and two forged proofs, each answer compared as a whole
with oracle/stark_ref.verify_proof on the C oracle's hash - plus one full-size proof."""
import copy
import ctypes
import functools
import random

import numpy as np
import pytest

import verify_cases as V
from oracle import ref_py as R
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
AIRS = ("range_check", "ec_ladder", "pedersen", "ecdsa")
P = V.P
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from starkperp import _lib, stark
    return torch, _lib.ensure_init(), stark


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


def ptr(t):
    return None if t is None else t.data_ptr()


def points_raw(gpu, air_id, log_n, per, alphas, shift, count, pos, cur, nxt, extra=3):
    """The C call on sentinel-filled outputs of count + extra items: (rc, values, statuses, tail untouched)."""
    torch, lib, _ = gpu
    from starkperp import _lib
    out = torch.full((count + extra, 4), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.full((count + extra,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.sp_air_eval_points_dev(air_id, log_n, ptr(per), _lib.pack_felts(alphas), _lib.pack_felts([shift]), count,
                                    ptr(pos), ptr(cur), ptr(nxt), out.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    vals, st = V.ints_of(out.cpu().numpy().view(np.uint64)), status.cpu().tolist()
    sentinel_felt = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little")
    clean = vals[count:] == [sentinel_felt] * extra and st[count:] == [0xEE] * extra
    return rc, vals[:count], st[:count], clean


def fri_raw(gpu, log_m, n_layers, shift, betas, count, index, pairs, final, extra=3):
    torch, lib, _ = gpu
    from starkperp import _lib
    status = torch.full((count * n_layers + extra,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.sp_fri_check_queries_dev(log_m, n_layers, _lib.pack_felts([shift]), _lib.pack_felts(betas), count,
                                      ptr(index), ptr(pairs), ptr(final), status.data_ptr(), None)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    return rc, [st[q * n_layers:(q + 1) * n_layers] for q in range(count)], st[count * n_layers:] == [0xEE] * extra


# ---- composition values: the dense kernels, bit for bit ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_of(air):
    """(cols tensor, periodic tensor, dense composition as ints) of the AIR's case, computed once."""
    import torch
    from starkperp import stark
    c = V.air_case(air)
    cols = torch.stack([to_device(torch, V.felts_np(col)) for col in c.cols])
    per = stark.periodic_lde(c.n, V.SHIFT, "cuda", air)
    dense = stark.air_eval(cols, per, c.n, c.alphas, V.SHIFT, air)
    return cols, per, stark.tensor_to_felts(dense)


@pytest.mark.parametrize("air", AIRS)
def test_points_equal_the_dense_kernel_and_the_integers(gpu, air):
    torch, lib, stark = gpu
    c = V.air_case(air)
    cols, per, dense = dense_of(air)
    assert V.ints_of(per.cpu().numpy().view(np.uint64)) == [v for tab in c.per for v in tab]
    for count in V.ITEM_COUNTS:
        pos, cur, nxt, want = c.arrays(count)
        idx = to_device(torch, pos)
        # the rows gathered on the device from the dense columns are the case's rows
        g_cur = cols[:, idx, :].permute(1, 0, 2).contiguous()
        g_nxt = cols[:, (idx + 4) % c.M, :].permute(1, 0, 2).contiguous()
        assert torch.equal(g_cur.reshape(-1, 4), to_device(torch, cur))
        (res, launches, units) = profiled(lib, lambda: points_raw(gpu, V.AIR_IDS[air], V.MIN_LOG_N[air], per, c.alphas,
                                                                  V.SHIFT, count, idx, g_cur, g_nxt))
        rc, vals, st, clean = res
        assert rc == 0 and clean and (launches, units) == (1, count)
        assert st == [V.POINT_OK] * count
        assert vals == [dense[p] for p in c.positions[:count]], (air, count)
        assert vals == want, (air, count)
    out, st = stark.air_eval_points(air, c.n, per, c.alphas, V.SHIFT, idx, g_cur, g_nxt)  # the wrapper, 257 points
    assert stark.tensor_to_felts(out) == c.expected and st.cpu().tolist() == [0] * 257


@pytest.mark.parametrize("air", AIRS)
def test_points_flag_out_of_range_items(gpu, air):
    torch, lib, stark = gpu
    c = V.air_case(air)
    _, per, _ = dense_of(air)
    items = c.bad_items()
    pos = to_device(torch, np.array([it[0] for it in items], dtype=np.uint64))
    cur = to_device(torch, V.felts_np([v for it in items for v in it[1]]))
    nxt = to_device(torch, V.felts_np([v for it in items for v in it[2]]))
    rc, vals, st, clean = points_raw(gpu, V.AIR_IDS[air], V.MIN_LOG_N[air], per, c.alphas, V.SHIFT, len(items), pos, cur, nxt)
    assert rc == 0 and clean
    assert st == [V.POINT_OK if it[3] is not None else V.POINT_OUT_OF_RANGE for it in items]
    assert vals == [it[3] or 0 for it in items]


# ---- fold chains -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.FRI_SHAPES)
def test_fold_checks_accept_the_layers_of_the_fold_kernel(gpu, shape):
    torch, lib, stark = gpu
    c = V.fri_case(*shape)
    layers, s = [to_device(torch, V.felts_np(c.layers[0]))], V.SHIFT
    for k in range(c.n_layers):
        layers.append(stark.fri_fold(layers[-1], c.betas[k], s))
        s = s * s % P
    host = [stark.tensor_to_felts(t) for t in layers]
    assert host == c.layers
    m = 1 << c.log_m
    index = list(range(0, m // 2, max(1, m // 512)))[:256] + [m // 2 - 1]
    pairs = []
    for j in index:
        for k in range(c.n_layers):
            mk = m >> k
            pairs += [host[k][j % (mk // 2)], host[k][j % (mk // 2) + mk // 2]]
    st = stark.fri_check_queries(c.log_m, c.betas, V.SHIFT, torch.tensor(index, dtype=torch.int64, device="cuda"),
                                 to_device(torch, V.felts_np(pairs)).reshape(len(index), c.n_layers, 2, 4), layers[-1])
    assert st.cpu().tolist() == [[V.FOLD_OK] * c.n_layers] * len(index)


@pytest.mark.parametrize("shape", V.FRI_SHAPES)
def test_fold_checks_equal_the_integer_statuses(gpu, shape):
    torch, lib, stark = gpu
    c = V.fri_case(*shape)
    index, pairs, final, _ = c.arrays()
    args = [to_device(torch, a) for a in (index, pairs, final)]
    (res, launches, units) = profiled(lib, lambda: fri_raw(gpu, c.log_m, c.n_layers, V.SHIFT, c.betas, len(index), *args))
    rc, st, clean = res
    assert rc == 0 and clean and (launches, units) == (1, len(index) * c.n_layers)
    for q, (got, want) in enumerate(zip(st, c.expected)):
        assert got == want, (q, c.notes[q], c.index[q])


# ---- argument edges ----------------------------------------------------------------------------------------------------
def test_argument_rules_of_both_calls(gpu):
    torch, lib, stark = gpu
    from starkperp import _lib
    c = V.air_case("range_check")
    _, per, _ = dense_of("range_check")
    pos, cur, nxt, want = c.arrays(65)
    d = [to_device(torch, a) for a in (pos, cur, nxt)]
    good = (V.AIR_IDS["range_check"], 7, per, c.alphas, V.SHIFT, 65) + tuple(d)
    assert points_raw(gpu, *good)[:2] == (0, want)

    def refused(args, raw=points_raw):
        (res, launches, _) = profiled(lib, lambda: raw(gpu, *args))
        assert res[0] == -3 and res[-1] and launches == 0, args[:2]
        return _lib.last_error()
    # a count of 0: SP_OK, no launch, nothing written, NULL arrays allowed
    (res, launches, _) = profiled(lib, lambda: points_raw(gpu, 3, 7, None, c.alphas, V.SHIFT, 0, None, None, None))
    assert res[0] == 0 and res[3] and launches == 0
    for air_id in (-1, 4, 1 << 20):
        assert "air" in refused((air_id,) + good[1:])
    for air, lo in V.MIN_LOG_N.items():
        for log_n in (lo - 1, 31, 0):
            assert "log_n" in refused((V.AIR_IDS[air], log_n) + good[2:])
    for k in (2, 6, 7, 8):  # per, pos, cur, nxt
        assert "NULL" in refused(good[:k] + (None,) + good[k + 1:])
    for bad_shift in (0, 1, P - 1, P, pow(3, (P - 1) // 512, P)):
        assert "shift" in refused(good[:4] + (bad_shift,) + good[5:])
    # above 2^30 items: refused from the count alone (called directly: no output of that size is allocated here)
    small = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    st8 = torch.full((8,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.sp_air_eval_points_dev(3, 7, ptr(per), _lib.pack_felts(c.alphas), _lib.pack_felts([V.SHIFT]), (1 << 30) + 1,
                                    ptr(d[0]), ptr(d[1]), ptr(d[2]), small.data_ptr(), st8.data_ptr(), None)
    assert rc == -3 and "2^30" in _lib.last_error()
    torch.cuda.synchronize()
    assert st8.cpu().tolist() == [0xEE] * 8 and bool((small == SENTINEL).all())
    # the fold call
    f = V.fri_case(7, 1)
    index, pairs, final, _ = f.arrays()
    fd = [to_device(torch, a) for a in (index, pairs, final)]
    fgood = (7, 1, V.SHIFT, f.betas, len(index)) + tuple(fd)
    assert fri_raw(gpu, *fgood)[:2] == (0, f.expected)
    (res, launches, _) = profiled(lib, lambda: fri_raw(gpu, 7, 1, V.SHIFT, f.betas, 0, None, None, None))
    assert res[0] == 0 and res[2] and launches == 0
    for log_m, n_layers in ((7, 0), (7, 7), (7, 9), (33, 1), (1, 1), (0, 0)):
        assert "n_layers" in refused((log_m, n_layers) + fgood[2:], fri_raw)
    for k in (5, 6, 7):
        assert "NULL" in refused(fgood[:k] + (None,) + fgood[k + 1:], fri_raw)
    for bad_shift in (0, P, 2**256 - 1):
        assert "shift" in refused(fgood[:2] + (bad_shift,) + fgood[3:], fri_raw)


def test_one_launch_serves_two_to_the_sixteen_items(gpu):
    torch, lib, stark = gpu
    count = 1 << 16
    c = V.air_case("range_check")
    _, per, _ = dense_of("range_check")
    pos, cur, nxt, want = c.arrays(256)
    reps = count // 256
    d = [to_device(torch, np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in (pos, cur, nxt)]
    (res, launches, units) = profiled(lib, lambda: points_raw(gpu, 3, 7, per, c.alphas, V.SHIFT, count, *d))
    assert res[0] == 0 and res[3] and (launches, units) == (1, count)
    assert res[1] == want * reps and res[2] == [0] * count
    f = V.fri_case(9, 3)
    index, pairs, final, _ = f.arrays()
    nq = len(index)
    reps = -(-count // nq)
    big_index = np.tile(index, reps)[:count]
    big_pairs = np.tile(pairs, (reps, 1))[:count * 3 * 2]
    fd = [to_device(torch, a) for a in (big_index, big_pairs, final)]
    (res, launches, units) = profiled(lib, lambda: fri_raw(gpu, 9, 3, V.SHIFT, f.betas, count, *fd))
    assert res[0] == 0 and res[2] and (launches, units) == (1, 3 * count)
    assert res[1] == (f.expected * reps)[:count]


# ---- end to end ----------------------------------------------------------------------------------------------------------
FINAL_LOG = {"ecdsa": 6, "pedersen": 6, "ec_ladder": 5, "range_check": 5}


def chash(a, b):
    from oracle import cref
    return cref.pedersen_hash_many([a], [b])[0][0]


@functools.lru_cache(maxsize=None)
def proof_of(air):
    """One proof per AIR at the smallest n, 3 queries."""
    from starkperp import stark
    rng = random.Random("verify-e2e-" + air)
    kw = {"n_queries": 3, "seed": 11, "final_log": FINAL_LOG[air]}
    if air == "pedersen":
        return stark.prove(stark.felts_to_tensor([rng.randrange(P)]), stark.felts_to_tensor([rng.randrange(P)]), **kw)
    if air == "ec_ladder":
        q = R.ec_mult(rng.randrange(1, R.EC_ORDER), tuple(R.EC_GEN))
        return stark.prove_ec_ladders(stark.felts_to_tensor([rng.randrange(1, 2**251)]), stark.felts_to_tensor([q[0]]),
                                      stark.felts_to_tensor([q[1]]), **kw)
    if air == "range_check":
        return stark.prove_range_checks([rng.randrange(2**128)], **kw)
    while True:
        z, d = rng.randrange(1, 2**251), rng.randrange(1, R.EC_ORDER)
        r, s = R.sign(z, d)
        if 1 <= pow(s, -1, R.EC_ORDER) < 2**251:
            return stark.prove_ecdsa([z], [r], [s], [R.ec_mult(d, tuple(R.EC_GEN))], **kw)


def _swap_pair(p):
    pair = p["queries"][1]["layers"][1]
    pair[0], pair[1] = pair[1], pair[0]


def _set(path, fn):
    def f(p):
        o = p
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = fn(o[path[-1]])
    return f


TAMPERINGS = {
    "nothing": lambda p: None,
    "a trace value": _set(("queries", 0, "trace", 0, "values", 0), lambda v: v ^ 1),
    "a trace path node": _set(("queries", 2, "trace", 3, "path", 4), lambda v: v ^ 1),
    "a layer path node": _set(("queries", 1, "layers", 1, 1, "path", 0), lambda v: v ^ 1),
    "a layer value": _set(("queries", 1, "layers", 2, 0, "value"), lambda v: v ^ 1),
    "a final-layer value": _set(("final_layer", 5), lambda v: v ^ 1),
    "a layer root": _set(("layer_roots", 0), lambda v: v ^ 1),
    "the seed": _set(("seed",), lambda v: v + 1),
    "the public inputs": _set(("public_inputs",), lambda v: [1]),
    "a swapped pair": _swap_pair,
    "a wrong row": _set(("queries", 0, "trace", 2, "row"), lambda v: v + 1),
    "a wrong index": _set(("queries", 2, "index"), lambda v: v ^ 1),
}


@pytest.mark.parametrize("what", sorted(TAMPERINGS))
@pytest.mark.parametrize("air", AIRS)
def test_verify_agrees_with_the_oracle(gpu, air, what):
    torch, lib, stark = gpu
    proof = copy.deepcopy(proof_of(air))
    TAMPERINGS[what](proof)
    want = S.verify_proof(proof, hash2=chash, final_log=FINAL_LOG[air])
    assert stark.verify(proof, final_log=FINAL_LOG[air]) == want, (air, what)
    assert want == (True, "ok") if what == "nothing" else not want[0]
    if what == "nothing":
        assert stark.verify(proof, final_log=FINAL_LOG[air], n_queries=3) == (True, "ok")
        assert stark.verify(proof, final_log=FINAL_LOG[air], n_queries=4) == (False, "shape")


def forge(stark, trace, air, final_log, n_queries, bad_alpha=False, bad_beta_layer=None, seed=5):
    """prove_trace written out with the module's public pieces, with one dishonest step: the composition column
    computed with alphas[0] + 1, or ONE layer folded with beta + 1.  Every commitment and opening is honest about the
    columns the forger holds, so the Merkle checks pass and only the algebra can tell."""
    shift = stark.FIELD_GEN
    spec = stark.AIRS[air]
    n = trace.shape[1]
    M = 4 * n
    tr = stark.Transcript(air, n, shift, seed, ())
    trace_lde = stark.lde(trace)
    lv_trace = stark.commit_rows(trace_lde)
    root_t = stark.root_of(lv_trace)
    tr.absorb("trace_root", root_t)
    alphas = [tr.challenge("alpha", k) for k in range(spec["n_constraints"])]
    if bad_alpha:
        alphas[0] = (alphas[0] + 1) % P
    comp = stark.air_eval(trace_lde, stark.periodic_lde(n, shift, "cuda", air), n, alphas, shift, air)
    layers, bufs, roots, s = [comp], [], [], shift
    while layers[-1].shape[0] > (1 << final_log):
        lv = stark.commit_rows(layers[-1].unsqueeze(0))
        bufs.append(lv)
        roots.append(stark.root_of(lv))
        tr.absorb("layer_root", roots[-1])
        beta = tr.challenge("beta", len(roots))
        if bad_beta_layer == len(roots) - 1:
            beta = (beta + 1) % P
        layers.append(stark.fri_fold(layers[-1], beta, s))
        s = s * s % P
    final = stark.tensor_to_felts(layers[-1])
    tr.absorb("final_layer", *final)
    tables = [(trace_lde, lv_trace)] + list(zip(layers[:-1], bufs))
    indices = [tr.challenge("query", q, modulus=M // 2) for q in range(n_queries)]
    picks = []
    for j in indices:
        picks += [(0, r) for pos in (j, j + M // 2) for r in (pos, (pos + 4) % M)]
        for k in range(len(bufs)):
            mk = M >> k
            picks += [(1 + k, j % (mk // 2)), (1 + k, j % (mk // 2) + mk // 2)]
    opened = iter(zip(picks, stark.open_rows(tables, picks)))
    queries = []
    for j in indices:
        q = {"index": j, "trace": [], "layers": []}
        for _ in range(4):
            (_, row), (values, _, path) = next(opened)
            q["trace"].append({"row": row, "values": values, "path": path})
        for _ in bufs:
            q["layers"].append([{"pos": pos, "value": values[0], "path": path}
                                for (_, pos), (values, _, path) in (next(opened), next(opened))])
        queries.append(q)
    return {"n": n, "air": air, "seed": seed, "shift": shift, "public_inputs": [], "trace_root": root_t,
            "layer_roots": roots, "final_layer": final, "queries": queries}


def test_forged_proofs_fail_on_the_algebra_alone(gpu):
    torch, lib, stark = gpu
    rng = random.Random(77)
    trace = stark.pedersen_trace(stark.felts_to_tensor([rng.randrange(P)]), stark.felts_to_tensor([rng.randrange(P)]))
    honest = forge(stark, trace, "pedersen", 6, 3)
    assert stark.verify(honest) == (True, "ok") == S.verify_proof(honest, hash2=chash)
    bad = forge(stark, trace, "pedersen", 6, 3, bad_alpha=True)
    assert all(ok for _, ok in stark.check_merkle_openings(bad))
    assert stark.verify(bad) == (False, "composition value") == S.verify_proof(bad, hash2=chash)
    bad = forge(stark, trace, "pedersen", 6, 3, bad_beta_layer=2)  # log_m 11, 5 layers: a middle one
    assert all(ok for _, ok in stark.check_merkle_openings(bad))
    assert stark.verify(bad) == (False, "fold consistency at layer 2") == S.verify_proof(bad, hash2=chash)


def test_a_full_size_proof_verifies(gpu):
    """2^20 rows of the Pedersen-step AIR, 4 queries: log_m 22, 16 layers."""
    torch, lib, stark = gpu
    g = torch.Generator().manual_seed(19)
    xs = torch.randint(0, 2**62, (2048, 4), dtype=torch.int64, generator=g)
    ys = torch.randint(0, 2**62, (2048, 4), dtype=torch.int64, generator=g)
    xs[:, 3] &= (1 << 58) - 1
    ys[:, 3] &= (1 << 58) - 1
    proof = stark.prove(xs.cuda(), ys.cuda(), n_queries=4, seed=3)
    assert len(proof["layer_roots"]) == 16 and len(proof["final_layer"]) == 64
    assert stark.verify(proof, n_queries=4) == (True, "ok")
    proof["queries"][3]["layers"][15][1]["path"][0] ^= 1 << 100
    assert stark.verify(proof) == (False, "layer path")
