"""The builtins verifier on the GPU: sp_builtins_eval_points_dev against the dense column that _commit_builtins builds
(air_eval per segment, air_eval_rc16, felt_add) bit for bit and against the integers of
tests/builtins_verify_cases.py, its out-of-range items, argument rules and one-launch promise, and
stark.verify_builtins end to end - proofs of four segment lists, every tampering a list's segments admit and four
forged proofs, each answer compared as a whole with oracle/stark_ref.verify_builtins_proof on the C oracle's hash."""
import copy
import functools
import random

import numpy as np
import pytest

import builtins_verify_cases as B
from oracle import ref_py as R
from oracle import stark_ref as S
from test_gpu_verify import SENTINEL, chash, profiled, ptr, to_device

pytestmark = pytest.mark.gpu
SETS = B.SEGMENT_SETS
set_id = "+".join
P = B.P
SENTINEL_FELT = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from starkperp import _lib, stark
    return torch, _lib.ensure_init(), stark


@functools.lru_cache(maxsize=None)
def device_case(segments):
    """(columns [n_cols, M, 4], phase-2 column [M, 4], periodic tables by name, dense composition as ints) of the
    set's case: the dense column built the way _commit_builtins builds it, once."""
    import torch
    from starkperp import stark
    c = B.builtins_case(segments)
    cols = torch.stack([to_device(torch, B.felts_np(col)) for col in c.cols])
    pcol = to_device(torch, B.felts_np(c.pcol))
    pers = {s: stark.periodic_lde(c.n, B.SHIFT, "cuda", s) for s in segments}
    comp = None
    for seg, c0, nc, a0, na in c.layout:
        sl, al = cols[c0:c0 + nc], c.alphas[a0:a0 + na]
        part = (stark.air_eval_rc16(sl, pcol, pers[seg], c.n, al, c.z, c.rc_min, c.rc_max, B.SHIFT) if seg == "rc16"
                else stark.air_eval(sl, pers[seg], c.n, al, B.SHIFT, seg))
        comp = part if comp is None else stark.felt_add(comp, part)
    return cols, pcol, pers, stark.tensor_to_felts(comp)


def good_args(segments, count, arrays=None):
    """The arguments of a good raw call on the set's case, by name (device arrays from the case's first `count`
    points unless `arrays` gives the five host arrays)."""
    import torch
    c = B.builtins_case(segments)
    _, _, pers, _ = device_case(segments)
    pos, cur, nxt, pcur, pnxt = (c.arrays(count)[:5] if arrays is None else arrays)
    d = [to_device(torch, a) for a in (pos, cur, nxt, pcur, pnxt)]
    return {"mask": c.mask, "log_n": c.log_n, "per_pedersen": pers.get("pedersen"), "per_ecdsa": pers.get("ecdsa"),
            "per_rc16": pers.get("rc16"), "alphas": c.alphas, "shift": B.SHIFT, "z": c.z if c.has_rc else None,
            "rc_min": c.rc_min, "rc_max": c.rc_max, "count": len(pos), "pos": d[0], "cur": d[1], "nxt": d[2],
            "pcur": d[3] if c.has_rc else None, "pnxt": d[4] if c.has_rc else None, "out": True, "status": True}


def points_raw(gpu, a, extra=3):
    """The C call on sentinel-filled outputs of count + extra items: (rc, values, statuses, tail untouched).  An
    output named None in `a` is passed as NULL (the buffers are still checked)."""
    torch, lib, _ = gpu
    from starkperp import _lib
    count = a["count"]
    out = torch.full((count + extra, 4), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.full((count + extra,), 0xEE, dtype=torch.uint8, device="cuda")
    pack = lambda v: None if v is None else _lib.pack_felts(v if isinstance(v, list) else [v])
    rc = lib.sp_builtins_eval_points_dev(a["mask"], a["log_n"], ptr(a["per_pedersen"]), ptr(a["per_ecdsa"]),
                                         ptr(a["per_rc16"]), pack(a["alphas"]), pack(a["shift"]), pack(a["z"]),
                                         a["rc_min"], a["rc_max"], count, ptr(a["pos"]), ptr(a["cur"]), ptr(a["nxt"]),
                                         ptr(a["pcur"]), ptr(a["pnxt"]), out.data_ptr() if a["out"] else None,
                                         status.data_ptr() if a["status"] else None, None)
    torch.cuda.synchronize()
    vals, st = B.ints_of(out.cpu().numpy().view(np.uint64)), status.cpu().tolist()
    clean = vals[count:] == [SENTINEL_FELT] * extra and st[count:] == [0xEE] * extra
    if rc != 0:
        clean = clean and vals[:count] == [SENTINEL_FELT] * count and st[:count] == [0xEE] * count
    return rc, vals[:count], st[:count], clean


# ---- composition values: the dense column, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("segments", SETS, ids=set_id)
def test_points_equal_the_dense_column_and_the_integers(gpu, segments):
    torch, lib, stark = gpu
    c = B.builtins_case(segments)
    cols, pcol, pers, dense = device_case(segments)
    for seg in segments:
        assert B.ints_of(pers[seg].cpu().numpy().view(np.uint64)) == [v for tab in c.pers[seg] for v in tab]
    for count in B.ITEM_COUNTS:
        pos, cur, nxt, pcur, pnxt, want = c.arrays(count)
        idx = to_device(torch, pos)
        # the rows gathered on the device from the dense columns are the case's rows
        nidx = (idx + 4) % c.M
        g = [cols[:, idx, :].permute(1, 0, 2).contiguous(), cols[:, nidx, :].permute(1, 0, 2).contiguous(),
             pcol[idx].contiguous(), pcol[nidx].contiguous()]
        assert torch.equal(g[0].reshape(-1, 4), to_device(torch, cur)) and torch.equal(g[3], to_device(torch, pnxt))
        a = good_args(segments, count)
        a.update({"pos": idx, "cur": g[0], "nxt": g[1]})
        if c.has_rc:
            a.update({"pcur": g[2], "pnxt": g[3]})
        (res, launches, units) = profiled(lib, lambda: points_raw(gpu, a))
        rc, vals, st, clean = res
        assert rc == 0 and clean and (launches, units) == (1, count)
        assert st == [B.POINT_OK] * count
        assert vals == [dense[p] for p in c.positions[:count]], (segments, count)
        assert vals == want, (segments, count)
    out, st = stark.builtins_eval_points(list(segments), c.n, pers, c.alphas, B.SHIFT, c.z, c.rc_min, c.rc_max, idx,
                                         g[0], g[1], g[2] if c.has_rc else None, g[3] if c.has_rc else None)
    assert stark.tensor_to_felts(out) == c.expected and st.cpu().tolist() == [0] * 257  # the wrapper, 257 points


@pytest.mark.parametrize("segments", SETS, ids=set_id)
def test_points_flag_out_of_range_items(gpu, segments):
    c = B.builtins_case(segments)
    items = c.bad_items()
    rc, vals, st, clean = points_raw(gpu, good_args(segments, 0, c.pack(items)))
    assert rc == 0 and clean
    assert st == [B.POINT_OK if it[5] is not None else B.POINT_OUT_OF_RANGE for it in items]
    assert vals == [it[5] or 0 for it in items]  # the neighbours' values are unchanged
    assert st.count(B.POINT_OUT_OF_RANGE) == c.n_bad()


# ---- argument edges --------------------------------------------------------------------------------------------------
def test_argument_rules(gpu):
    torch, lib, stark = gpu
    from starkperp import _lib
    rc_only, full = ("rc16",), ("pedersen", "ecdsa", "rc16")
    good = good_args(rc_only, 5)
    assert points_raw(gpu, good)[:2] == (0, B.builtins_case(rc_only).expected[:5])

    def refused(a):
        (res, launches, _) = profiled(lib, lambda: points_raw(gpu, a))
        assert res[0] == -3 and res[3] and launches == 0, a["mask"]
        return _lib.last_error()
    # the scalar rules, the same table as without a GPU
    for what, word, kw in B.refused_scalars():
        assert word in refused(dict(good, **kw)), what
    # a count of 0: SP_OK, no launch, nothing written, NULL arrays allowed
    nothing = dict(good_args(full, 1), count=0, pos=None, cur=None, nxt=None, pcur=None, pnxt=None, per_ecdsa=None)
    (res, launches, _) = profiled(lib, lambda: points_raw(gpu, nothing))
    assert res[0] == 0 and res[3] and launches == 0
    # a NULL for each needed pointer; what an absent segment would read may be NULL
    whole = good_args(full, 5)
    assert points_raw(gpu, whole)[:2] == (0, B.builtins_case(full).expected[:5])
    for key in ("per_pedersen", "per_ecdsa", "per_rc16", "alphas", "shift", "z", "pos", "cur", "nxt", "pcur", "pnxt", "out",
                "status"):
        assert "NULL" in refused(dict(whole, **{key: None})), key
    lone = good_args(("ecdsa",), 5)
    assert lone["per_pedersen"] is None and lone["per_rc16"] is None and lone["z"] is None and lone["pcur"] is None
    assert points_raw(gpu, lone)[:2] == (0, B.builtins_case(("ecdsa",)).expected[:5])
    for bad_shift in (0, 1, P - 1, P, pow(3, (P - 1) // 32, P)):  # 4 n = 32 at log_n 3
        assert "shift" in refused(dict(good, shift=bad_shift)), bad_shift
    # above 2^30 points: refused from the count alone (called directly: no output of that size is allocated here)
    small = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    st8 = torch.full((8,), 0xEE, dtype=torch.uint8, device="cuda")
    g = good
    (rc, launches, _) = profiled(lib, lambda: lib.sp_builtins_eval_points_dev(
        4, 3, None, None, ptr(g["per_rc16"]), _lib.pack_felts(g["alphas"]), _lib.pack_felts([B.SHIFT]),
        _lib.pack_felts([g["z"]]), g["rc_min"], g["rc_max"], (1 << 30) + 1, ptr(g["pos"]), ptr(g["cur"]), ptr(g["nxt"]),
        ptr(g["pcur"]), ptr(g["pnxt"]), small.data_ptr(), st8.data_ptr(), None))
    assert rc == -3 and launches == 0 and "2^30" in _lib.last_error()
    torch.cuda.synchronize()
    assert st8.cpu().tolist() == [0xEE] * 8 and bool((small == SENTINEL).all())


def test_one_launch_serves_two_to_the_sixteen_points(gpu):
    torch, lib, stark = gpu
    count = 1 << 16
    c = B.builtins_case(("rc16",))
    pos, cur, nxt, pcur, pnxt, want = c.arrays(256)
    reps = count // 256
    tiled = [np.tile(a, (reps,) + (1,) * (a.ndim - 1)) for a in (pos, cur, nxt, pcur, pnxt)]
    a = good_args(("rc16",), 0, tiled)
    (res, launches, units) = profiled(lib, lambda: points_raw(gpu, a))
    assert res[0] == 0 and res[3] and (launches, units) == (1, count)
    assert res[1] == want * reps and res[2] == [0] * count


# ---- end to end ------------------------------------------------------------------------------------------------------
def narrow_values(rng, count, lo=300, hi=420):
    """range-checked values whose limbs lie in a narrow band, so that a short trace can fill the holes"""
    return [sum(rng.randrange(lo, hi) << (16 * k) for k in range(8)) for _ in range(count)]


def instances(rng, n_hashes, n_sigs, n_values):
    hashes = [(rng.randrange(P), rng.randrange(P)) for _ in range(n_hashes)]
    signatures = []
    while len(signatures) < n_sigs:
        z, d = rng.randrange(1, 2**251), rng.randrange(1, R.EC_ORDER)
        r, s = R.sign(z, d)
        if 1 <= pow(s, -1, R.EC_ORDER) < 2**251:
            signatures.append((z, r, s, R.ec_mult(d, tuple(R.EC_GEN))))
    return hashes, signatures, narrow_values(rng, n_values)


# segment list -> (hashes, signatures, values, queries, final_log); n = 1024, 256, 1024, 1024: 6, 4, 6, 6 layers
PROOFS = {("pedersen", "ecdsa", "rc16"): (2, 1, 16, 3, 6), ("rc16",): (0, 0, 24, 2, 6), ("pedersen", "rc16"): (2, 0, 24, 2, 6),
          ("ecdsa",): (0, 1, 0, 2, 6)}


@functools.lru_cache(maxsize=None)
def proof_of(segments):
    from starkperp import stark
    nh, ns, nv, nq, final_log = PROOFS[segments]
    hashes, signatures, values = instances(random.Random("builtins-e2e-" + "+".join(segments)), nh, ns, nv)
    proof = stark.prove_builtins(hashes or None, signatures or None, values or None, n_queries=nq, seed=11,
                                 final_log=final_log)
    assert tuple(proof["segments"]) == segments and len(proof["layer_roots"]) >= 3
    return proof


def _set(path, fn):
    def f(p):
        o = p
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = fn(o[path[-1]])
    return f


def _swap_pair(p):
    pair = p["queries"][1]["layers"][1]
    pair[0], pair[1] = pair[1], pair[0]


def _drop_value(p):
    p["queries"][1]["phase1"][1]["values"].pop()


flip = lambda v: v ^ 1
COL0 = {"pedersen": lambda segs: 0, "ecdsa": lambda segs: 4 if "pedersen" in segs else 0,
        "rc16": lambda segs: sum({"pedersen": 4, "ecdsa": 10}[s] for s in segs if s != "rc16")}
# name -> (the segment the tampering needs or None, the tampering)
TAMPERINGS = {
    "nothing": (None, lambda p: None),
    "a phase-1 value of pedersen": ("pedersen", lambda p: _set(("queries", 0, "phase1", 0, "values", COL0["pedersen"](p["segments"]) + 1), flip)(p)),
    "a phase-1 value of ecdsa": ("ecdsa", lambda p: _set(("queries", 1, "phase1", 2, "values", COL0["ecdsa"](p["segments"]) + 9), flip)(p)),
    "a phase-1 value of rc16": ("rc16", lambda p: _set(("queries", 0, "phase1", 3, "values", COL0["rc16"](p["segments"]) + 2), flip)(p)),
    "a phase-1 path node": (None, _set(("queries", 1, "phase1", 3, "path", 4), flip)),
    "a phase-2 value": ("rc16", _set(("queries", 1, "phase2", 2, "value"), flip)),
    "a phase-2 path node": ("rc16", _set(("queries", 0, "phase2", 1, "path", 0), flip)),
    "phase2_root": ("rc16", _set(("phase2_root",), flip)),
    "a layer value": (None, _set(("queries", 1, "layers", 2, 0, "value"), flip)),
    "a layer path node": (None, _set(("queries", 1, "layers", 1, 1, "path", 0), flip)),
    "a final-layer value": (None, _set(("final_layer", 5), flip)),
    "a layer root": (None, _set(("layer_roots", 0), flip)),
    "the seed": (None, _set(("seed",), lambda v: v + 1)),
    "rc_max - 1": ("rc16", _set(("public_inputs", "rc_max"), lambda v: v - 1)),
    "a signature's r = 0": ("ecdsa", _set(("public_inputs", "signatures", 0, 1), lambda v: 0)),
    "a swapped pair": (None, _swap_pair),
    "a wrong phase-1 row": (None, _set(("queries", 0, "phase1", 2, "row"), lambda v: v + 1)),
    "a wrong phase-2 row": ("rc16", _set(("queries", 1, "phase2", 0, "row"), lambda v: v + 1)),
    "a wrong index": (None, _set(("queries", 1, "index"), flip)),
    "a phase-1 row with one value dropped": (None, _drop_value),
}
E2E = [(segs, what) for segs in PROOFS for what, (needs, _) in sorted(TAMPERINGS.items()) if needs is None or needs in segs]


def test_the_end_to_end_table_is_whole():
    assert len(TAMPERINGS) == 20 and len(E2E) == 20 + 17 + 18 + 13
    assert {what for segs, what in E2E if segs == ("pedersen", "ecdsa", "rc16")} == set(TAMPERINGS)


@pytest.mark.parametrize("segments,what", E2E, ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_verify_builtins_agrees_with_the_oracle(gpu, segments, what):
    torch, lib, stark = gpu
    final_log = PROOFS[segments][4]
    proof = copy.deepcopy(proof_of(segments))
    TAMPERINGS[what][1](proof)
    want = S.verify_builtins_proof(proof, hash2=chash, final_log=final_log)
    assert stark.verify_builtins(proof, final_log=final_log) == want, (segments, what)
    assert want == (True, "ok") if what == "nothing" else not want[0]
    if what == "nothing":
        nq = PROOFS[segments][3]
        assert stark.verify_builtins(proof, final_log=final_log, n_queries=nq) == (True, "ok")
        assert stark.verify_builtins(proof, final_log=final_log, n_queries=nq + 1) == (False, "shape")


@pytest.mark.parametrize("segments", sorted(PROOFS), ids=set_id)
def test_openings_of_an_honest_proof_are_all_true_in_proof_order(gpu, segments):
    torch, lib, stark = gpu
    proof = proof_of(segments)
    got = stark.check_builtins_openings(proof)
    two = "rc16" in segments
    labels = []
    for qi, q in enumerate(proof["queries"]):
        for k, t in enumerate(q["phase1"]):
            labels.append("q%d/phase1/row %d" % (qi, t["row"]))
            if two:
                labels.append("q%d/phase2/row %d" % (qi, q["phase2"][k]["row"]))
        for k, pair in enumerate(q["layers"]):
            labels += ["q%d/layer %d/pos %d" % (qi, k, o["pos"]) for o in pair]
    assert [label for label, _ in got] == labels and all(ok for _, ok in got)
    assert len(got) == len(proof["queries"]) * ((8 if two else 4) + 2 * len(proof["layer_roots"]))
    bad = copy.deepcopy(proof)
    bad["queries"][0]["layers"][1][0]["value"] ^= 1
    if two:
        bad["queries"][1]["phase2"][3]["path"][2] ^= 1
    wrong = [label for label, ok in stark.check_builtins_openings(bad) if not ok]
    assert wrong == ["q0/layer 1/pos %d" % bad["queries"][0]["layers"][1][0]["pos"]] + (
        ["q1/phase2/row %d" % bad["queries"][1]["phase2"][3]["row"]] if two else [])


# ---- forged proofs that only the algebra can catch -------------------------------------------------------------------
def forge(stark, hashes, signatures, values, final_log, n_queries, bad_z=False, bad_alpha=None, bad_beta_layer=None, seed=5):
    """_commit_builtins and _query_builtins written out with the module's public pieces for the three segments at
    n = 1024, with one dishonest step: the product column and the rc16 composition made with z + 1, ONE alpha + 1 in
    the composition, or ONE layer folded with beta + 1.  Every commitment and opening is honest about the columns the
    forger holds, so the Merkle checks pass and only the algebra can tell."""
    import torch
    shift, n = stark.FIELD_GEN, 1024
    M = 4 * n
    segments = ["pedersen", "ecdsa", "rc16"]
    padded, rc_min, rc_max = stark.rc16_fill(list(values), n // 8)
    (sz, sr, ss, sq), = signatures
    public = {"rc_min": rc_min, "rc_max": rc_max, "signatures": [[sz, sr, ss, sq[0], sq[1]]]}
    flat_pub = [3, 0, 1, 2, rc_min, rc_max, sz, sr, ss, sq[0], sq[1]]
    ft = lambda vals: stark.felts_to_tensor(vals, "cuda")
    hs = [hashes[i % len(hashes)] for i in range(n // 512)]
    trace = torch.cat([stark.pedersen_trace(ft([x for x, _ in hs]), ft([y for _, y in hs])),
                       stark.ecdsa_trace(ft([sz]), ft([sr]), ft([pow(ss, -1, stark.EC_ORDER)]), ft([sq[0]]), ft([sq[1]])),
                       stark.rc16_columns(ft(padded))])
    assert trace.shape[0] == 17 and trace.shape[1] == n
    tr = stark.Transcript("builtins", n, shift, seed, flat_pub)
    trace_lde = stark.lde(trace)
    lv1 = stark.commit_rows(trace_lde)
    root1 = stark.root_of(lv1)
    tr.absorb("phase1_root", root1)
    z = tr.challenge("rc16_z")
    z_used = (z + 1) % P if bad_z else z
    p_lde = stark.lde(stark.rc16_product(trace[14], trace[16], z_used).unsqueeze(0))[0]
    lv2 = stark.commit_rows(p_lde.unsqueeze(0))
    root2 = stark.root_of(lv2)
    tr.absorb("phase2_root", root2)
    alphas = [tr.challenge("alpha", k) for k in range(45)]
    if bad_alpha is not None:
        alphas[bad_alpha] = (alphas[bad_alpha] + 1) % P
    per = lambda seg: stark.periodic_lde(n, shift, "cuda", seg)
    comp = stark.air_eval(trace_lde[0:4], per("pedersen"), n, alphas[:11], shift, "pedersen")
    comp = stark.felt_add(comp, stark.air_eval(trace_lde[4:14], per("ecdsa"), n, alphas[11:37], shift, "ecdsa"))
    comp = stark.felt_add(comp, stark.air_eval_rc16(trace_lde[14:17], p_lde, per("rc16"), n, alphas[37:], z_used, rc_min,
                                                    rc_max, shift))
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
    tables = [(trace_lde, lv1), (p_lde, lv2)] + list(zip(layers[:-1], bufs))
    indices = [tr.challenge("query", q, modulus=M // 2) for q in range(n_queries)]
    picks = []
    for j in indices:
        for pos in (j, j + M // 2):
            for r in (pos, (pos + 4) % M):
                picks += [(0, r), (1, r)]
        for k in range(len(bufs)):
            mk = M >> k
            picks += [(2 + k, j % (mk // 2)), (2 + k, j % (mk // 2) + mk // 2)]
    opened = iter(zip(picks, stark.open_rows(tables, picks)))
    queries = []
    for j in indices:
        q = {"index": j, "phase1": [], "phase2": [], "layers": []}
        for _ in range(4):
            (_, row), (vals, _, path) = next(opened)
            q["phase1"].append({"row": row, "values": vals, "path": path})
            (_, row), (vals, _, path) = next(opened)
            q["phase2"].append({"row": row, "value": vals[0], "path": path})
        for _ in bufs:
            q["layers"].append([{"pos": pos, "value": vals[0], "path": path}
                                for (_, pos), (vals, _, path) in (next(opened), next(opened))])
        queries.append(q)
    return {"n": n, "air": "builtins", "segments": segments, "seed": seed, "shift": shift, "public_inputs": public,
            "phase1_root": root1, "phase2_root": root2, "layer_roots": roots, "final_layer": final, "queries": queries}


FORGERIES = {"honest": ({}, "ok"), "z + 1": ({"bad_z": True}, "composition value"),
             "the last alpha + 1": ({"bad_alpha": 44}, "composition value"),
             "alpha 0 + 1": ({"bad_alpha": 0}, "composition value"),
             "beta + 1 at layer 2": ({"bad_beta_layer": 2}, "fold consistency at layer 2")}


@pytest.mark.parametrize("what", sorted(FORGERIES))
def test_forged_proofs_fail_on_the_algebra_alone(gpu, what):
    torch, lib, stark = gpu
    hashes, signatures, values = instances(random.Random(78), 2, 1, 16)
    kw, reason = FORGERIES[what]
    proof = forge(stark, hashes, signatures, values, 6, 3, **kw)  # log_m 12, 6 layers: layer 2 is a middle one
    assert all(ok for _, ok in stark.check_builtins_openings(proof))
    want = (reason == "ok", reason)
    assert stark.verify_builtins(proof) == want == S.verify_builtins_proof(proof, hash2=chash)
    if what == "honest":
        assert proof == stark.prove_builtins(hashes, signatures, values, n_queries=3, seed=5)  # the forge is the prover
