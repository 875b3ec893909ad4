"""The verifier without a GPU: the per-item logic of sp_air_eval_points_dev and sp_fri_check_queries_dev
(csrc/verify.hpp) built by g++ (tests/host/verify_shim.cpp replays the kernels' launch plans lane by lane over host
arrays) against the integer expectations of tests/verify_cases.py; the stand-alone form of the shim under
-fsanitize=address,undefined, run directly; the case builders' own promises; and stark.verify on malformed proofs, which
must answer "malformed" before the library is initialised."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import verify_cases as V

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "verify_shim.cpp")
AIRS = ("range_check", "ec_ladder", "pedersen", "ecdsa")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "verify_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    lib.vs_blocks.restype = lib.vs_next_side.restype = ctypes.c_uint
    lib.vs_blocks.argtypes = [ctypes.c_size_t]
    lib.vs_layer_pos.restype = ctypes.c_uint64
    lib.vs_layer_pos.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint64]
    lib.vs_next_side.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint64]
    lib.vs_is_felt.restype = ctypes.c_int
    lib.vs_is_felt.argtypes = [ctypes.c_void_p]
    lib.vs_points.restype = lib.vs_fri.restype = ctypes.c_int
    lib.vs_points.argtypes = [ctypes.c_int, ctypes.c_uint] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [
        ctypes.c_void_p] * 6 + [ctypes.c_size_t]
    lib.vs_fri.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [
        ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    return lib


def run_points(shim, case, pos, cur, nxt, log_n=None, air_id=None):
    n = len(pos)
    out = np.full((n, 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(n, 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(128)
    per, alphas, shift = case.per_np(), V.felts_np(case.alphas), V.felts_np([V.SHIFT])
    rc = shim.vs_points(V.AIR_IDS[case.air] if air_id is None else air_id,
                        V.MIN_LOG_N[case.air] if log_n is None else log_n, per.ctypes.data, alphas.ctypes.data,
                        shift.ctypes.data, n, pos.ctypes.data, cur.ctypes.data, nxt.ctypes.data, out.ctypes.data,
                        status.ctypes.data, err, 128)
    return rc, V.ints_of(out), status.tolist(), err.value.decode()


def run_fri(shim, case, log_m=None, n_layers=None):
    index, pairs, final, betas = case.arrays()
    status = np.full(len(index) * case.n_layers, 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(128)
    shift = V.felts_np([V.SHIFT])
    rc = shim.vs_fri(case.log_m if log_m is None else log_m, case.n_layers if n_layers is None else n_layers,
                     shift.ctypes.data, betas.ctypes.data, len(index), index.ctypes.data, pairs.ctypes.data,
                     final.ctypes.data, status.ctypes.data, err, 128)
    return rc, status.reshape(len(index), case.n_layers).tolist(), err.value.decode()


# ---- the case builders keep their promises ---------------------------------------------------------------------------
@pytest.mark.parametrize("air", AIRS)
def test_air_cases_hold_the_edges(air):
    c = V.air_case(air)
    M = c.M
    assert c.n == V.S.AIRS[air]["period"] and M == {"range_check": 512, "ec_ladder": 1024, "pedersen": 2048,
                                                    "ecdsa": 4096}[air]
    assert len(c.positions) == 257 and all(0 <= p < M for p in c.positions)
    # at the smallest size 4 * period IS M: the position after the periodic table's last entry is 0 again
    for p in (0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1, 4 * c.n - 1, M // 2 - 1, M // 2):
        assert p in c.positions[:12]
    flat = {v for col in c.cols for v in col}
    assert set(V.EXTREMES) <= flat
    # random rows make every constraint term non-zero: the value is not the value of zeroed alphas
    assert len(set(c.expected)) >= len(set(c.positions)) - 2 and 0 not in c.expected[:12]
    # the integer composition of the oracle at a few whole positions
    dense = V.S.composition_on_coset(c.cols, c.per, c.n, c.alphas, V.SHIFT, air) if air != "ecdsa" else None
    if dense is not None:
        assert [dense[p] for p in c.positions] == c.expected


@pytest.mark.parametrize("shape", V.FRI_SHAPES)
def test_fri_cases_hold_the_edges(shape):
    c = V.fri_case(*shape)
    m = 1 << c.log_m
    assert 0 in c.index and m // 2 - 1 in c.index
    honest = [q for q, note in enumerate(c.notes) if note == "honest"]
    assert all(c.expected[q] == [V.FOLD_OK] * c.n_layers for q in honest)
    for k in range(c.n_layers):  # both sides of a quarter of layer k
        mk = m >> k
        sides = {(c.index[q] % (mk // 2)) < mk // 4 for q in honest}
        assert sides == {True, False}
        assert {c.index[q] % (mk // 2) for q in honest} >= {mk // 4 - 1, mk // 4}
    assert any(a + b >= V.P for q in honest for a, b in c.pairs[q])
    assert any(a == b for q, pr in enumerate(c.pairs) for a, b in pr if c.notes[q].startswith("a == b"))
    for q, k in c.single.items():
        want = [V.FOLD_OK] * c.n_layers
        want[k] = V.FOLD_MISMATCH
        assert c.expected[q] == want, c.notes[q]
    assert len(c.single) >= (3 if c.n_layers >= 3 else 2)
    for q, note in enumerate(c.notes):
        if note == "index >= m / 2":
            assert c.expected[q] == [V.FOLD_OUT_OF_RANGE] * c.n_layers
        if ">= p" in note:
            assert V.FOLD_OUT_OF_RANGE in c.expected[q] and c.expected[q] != [V.FOLD_OUT_OF_RANGE] * c.n_layers or \
                c.n_layers == 1
    if c.n_layers >= 3:
        a_eq_b = c.notes.index("a == b at layer 0")
        assert c.expected[a_eq_b][0] == V.FOLD_OK


# ---- the shim against the integers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("air", AIRS)
def test_points_shim_matches_the_integers(shim, air):
    c = V.air_case(air)
    for count in V.ITEM_COUNTS:
        pos, cur, nxt, want = c.arrays(count)
        rc, out, status, err = run_points(shim, c, pos, cur, nxt)
        assert rc == 0, err
        assert status == [V.POINT_OK] * count
        assert out == want, (air, count)
    assert shim.vs_blocks(1) == 1 and shim.vs_blocks(64) == 1 and shim.vs_blocks(65) == 2 and shim.vs_blocks(257) == 5


@pytest.mark.parametrize("air", AIRS)
def test_points_shim_flags_out_of_range_items(shim, air):
    c = V.air_case(air)
    items = c.bad_items()
    pos = np.array([it[0] for it in items], dtype=np.uint64)
    cur = V.felts_np([v for it in items for v in it[1]])
    nxt = V.felts_np([v for it in items for v in it[2]])
    rc, out, status, err = run_points(shim, c, pos, cur, nxt)
    assert rc == 0, err
    assert status == [V.POINT_OK if it[3] is not None else V.POINT_OUT_OF_RANGE for it in items]
    assert out == [it[3] or 0 for it in items]
    assert status.count(V.POINT_OUT_OF_RANGE) == 4 + 2 * c.n_cols


def test_points_shim_argument_rules(shim):
    c = V.air_case("range_check")
    pos, cur, nxt, _ = c.arrays(1)
    for air_id in (-1, 4, 99):
        assert run_points(shim, c, pos, cur, nxt, air_id=air_id)[0] == -3
    for air, lo in V.MIN_LOG_N.items():
        case = V.air_case("range_check")  # the bounds are checked before any table is read
        assert run_points(shim, case, pos, cur, nxt, log_n=lo - 1, air_id=V.AIR_IDS[air])[0] == -3
        assert run_points(shim, case, pos, cur, nxt, log_n=31, air_id=V.AIR_IDS[air])[0] == -3
    rc, out, status, _ = run_points(shim, c, pos[:0], cur[:0], nxt[:0])
    assert rc == 0 and out == [] and status == []


@pytest.mark.parametrize("shape", V.FRI_SHAPES)
def test_fri_shim_matches_the_integers(shim, shape):
    c = V.fri_case(*shape)
    rc, status, err = run_fri(shim, c)
    assert rc == 0, err
    for q, (got, want) in enumerate(zip(status, c.expected)):
        assert got == want, (q, c.notes[q], c.index[q])
    for k in range(c.n_layers):
        for j in c.index:
            if j < 1 << (c.log_m - 1):
                jk = j % (1 << (c.log_m - k - 1))
                assert shim.vs_layer_pos(c.log_m, k, j) == jk
                if k + 1 < c.n_layers:
                    assert shim.vs_next_side(c.log_m, k, jk) == (0 if jk < 1 << (c.log_m - k - 2) else 1)


def test_fri_shim_argument_rules(shim):
    c = V.fri_case(7, 1)
    for log_m, n_layers in ((7, 0), (7, 7), (7, 8), (33, 1), (1, 1), (0, 0)):
        assert run_fri(shim, c, log_m, n_layers)[0] == -3
    for v in (0, V.P, 2**256 - 1):
        arr = V.felts_np([v])
        assert shim.vs_is_felt(arr.ctypes.data) == (1 if v < V.P else 0)


def test_shim_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DVERIFY_SHIM_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "verify check passed" in run.stdout, run.stdout + run.stderr


# ---- the binding and the header --------------------------------------------------------------------------------------
def test_header_and_binding_name_the_two_calls():
    from starkperp import _lib
    text = open(os.path.join(os.path.dirname(HERE), "include", "starkperp.h")).read()
    for name in ("sp_air_eval_points_dev", "sp_fri_check_queries_dev"):
        assert name + "(" in text and name in _lib.declared_symbols()
    for air, k in V.AIR_IDS.items():
        assert "#define SP_AIR_%s %d" % (air.upper(), k) in text
    from starkperp import stark
    assert stark.AIR_IDS == V.AIR_IDS
    assert (stark.FOLD_OK, stark.FOLD_MISMATCH, stark.FOLD_OUT_OF_RANGE) == (0, 1, 2)


# ---- stark.verify on malformed proofs: "malformed", nothing raised, the library never initialised --------------------
def skeleton(air="range_check", n=128, final_log=5, n_queries=2):
    """A proof-shaped dict with every key and every length right (its contents are not a proof)."""
    from starkperp import stark
    log_m = n.bit_length() + 1
    n_layers = log_m - final_log
    n_cols = stark.AIRS[air]["n_cols"]
    q = {"index": 5, "trace": [{"row": 5, "values": [1] * n_cols, "path": [2] * log_m} for _ in range(4)],
         "layers": [[{"pos": 1, "value": 3, "path": [4] * (log_m - k)} for _ in range(2)] for k in range(n_layers)]}
    return {"n": n, "air": air, "seed": 0, "shift": 3, "public_inputs": [7], "trace_root": 11,
            "layer_roots": [12] * n_layers, "final_layer": [0] * (1 << final_log),
            "queries": [copy.deepcopy(q) for _ in range(n_queries)]}


def test_the_skeleton_itself_is_wellformed():
    from starkperp import stark
    assert stark._wellformed(skeleton())
    assert stark._wellformed(skeleton("ecdsa", 1024, 6))


def malformations():
    P = V.P

    def drop(path):
        def f(p):
            o = p
            for k in path[:-1]:
                o = o[k]
            del o[path[-1]]
        return f

    def put(path, value):
        def f(p):
            o = p
            for k in path[:-1]:
                o = o[k]
            o[path[-1]] = value
        return f
    q0, t0, o0 = ("queries", 0), ("queries", 0, "trace", 1), ("queries", 1, "layers", 2, 1)
    out = {"not a dict": lambda p: None}
    for key in ("n", "seed", "shift", "trace_root", "layer_roots", "final_layer", "queries"):
        out["no " + key] = drop((key,))
    for key in ("index", "trace", "layers"):
        out["query without " + key] = drop(q0 + (key,))
    for key in ("row", "values", "path"):
        out["trace opening without " + key] = drop(t0 + (key,))
    for key in ("pos", "value", "path"):
        out["layer opening without " + key] = drop(o0 + (key,))
    for name, bad in (("float", 1.0), ("str", "1"), ("None", None), ("bool", True), ("negative", -1), ("p", P),
                      ("2^256", 2**256)):
        out["trace_root " + name] = put(("trace_root",), bad)
        out["trace value " + name] = put(t0 + ("values", 0), bad)
        out["path node " + name] = put(o0 + ("path", 0), bad)
        out["layer value " + name] = put(o0 + ("value",), bad)
        out["final felt " + name] = put(("final_layer", 3), bad)
        out["layer root " + name] = put(("layer_roots", 1), bad)
    for name, bad in (("float", 128.0), ("str", "128"), ("not a power of two", 129), ("below the period", 64), ("0", 0),
                      ("too long", 1 << 31)):
        out["n " + name] = put(("n",), bad)
    for name, bad in (("0", 0), ("1", 1), ("p - 1", P - 1), ("p", P), ("a power of w_4n", pow(3, (P - 1) // 512, P))):
        out["shift " + name] = put(("shift",), bad)
    out["seed 2^256"] = put(("seed",), 2**256)
    out["row str"] = put(t0 + ("row",), "5")
    out["pos float"] = put(o0 + ("pos",), 1.0)
    out["index None"] = put(q0 + ("index",), None)
    out["public input str"] = put(("public_inputs", 0), "7")
    out["public input 2^256"] = put(("public_inputs", 0), 2**256)
    out["unknown air"] = put(("air",), "rc16")
    out["air not a string"] = put(("air",), 3)
    out["trace path short"] = put(t0 + ("path",), [2] * 8)
    out["trace path long"] = put(t0 + ("path",), [2] * 10)
    out["layer path short"] = put(o0 + ("path",), [4] * 6)
    out["three trace openings"] = lambda p: p["queries"][0]["trace"].pop()
    out["a pair of three"] = lambda p: p["queries"][0]["layers"][0].append(p["queries"][0]["layers"][0][0])
    out["too few values"] = put(t0 + ("values",), [])
    out["a query with a layer missing"] = lambda p: p["queries"][1]["layers"].pop()
    out["queries not a list"] = put(("queries",), {"0": 1})
    return out


@pytest.mark.parametrize("name", sorted(malformations()))
def test_verify_answers_malformed_without_the_library(name):
    from starkperp import _lib, stark
    proof = skeleton()
    mutated = malformations()[name](proof)
    if name == "not a dict":
        proof = mutated
    assert stark.verify(proof, final_log=5) == (False, "malformed"), name
    assert _lib._lib is None or not _lib._lib.sp_is_initialised()


def test_verify_statement_and_shape_answers_come_before_the_device():
    """"public inputs" and "shape" are decided on the host, in the oracle's order, before anything is initialised."""
    from starkperp import _lib, stark
    p = skeleton()
    p["public_inputs"] = [2**128]
    assert stark.verify(p, final_log=5) == (False, "public inputs")
    assert V.S.verify_proof(p, final_log=5)[1] == "public inputs"
    p = skeleton()
    p["public_inputs"] = []
    assert stark.verify(p, final_log=5) == (False, "public inputs")
    e = skeleton("ecdsa", 1024, 6)
    e["public_inputs"] = [1, 1, 0, 1, 1]  # s = 0
    assert stark.verify(e) == (False, "public inputs") and V.S.verify_proof(e)[1] == "public inputs"
    p = skeleton()
    p["public_inputs"] = [7]
    assert stark.verify(p, final_log=6) == (False, "shape") and V.S.verify_proof(p, final_log=6)[1] == "shape"
    assert stark.verify(p, final_log=5, n_queries=3) == (False, "shape")
    p["final_layer"] = p["final_layer"][:-1]
    assert stark.verify(p, final_log=5) == (False, "shape")
    assert stark.verify(p, final_log="5") == (False, "malformed")
    assert _lib._lib is None or not _lib._lib.sp_is_initialised()


def test_verify_refuses_builtins_proofs_by_name():
    from starkperp import stark
    with pytest.raises(ValueError, match="builtins verifier"):
        stark.verify({"air": "builtins", "n": 1024})
