"""The builtins verifier without a GPU: the per-point logic of sp_builtins_eval_points_dev (csrc/verify_builtins.hpp)
built by g++ (tests/host/builtins_verify_shim.cpp replays the kernel's launch plan - one wave per present segment,
lane by lane - over host arrays) against the integer expectations of tests/builtins_verify_cases.py; the stand-alone
form of the shim under -fsanitize=address,undefined, run directly; the header and the binding; and
stark.verify_builtins on malformed proofs and on the answers that are decided on the host, which must come before the
library is initialised."""
import copy
import ctypes
import os
import subprocess

import numpy as np
import pytest

import builtins_verify_cases as B
from test_verify_cpu import malformations as trace_malformations

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "builtins_verify_shim.cpp")
SETS = B.SEGMENT_SETS
set_id = "+".join


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "host", "builtins_verify_shim.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    for name in ("bvs_n_cols", "bvs_n_alpha", "bvs_block_threads"):
        getattr(lib, name).restype = ctypes.c_uint
        getattr(lib, name).argtypes = [ctypes.c_uint]
    lib.bvs_points.restype = ctypes.c_int
    lib.bvs_points.argtypes = [ctypes.c_uint, ctypes.c_uint] + [ctypes.c_void_p] * 6 + [
        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t] + [ctypes.c_void_p] * 8 + [ctypes.c_size_t]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def run_points(shim, case, pos, cur, nxt, pcur, pnxt, mask=None, log_n=None, rc_min=None, rc_max=None, z=None, extra=3):
    """The shim on sentinel-filled outputs of len(pos) + extra items: (rc, values, statuses, tail untouched, text)."""
    n = len(pos)
    out = np.full((n + extra, 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    status = np.full(n + extra, 0xEE, dtype=np.uint8)
    err = ctypes.create_string_buffer(128)
    pers = [case.per_np(s) for s in B.SEG_NAMES]
    alphas, shift = B.felts_np(case.alphas), B.felts_np([B.SHIFT])
    zz = B.felts_np([case.z if z is None else z])
    rc = shim.bvs_points(case.mask if mask is None else mask, case.log_n if log_n is None else log_n, ptr(pers[0]),
                         ptr(pers[1]), ptr(pers[2]), ptr(alphas), ptr(shift), ptr(zz),
                         case.rc_min if rc_min is None else rc_min, case.rc_max if rc_max is None else rc_max, n,
                         ptr(pos), ptr(cur), ptr(nxt), ptr(pcur) if case.has_rc else None,
                         ptr(pnxt) if case.has_rc else None, ptr(out), ptr(status), err, 128)
    vals, st = B.ints_of(out), status.tolist()
    clean = vals[n:] == [int.from_bytes(b"\xaa" * 32, "little")] * extra and st[n:] == [0xEE] * extra
    return rc, vals[:n], st[:n], clean, err.value.decode()


# ---- the case builder keeps its promises -----------------------------------------------------------------------------
@pytest.mark.parametrize("segments", SETS, ids=set_id)
def test_cases_hold_the_edges(segments):
    c = B.builtins_case(segments)
    M = c.M
    assert c.log_n == max({"pedersen": 9, "ecdsa": 10, "rc16": 3}[s] for s in segments) and M == 4 << c.log_n
    assert c.n_cols == sum({"pedersen": 4, "ecdsa": 10, "rc16": 3}[s] for s in segments)
    assert c.n_alpha == sum({"pedersen": 11, "ecdsa": 26, "rc16": 8}[s] for s in segments)
    assert len(c.positions) == 257 and all(0 <= p < M for p in c.positions)
    if M <= 257:
        assert set(c.positions) == set(range(M))
    for p in (0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1, M // 2 - 1, M // 2):
        assert p in c.positions
    assert {p % 32 for p in c.positions} >= {0, 31}
    assert set(B.EXTREMES) <= {v for col in c.cols for v in col}
    # random rows make every segment's value non-zero: the sum is not the sum of fewer segments
    honest = [p for p in c.positions[:64]]
    for p in honest[:8]:
        parts = c.parts(p, *c.rows(p))
        assert set(parts) == set(segments) and 0 not in parts.values()
    if segments == ("rc16",):
        assert len(c.pers["rc16"][0]) == M == 32  # the periodic table is exactly M rows
        dense = B.S.rc16_composition_on_coset(c.cols, c.pcol, c.n, c.alphas, c.z, c.rc_min, c.rc_max, B.SHIFT)
        assert [dense[p] for p in c.positions] == c.expected and len(dense) == M


# ---- the shim against the integers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", SETS, ids=set_id)
def test_shim_matches_the_integers(shim, segments):
    c = B.builtins_case(segments)
    assert shim.bvs_n_cols(c.mask) == c.n_cols and shim.bvs_n_alpha(c.mask) == c.n_alpha
    assert shim.bvs_block_threads(c.mask) == 64 * len(segments)  # one wave per present segment
    for count in B.ITEM_COUNTS:
        pos, cur, nxt, pcur, pnxt, want = c.arrays(count)
        rc, out, status, clean, err = run_points(shim, c, pos, cur, nxt, pcur, pnxt)
        assert rc == 0 and clean, err
        assert status == [B.POINT_OK] * count
        assert out == want, (segments, count)


@pytest.mark.parametrize("segments", SETS, ids=set_id)
def test_shim_flags_out_of_range_items(shim, segments):
    c = B.builtins_case(segments)
    items = c.bad_items()
    rc, out, status, clean, err = run_points(shim, c, *c.pack(items))
    assert rc == 0 and clean, err
    assert status == [B.POINT_OK if it[5] is not None else B.POINT_OUT_OF_RANGE for it in items]
    assert out == [it[5] or 0 for it in items]  # the neighbours' values are unchanged
    assert status.count(B.POINT_OUT_OF_RANGE) == c.n_bad() == 2 + 2 * c.n_cols + (2 if c.has_rc else 0) + 3
    assert status[0] == status[-1] == B.POINT_OK and all(it[5] for it in items if it[5] is not None)


def test_shim_argument_rules(shim):
    c = B.builtins_case(("rc16",))
    pos, cur, nxt, pcur, pnxt, want = c.arrays(5)
    assert run_points(shim, c, pos, cur, nxt, pcur, pnxt)[:2] == (0, want)
    table = B.refused_scalars()
    assert len(table) == 2 + 14 + 3
    for what, word, kw in table:
        # the bounds are checked before any table or row is read: the rc16 case's arrays serve every mask
        rc, _, _, clean, err = run_points(shim, c, pos, cur, nxt, pcur, pnxt, **kw)
        assert rc == -3 and clean and word in err, (what, err)
    for segs, lo, hi in ((("pedersen",), 9, 30), (("ecdsa",), 10, 30), (("rc16",), 3, 24), (("pedersen", "rc16"), 9, 24),
                         (("pedersen", "ecdsa"), 10, 30)):
        assert (B.min_log_n(segs), B.max_log_n(segs)) == (lo, hi)
    for bad_shift_case in (0, 1, B.P - 1, B.P, pow(3, (B.P - 1) // 32, B.P)):
        out = np.full((8, 4), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
        status = np.full(8, 0xEE, dtype=np.uint8)
        err = ctypes.create_string_buffer(128)
        per, alphas, zz, sh = c.per_np("rc16"), B.felts_np(c.alphas), B.felts_np([c.z]), B.felts_np([bad_shift_case])
        rc = shim.bvs_points(4, 3, None, None, ptr(per), ptr(alphas), ptr(sh), ptr(zz), 3, 40000, 5, ptr(pos), ptr(cur),
                             ptr(nxt), ptr(pcur), ptr(pnxt), ptr(out), ptr(status), err, 128)
        assert rc == -3 and "shift" in err.value.decode() and status.tolist() == [0xEE] * 8
    # a count of 0 is SP_OK with nothing written, whatever the pointers
    rc, out, status, clean, _ = run_points(shim, c, pos[:0], cur[:0], nxt[:0], pcur[:0], pnxt[:0])
    assert rc == 0 and out == [] and status == [] and clean
    err = ctypes.create_string_buffer(128)
    assert shim.bvs_points(7, 10, *[None] * 6, 0, 1, 0, *[None] * 7, err, 128) == 0
    assert shim.bvs_points(7, 10, *[None] * 6, 0, 1, 1, *[None] * 7, err, 128) == -3 and b"NULL" in err.value
    assert shim.bvs_points(7, 10, *[None] * 6, 0, 1, (1 << 30) + 1, *[None] * 7, err, 128) == -3 and b"2^30" in err.value


def test_shim_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "builtins_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DBUILTINS_SHIM_MAIN", "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "builtins verify check passed" in run.stdout, run.stdout + run.stderr


# ---- the binding and the header --------------------------------------------------------------------------------------
def test_header_and_binding_name_the_call():
    from starkperp import _lib, stark
    text = open(os.path.join(os.path.dirname(HERE), "include", "starkperp.h")).read()
    assert "sp_builtins_eval_points_dev(" in text and "sp_builtins_eval_points_dev" in _lib.declared_symbols()
    for seg, bit in B.SEG_BITS.items():
        assert "#define SP_SEG_%s %d" % (seg.upper(), bit) in text
    assert stark.SEG_BITS == B.SEG_BITS and tuple(stark.BUILTIN_SEGMENTS) == B.SEG_NAMES
    assert stark.AIR_IDS == {"pedersen": 0, "ec_ladder": 1, "ecdsa": 2, "range_check": 3}  # the single-AIR call stays


# ---- stark.verify_builtins on malformed proofs: "malformed", nothing raised, the library never initialised -----------
SIG = [1, 1, 1, B.S.R.EC_GEN[0], B.S.R.EC_GEN[1]]


def skeleton(segments=("pedersen", "ecdsa", "rc16"), n=1024, final_log=6, n_queries=2):
    """A prove_builtins-shaped dict with every key and every length right (its contents are not a proof)."""
    from starkperp import stark
    log_m = n.bit_length() + 1
    n_layers = log_m - final_log
    n_cols = sum(stark.AIRS[s]["n_cols"] for s in segments)
    has_rc = "rc16" in segments
    q = {"index": 5, "phase1": [{"row": 5, "values": [1] * n_cols, "path": [2] * log_m} for _ in range(4)],
         "phase2": [{"row": 5, "value": 6, "path": [2] * log_m} for _ in range(4)] if has_rc else [],
         "layers": [[{"pos": 1, "value": 3, "path": [4] * (log_m - k)} for _ in range(2)] for k in range(n_layers)]}
    pub = {}
    if has_rc:
        pub.update({"rc_min": 0, "rc_max": 9})
    if "ecdsa" in segments:
        pub["signatures"] = [list(SIG) for _ in range(n // 1024)]
    return {"n": n, "air": "builtins", "segments": list(segments), "seed": 0, "shift": 3, "public_inputs": pub,
            "phase1_root": 11, "phase2_root": 13 if has_rc else None, "layer_roots": [12] * n_layers,
            "final_layer": [0] * (1 << final_log), "queries": [copy.deepcopy(q) for _ in range(n_queries)]}


def test_the_skeleton_itself_is_wellformed():
    from starkperp import stark
    for segments in SETS:
        assert stark._wellformed_builtins(skeleton(segments)), segments
    assert stark._wellformed_builtins(skeleton(("rc16",), 8, 3))


def malformations():
    """The malformations of test_verify_cpu.malformations() carried over to the keys of a builtins proof (trace ->
    phase1, trace_root -> phase1_root; its public inputs are a dict, so those four are restated), and the ones
    that only this proof has."""
    out = {}
    for name, f in trace_malformations().items():
        if name.startswith("public input") or name in ("n below the period", "too few values"):
            continue  # restated below / answered with a reason here ("public inputs", "opened rows")

        def g(p, f=f):
            """f on the same objects under the single-AIR proof's names; what f removed stays removed."""
            queries = p["queries"]
            p["trace_root"] = p.pop("phase1_root")
            for q in queries:
                q["trace"] = q.pop("phase1")
            r = f(p)
            if "trace_root" in p:
                p["phase1_root"] = p.pop("trace_root")
            for q in queries:
                if "trace" in q:
                    q["phase1"] = q.pop("trace")
            return r
        out[name.replace("trace", "phase1")] = g

    def put(path, value):
        def f(p):
            o = p
            for k in path[:-1]:
                o = o[k]
            o[path[-1]] = value
        return f

    def drop(path):
        def f(p):
            o = p
            for k in path[:-1]:
                o = o[k]
            del o[path[-1]]
        return f
    t2 = ("queries", 1, "phase2", 2)
    out["segments a string"] = put(("segments",), "pedersen")
    out["segments with a number"] = put(("segments", 1), 2)
    out["no segments"] = drop(("segments",))
    out["air of a single-AIR proof"] = put(("air",), "pedersen")
    out["phase2 opening without value"] = drop(t2 + ("value",))
    out["phase2 opening without row"] = drop(t2 + ("row",))
    out["phase2 opening without path"] = drop(t2 + ("path",))
    out["phase2 value p"] = put(t2 + ("value",), B.P)
    out["phase2 path short"] = put(t2 + ("path",), [2] * 11)
    out["phase2 path node float"] = put(t2 + ("path", 3), 2.0)
    out["three phase2 openings"] = lambda p: p["queries"][0]["phase2"].pop()
    out["query without phase2"] = drop(("queries", 0, "phase2"))
    out["phase2_root missing with rc16"] = drop(("phase2_root",))
    out["phase2_root None with rc16"] = put(("phase2_root",), None)
    out["phase2_root p"] = put(("phase2_root",), B.P)
    out["public_inputs a list"] = put(("public_inputs",), [0, 9])
    out["no public_inputs"] = drop(("public_inputs",))
    out["no rc_max"] = drop(("public_inputs", "rc_max"))
    out["rc_min str"] = put(("public_inputs", "rc_min"), "0")
    out["no signatures"] = drop(("public_inputs", "signatures"))
    out["a signature of four"] = lambda p: p["public_inputs"]["signatures"][0].pop()
    out["a signature value 2^256"] = put(("public_inputs", "signatures", 0, 3), 2**256)
    out["a signature value str"] = put(("public_inputs", "signatures", 0, 0), "1")
    out["phase1 value p in the last column"] = put(("queries", 0, "phase1", 1, "values", 16), B.P)
    out["n 2^25 with rc16"] = put(("n",), 1 << 25)
    return out


def test_the_carried_over_malformations_are_all_there():
    names = set(malformations())
    assert len(names) == len(trace_malformations()) - 4 + 25
    for must in ("not a dict", "no phase1_root", "query without phase1", "phase1 opening without values",
                 "phase1_root p", "phase1 value float", "path node 2^256", "n not a power of two", "shift a power of w_4n",
                 "phase1 path short", "three phase1 openings", "a pair of three", "queries not a list",
                 "a query with a layer missing"):
        assert must in names, must


@pytest.mark.parametrize("name", sorted(malformations()))
def test_verify_builtins_answers_malformed_without_the_library(name):
    from starkperp import _lib, stark
    proof = skeleton()
    mutated = malformations()[name](proof)
    if name == "not a dict":
        proof = mutated
    assert stark.verify_builtins(proof) == (False, "malformed"), name
    assert _lib._lib is None or not _lib._lib.sp_is_initialised()


def test_host_only_answers_come_before_the_device_and_equal_the_oracle():
    """"segments", "public inputs" and "shape" are decided on the host, in the oracle's order, before anything is
    initialised; the oracle gives the same reason on the same dict."""
    from starkperp import _lib, stark

    def both(p, reason, **kw):
        assert stark.verify_builtins(p, **kw) == (False, reason), reason
        assert B.S.verify_builtins_proof(p, **kw) == (False, reason), reason
    for segs in (["ecdsa", "pedersen", "rc16"], [], ["pedersen", "ec_ladder"], ["rc16", "rc16"]):
        p = skeleton()
        p["segments"] = segs
        both(p, "segments")
    p = skeleton()
    p["public_inputs"]["rc_max"] = 65536
    both(p, "public inputs")
    p = skeleton()
    p["public_inputs"]["rc_min"] = 10  # above rc_max
    both(p, "public inputs")
    p = skeleton()
    p["public_inputs"]["signatures"][0][2] = 0  # s = 0
    both(p, "public inputs")
    p = skeleton()
    p["public_inputs"]["signatures"][0][1] = 0  # r = 0
    both(p, "public inputs")
    p = skeleton()
    p["public_inputs"]["signatures"].append(list(SIG))  # one signature too many for n = 1024
    both(p, "public inputs")
    p = skeleton(("pedersen",), 8, 3)  # n = 8 with pedersen listed
    both(p, "public inputs")
    p = skeleton(("rc16",), 4, 2)  # n below one range-checked value
    both(p, "public inputs")
    p = skeleton()
    both(p, "shape", final_log=7)
    assert stark.verify_builtins(p, n_queries=3) == (False, "shape")
    p["final_layer"] = p["final_layer"][:-1]
    both(p, "shape")
    p = skeleton(("rc16",), 8, 3)
    both(p, "shape", final_log=5)  # log_m = 5: no layer would be left
    assert stark.verify_builtins(p, final_log=6) == (False, "shape")
    assert stark.verify_builtins(skeleton(), final_log="6") == (False, "malformed")
    assert _lib._lib is None or not _lib._lib.sp_is_initialised()


def test_verify_still_refuses_builtins_proofs_and_names_the_verifier():
    from starkperp import stark
    with pytest.raises(ValueError, match="builtins verifier.*verify_builtins"):
        stark.verify(skeleton())
