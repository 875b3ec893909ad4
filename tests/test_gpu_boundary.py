"""Boundary constraints from a descriptor, on the GPU: the two kernels of csrc/boundary.hip against the integers of
tests/boundary_ref.py (dense column at every index, points at every position, coefficient arrays below, at and above
one block's stride, statuses, argument edges) and, with the pedersen_io descriptor, bit for bit against the hand-written
kernels of csrc/hash_io.hip; then stark.prove_signatures / verify_signatures and prove_ranges / verify_ranges end to
end - round trips that the integer verifier accepts too, the gap the unbound proofs leave and its closing, tampered
and malformed proofs, one 2^18-row proof."""
import copy
import ctypes
import random

import pytest

import boundary_ref as B
import workloads as wl
from oracle import ref_py as R
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
P = S.P
OTHER_SHIFT = 0x5A17C0FFEE5A17C0FFEE5A17C0FFEE5A17C0FFEE
FILL = int("aa" * 32, 16)
DENSE_CASES = [("ecdsa_io", 1024), ("ecdsa_io", 2048), ("range_check_io", 128), ("range_check_io", 256),
               ("range_check_io", 512)]
# the widest descriptor the calls take, terms out of group order (no AIR of the project: the argument rules' limit)
WIDEST = {"period": 256, "n_cols": 16, "rows": (255, 0, 7, 128),
          "terms": ((15, 3), (0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 2), (6, 0))}


@pytest.fixture(scope="module")
def stark():
    from starkperp import stark as st
    return st


def c_hash(a, b):
    from oracle import cref
    return cref.pedersen_hash_many([a], [b])[0][0]


def mixed(count, seed):
    """0, 1, p - 1 and the other extreme limb patterns (0.85) among random felts: the mix of
    test_prover_kernels_on_extreme_limb_patterns."""
    rng = random.Random(seed)
    ext = wl.extreme_felts()
    return [rng.choice(ext) if rng.random() < 0.85 else rng.randrange(P) for _ in range(count)]


def dev_cols(stark, cols):
    import torch
    return torch.stack([stark.felts_to_tensor(c) for c in cols])


def host_cols(stark, t):
    return [stark.tensor_to_felts(c) for c in t]


def signatures(k, seed):
    """(zs, rs, ss, public keys) of k signatures the reference accepts, signed on the GPU."""
    from starkperp import batch
    rng = random.Random(seed)
    keys = [rng.randrange(1, R.EC_ORDER) for _ in range(k)]
    zs = [rng.randrange(1, 2**251) for _ in range(k)]
    sigs = batch.sign_many(zs, keys)
    return zs, [r for r, _ in sigs], [s for _, s in sigs], [tuple(q) for q in batch.public_keys_many(keys)]


def public_of(zs, rs, ss, pubs):
    return [v for z, r, s, q in zip(zs, rs, ss, pubs) for v in (z, r, s, q[0], q[1])]


def honest_trace(stark, name, k, seed):
    """(trace, public inputs) of an honest witness of k instances."""
    if name == "ecdsa_io":
        zs, rs, ss, pubs = signatures(k, seed)
        ws = [pow(s, -1, R.EC_ORDER) for s in ss]
        trace = stark.ecdsa_trace(*(stark.felts_to_tensor(v) for v in (zs, rs, ws, [q[0] for q in pubs],
                                                                       [q[1] for q in pubs])))
        return trace, public_of(zs, rs, ss, pubs)
    rng = random.Random(seed)
    values = [rng.randrange(1 << 128) for _ in range(k)]
    return stark.range_check_trace(stark.felts_to_tensor(values)), values


@pytest.fixture(scope="module")
def honest(stark):
    """(name, n) -> what the dense and points tests share, computed once: an honest trace LDE (device and integers),
    its public inputs, the boundary challenges and the integer boundary column at the default shift."""
    out = {}
    for name, n in DENSE_CASES:
        desc = B.DESCRIPTORS[name]
        trace, pub = honest_trace(stark, name, n // desc["period"], n)
        trace_lde = stark.lde(trace)
        ints = host_cols(stark, trace_lde)
        rng = random.Random(n + 1)
        alphas = [rng.randrange(P) for _ in desc["terms"]]
        values = B.term_values(name, pub)
        want = B.boundary_on_coset(desc, ints, B.public_columns_lde(desc, values, n, alphas), n, alphas)
        out[name, n] = {"pub": pub, "values": values, "trace": trace, "trace_lde": trace_lde, "ints": ints,
                        "alphas": alphas, "want": want}
    return out


# ---- the dense call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", DENSE_CASES)
def test_public_columns_and_dense_boundary_on_an_honest_trace(stark, honest, name, n):
    h, desc = honest[name, n], B.DESCRIPTORS[name]
    assert stark.boundary_term_values(name, h["pub"]) == h["values"]
    for (c, d), v in zip(desc["terms"], h["values"]):  # the trace holds the statement where the descriptor says
        assert stark.tensor_to_felts(h["trace"][c, desc["rows"][d]::desc["period"]]) == v
    pub_lde = stark.boundary_public_lde(name, h["values"], n, h["alphas"])
    assert host_cols(stark, pub_lde) == B.public_columns_lde(desc, h["values"], n, h["alphas"])
    got = stark.boundary(name, h["trace_lde"], pub_lde, n, h["alphas"])
    assert stark.tensor_to_felts(got) == h["want"]
    assert S.poly_degree_bound_check(h["want"], S.GEN, n - 1)


@pytest.mark.parametrize("name,n", DENSE_CASES)
def test_dense_boundary_acc_modes(stark, honest, name, n):
    """acc NULL is the test above; here acc distinct from out (and left as it was) and acc aliased to out."""
    h = honest[name, n]
    pub_lde = stark.boundary_public_lde(name, h["values"], n, h["alphas"])
    acc = mixed(4 * n, n + 2)
    summed = [(a + b) % P for a, b in zip(acc, h["want"])]
    acc_t = stark.felts_to_tensor(acc)
    got = stark.boundary(name, h["trace_lde"], pub_lde, n, h["alphas"], acc=acc_t)
    assert stark.tensor_to_felts(got) == summed and stark.tensor_to_felts(acc_t) == acc
    same = stark.boundary(name, h["trace_lde"], pub_lde, n, h["alphas"], acc=acc_t, out=acc_t)
    assert same.data_ptr() == acc_t.data_ptr() and stark.tensor_to_felts(acc_t) == summed


@pytest.mark.parametrize("name,n,shift", [(name, n, s) for name, n in DENSE_CASES for s in (S.GEN, OTHER_SHIFT)]
                         + [("widest", 256, S.GEN), ("widest", 512, OTHER_SHIFT)])
def test_dense_boundary_on_arbitrary_columns(stark, name, n, shift):
    """The column is a pointwise function of whatever the arrays hold: extreme limb patterns in the trace columns, the
    public columns, acc and the challenges; the default and another shift."""
    desc = WIDEST if name == "widest" else B.DESCRIPTORS[name]
    cols = [mixed(4 * n, 20 * n + c) for c in range(desc["n_cols"])]
    pub_lde = [mixed(4 * n, 20 * n + 16 + c) for c in range(len(desc["rows"]))]
    alphas, acc = mixed(len(desc["terms"]), 20 * n + 5), mixed(4 * n, 20 * n + 6)
    want = B.boundary_on_coset(desc, cols, pub_lde, n, alphas, shift)
    got = stark.boundary(desc if name == "widest" else name, dev_cols(stark, cols), dev_cols(stark, pub_lde), n, alphas,
                         shift, acc=stark.felts_to_tensor(acc))
    assert stark.tensor_to_felts(got) == [(a + b) % P for a, b in zip(acc, want)]


@pytest.mark.parametrize("name,n", (("ecdsa_io", 1024), ("range_check_io", 256)))
def test_dense_boundary_with_a_shifted_honest_trace(stark, honest, name, n):
    """A non-default shift end to end: public columns extended with it, the trace LDE on the same coset."""
    h, desc = honest[name, n], B.DESCRIPTORS[name]
    trace_lde = stark.lde(h["trace"], shift=OTHER_SHIFT)
    pub_lde = stark.boundary_public_lde(name, h["values"], n, h["alphas"], OTHER_SHIFT)
    want = B.boundary_on_coset(desc, host_cols(stark, trace_lde),
                               B.public_columns_lde(desc, h["values"], n, h["alphas"], OTHER_SHIFT), n, h["alphas"],
                               OTHER_SHIFT)
    assert stark.tensor_to_felts(stark.boundary(name, trace_lde, pub_lde, n, h["alphas"], OTHER_SHIFT)) == want
    assert S.poly_degree_bound_check(want, OTHER_SHIFT, n - 1)


def test_dense_boundary_reads_columns_col_stride_apart(stark, honest):
    """A trace LDE that is a view into a wider allocation: the stride is the view's, not M."""
    import torch
    name, n = "ecdsa_io", 1024
    h = honest[name, n]
    wide = torch.zeros((10, 4 * n + 3, 4), dtype=torch.int64, device="cuda")
    wide[:, :4 * n] = h["trace_lde"]
    pub_lde = stark.boundary_public_lde(name, h["values"], n, h["alphas"])
    assert stark.tensor_to_felts(stark.boundary(name, wide[:, :4 * n], pub_lde, n, h["alphas"])) == h["want"]


# ---- the cross-check against the hand-written kernels ----------------------------------------------------------------
@pytest.mark.parametrize("n", (512, 1024))
def test_pedersen_descriptor_equals_the_hash_io_kernels_bit_for_bit(stark, n):
    import torch
    k = n // 512
    rng = random.Random(n)
    xs, ys = [rng.randrange(P) for _ in range(k)], [rng.randrange(P) for _ in range(k)]
    trace = stark.pedersen_trace(stark.felts_to_tensor(xs), stark.felts_to_tensor(ys))
    pub = [v for t in zip(xs, ys, stark.tensor_to_felts(trace[1, 511::512])) for v in t]
    values = stark.boundary_term_values("pedersen_io", pub)
    alphas = [rng.randrange(P) for _ in range(3)]
    acc = stark.felts_to_tensor(mixed(4 * n, n))
    for shift in (S.GEN, OTHER_SHIFT):
        trace_lde = stark.lde(trace, shift=shift)
        old = stark.hash_io_boundary(trace_lde, stark.hash_io_public_lde(pub, n, shift), n, alphas, shift, acc=acc)
        new = stark.boundary("pedersen_io", trace_lde, stark.boundary_public_lde("pedersen_io", values, n, alphas, shift), n,
                             alphas, shift, acc=acc)
        assert torch.equal(old, new)
        pos = torch.arange(4 * n, dtype=torch.int64, device="cuda")
        cur = trace_lde.permute(1, 0, 2).contiguous()
        old_p, old_st = stark.hash_io_boundary_points(n, stark.hash_io_coefficients(pub, n), alphas, shift, pos, cur)
        new_p, new_st = stark.boundary_points("pedersen_io", n, stark.boundary_coefficients("pedersen_io", values, n, alphas),
                                              alphas, shift, pos, cur)
        assert torch.equal(old_p, new_p) and torch.equal(old_st, new_st)
        assert torch.equal(new_p, stark.boundary("pedersen_io", trace_lde,
                                                 stark.boundary_public_lde("pedersen_io", values, n, alphas, shift), n,
                                                 alphas, shift))


# ---- the points call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", DENSE_CASES)
def test_points_equal_the_dense_column_at_every_position(stark, honest, name, n):
    import torch
    h, desc = honest[name, n], B.DESCRIPTORS[name]
    M = 4 * n
    coef = stark.boundary_coefficients(name, h["values"], n, h["alphas"])
    assert host_cols(stark, coef) == B.public_coefficients(desc, h["values"], n, h["alphas"])
    pos = torch.arange(M, dtype=torch.int64, device="cuda")
    cur = h["trace_lde"].permute(1, 0, 2).contiguous()
    out, status = stark.boundary_points(name, n, coef, h["alphas"], S.GEN, pos, cur)
    assert status.cpu().tolist() == [stark.POINT_OK] * M
    assert stark.tensor_to_felts(out) == h["want"]


@pytest.mark.parametrize("name", ("ecdsa_io", "range_check_io", "widest"))
@pytest.mark.parametrize("k", (1, 2, 128, 256, 512, 4096))
def test_points_from_coefficient_arrays_alone(stark, name, k):
    """No trace: coefficient arrays below, at and above one block's stride of 256 against Horner in integers, eight
    points each (both ends of the coset among them), extreme limb patterns in the coefficients and the rows."""
    import torch
    desc = WIDEST if name == "widest" else B.DESCRIPTORS[name]
    n = desc["period"] * k
    coeffs = [mixed(k, 3 * k + c) for c in range(len(desc["rows"]))]
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in desc["terms"]]
    pos = [0, 1, 4 * n - 1, 2 * n] + [rng.randrange(4 * n) for _ in range(4)]
    cur = [mixed(desc["n_cols"], 7 * k + i) for i in range(8)]
    out, status = stark.boundary_points(desc if name == "widest" else name, n, dev_cols(stark, coeffs), alphas,
                                        OTHER_SHIFT, torch.tensor(pos, dtype=torch.int64, device="cuda"),
                                        dev_cols(stark, cur))
    assert status.cpu().tolist() == [stark.POINT_OK] * 8
    assert stark.tensor_to_felts(out) == [B.boundary_at(desc, n, coeffs, alphas, OTHER_SHIFT, p, c)
                                          for p, c in zip(pos, cur)]


def test_points_status_and_neighbours(stark):
    import torch
    n, desc = 2048, B.DESCRIPTORS["ecdsa_io"]
    coeffs = [mixed(2, c) for c in range(3)]
    alphas = [2, 3, 4, 5, 6]
    pos = [5, 4 * n, 6, -1, 7, 8, 9]          # -1 is 2^64 - 1 to the library
    cur = [list(range(1, 11)) for _ in pos]
    cur[5][9] = P                              # a felt of the row that the value does not even use
    cur[6][0] = (1 << 256) - 1
    out, status = stark.boundary_points("ecdsa_io", n, dev_cols(stark, coeffs), alphas, S.GEN,
                                        torch.tensor(pos, dtype=torch.int64, device="cuda"), dev_cols(stark, cur))
    ok, bad = stark.POINT_OK, stark.POINT_OUT_OF_RANGE
    assert status.cpu().tolist() == [ok, bad, ok, bad, ok, bad, bad]
    got = stark.tensor_to_felts(out)
    for i in (0, 2, 4):
        assert got[i] == B.boundary_at(desc, n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [got[i] for i in (1, 3, 5, 6)] == [0] * 4


# ---- argument edges of both C calls -------------------------------------------------------------------------------------
DESCRIPTOR_RULES = (({"log_period": 6}, "log_period"), ({"log_period": 11}, "log_period"), ({"n_cols": 0}, "n_cols"),
                    ({"n_cols": 17}, "n_cols"), ({"n_groups": 0}, "n_groups"), ({"n_groups": 5}, "n_groups"),
                    ({"n_terms": 0}, "n_terms"), ({"n_terms": 9}, "n_terms"), ({"group_rows": None}, "group_rows"),
                    ({"term_cols": None}, "term_cols"), ({"term_groups": None}, "term_groups"),
                    ({"group_rows": [0, 256, 1024]}, "group_rows"), ({"group_rows": [0, 256, 256]}, "group_rows"),
                    ({"term_cols": [0, 0, 3, 10, 0]}, "term_cols"), ({"term_groups": [0, 1, 1, 1, 3]}, "term_groups"),
                    ({"term_groups": [0, 1, 1, 1, 1]}, "without a term"))


def descriptor(**over):
    """The seven descriptor arguments of the ECDSA descriptor, fields replaced by `over`."""
    d = dict(log_period=10, n_cols=10, n_groups=3, group_rows=[0, 256, 512], n_terms=5, term_cols=[0, 0, 3, 4, 0],
             term_groups=[0, 1, 1, 1, 2])
    d.update(over)
    arr = lambda v: None if v is None else (ctypes.c_uint * len(v))(*v)
    return [d["log_period"], d["n_cols"], d["n_groups"], arr(d["group_rows"]), d["n_terms"], arr(d["term_cols"]),
            arr(d["term_groups"])]


def test_argument_edges(stark, honest):
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    h = honest["ecdsa_io", 1024]
    M = 4096
    pack = _lib.pack_felts
    trace, pub = h["trace_lde"], stark.boundary_public_lde("ecdsa_io", h["values"], 1024, h["alphas"])
    out = stark.felts_to_tensor([FILL] * M)
    on_domain = S.root_of_unity(12)  # w_4n at n = 1024: shift^(4n) = 1
    five = pack([1, 2, 3, 4, 5])

    def dense(log_n=10, shift=3, trace_p=trace.data_ptr(), stride=M, pub_p=pub.data_ptr(), alphas=five,
              out_p=out.data_ptr(), **over):
        shift_p = None if shift is None else pack([shift])
        return lib.sp_boundary_dev(*descriptor(**over), trace_p, stride, pub_p, log_n, alphas, shift_p, None, out_p,
                                   stark._stream())
    edges = [(over, word) for over, word in DESCRIPTOR_RULES] + [
        ({"log_n": 9}, "log_n"), ({"log_n": 25}, "log_n"), ({"shift": 0}, "shift"), ({"shift": 1}, "shift"),
        ({"shift": on_domain}, "shift"), ({"shift": P}, "shift"), ({"shift": None}, "shift_host"),
        ({"trace_p": None}, "trace_lde"), ({"pub_p": None}, "pub_lde"), ({"alphas": None}, "alphas_host"),
        ({"out_p": None}, "out"), ({"stride": M - 1}, "col_stride"),
        ({"log_period": 7, "n_cols": 1, "n_groups": 1, "group_rows": [0], "n_terms": 1, "term_cols": [0],
          "term_groups": [0], "log_n": 6}, "log_n")]  # the lower bound is the descriptor's own period
    for kwargs, word in edges:
        assert dense(**kwargs) == -3, kwargs
        err = _lib.last_error()
        assert err.startswith("sp_boundary_dev") and word in err, (kwargs, err)
    torch.cuda.synchronize()
    assert set(stark.tensor_to_felts(out)) == {FILL}

    coef = stark.boundary_coefficients("ecdsa_io", h["values"], 1024, h["alphas"])
    pos = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    cur = dev_cols(stark, [list(range(1, 11)), list(range(11, 21))])
    pout = stark.felts_to_tensor([FILL] * 2)
    status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")

    def points(log_n=10, shift=3, n_points=2, coef_p=coef.data_ptr(), alphas=five, pos_p=pos.data_ptr(),
               cur_p=cur.data_ptr(), out_p=pout.data_ptr(), status_p=status.data_ptr(), **over):
        shift_p = None if shift is None else pack([shift])
        return lib.sp_boundary_points_dev(*descriptor(**over), log_n, coef_p, alphas, shift_p, n_points, pos_p, cur_p,
                                          out_p, status_p, stark._stream())
    edges = [(over, word) for over, word in DESCRIPTOR_RULES] + [
        ({"log_n": 9}, "log_n"), ({"log_n": 31}, "log_n"), ({"shift": 0}, "shift"), ({"shift": 1}, "shift"),
        ({"shift": on_domain}, "shift"), ({"shift": P}, "shift"), ({"shift": None}, "shift_host"),
        ({"coef_p": None}, "coef"), ({"alphas": None}, "alphas_host"), ({"pos_p": None}, "pos"), ({"cur_p": None}, "cur"),
        ({"out_p": None}, "out"), ({"status_p": None}, "status"), ({"n_points": (1 << 30) + 1}, "n_points")]
    for kwargs, word in edges:
        assert points(**kwargs) == -3, kwargs
        err = _lib.last_error()
        assert err.startswith("sp_boundary_points_dev") and word in err, (kwargs, err)
    # nothing to do is SP_OK, whatever the pointers
    assert points(n_points=0, coef_p=None, pos_p=None, cur_p=None, out_p=None, status_p=None) == 0
    torch.cuda.synchronize()
    assert set(stark.tensor_to_felts(pout)) == {FILL} and status.cpu().tolist() == [0xEE, 0xEE]


def test_log_n_at_its_bounds_is_accepted(stark):
    """One inside each bound the edges above step over: log_n = log_period for both calls (the dense tests run it),
    log_n = 30 for the points call - k = 2^20 coefficients per group, 4096 Horner steps a lane.  log_n = 24 of the
    dense call is 2^26 points of every column and is left to tools/quick_boundary.py."""
    import torch
    desc = B.DESCRIPTORS["ecdsa_io"]
    k, n = 1 << 20, 1 << 30
    coef = torch.zeros((3, k, 4), dtype=torch.int64, device="cuda")
    sparse = {0: 5, 1: 7, 255: 11, 256: 13, k - 1: 17}
    for d in range(3):
        for i, v in sparse.items():
            coef[d, i, 0] = v + d
    alphas = [3, 5, 7, 11, 13]
    pos = [0, 1, 4 * n - 1, 3 * n + 12345]
    cur = [mixed(10, i) for i in range(4)]
    out, status = stark.boundary_points("ecdsa_io", n, coef, alphas, S.GEN, torch.tensor(pos, dtype=torch.int64,
                                                                                         device="cuda"),
                                        dev_cols(stark, cur))
    assert status.cpu().tolist() == [stark.POINT_OK] * 4
    g, wp, w = S.root_of_unity(30), S.root_of_unity(10), S.root_of_unity(32)
    want = []
    for p_, c in zip(pos, cur):  # boundary_at with sparse polynomials
        x = S.GEN * pow(w, p_, P) % P
        num = []
        for d, o in enumerate(desc["rows"]):
            y = x * pow(g, -o, P) % P
            num.append(-sum((v + d) * pow(y, i, P) for i, v in sparse.items()))
        for (col, d), a in zip(desc["terms"], alphas):
            num[d] += a * c[col]
        want.append(sum(u * pow((pow(x, k, P) - pow(wp, o, P)) % P, -1, P) for u, o in zip(num, desc["rows"])) % P)
    assert stark.tensor_to_felts(out) == want


# ---- prove_signatures / verify_signatures, prove_ranges / verify_ranges ----------------------------------------------
@pytest.fixture(scope="module")
def sig_proofs(stark):
    """k -> (signatures, proof) with three queries, proved once."""
    out = {}
    for k in (1, 2, 4):
        sigs = signatures(k, 40 + k)
        out[k] = (sigs, stark.prove_signatures(*sigs, n_queries=3, seed=7 + k))
    return out


@pytest.fixture(scope="module")
def range_proofs(stark):
    out = {}
    for k in (1, 4, 16):
        rng = random.Random(50 + k)
        values = [0, (1 << 128) - 1][:k] + [rng.randrange(1 << 128) for _ in range(max(k - 2, 0))]
        out[k] = (values, stark.prove_ranges(values, n_queries=3, seed=9 + k))
    return out


@pytest.mark.parametrize("k", (1, 2, 4))
def test_signatures_round_trip(stark, sig_proofs, k):
    sigs, proof = sig_proofs[k]
    assert proof["air"] == "ecdsa_io" and proof["n"] == 1024 * k and len(proof["queries"]) == 3
    assert proof["public_inputs"] == public_of(*sigs)
    for z, r, s, q in zip(*sigs):
        assert R.verify(z, r, s, q)
    assert stark.verify_signatures(proof) == (True, "ok")
    assert stark.verify_signatures(proof, n_queries=3) == (True, "ok")
    assert stark.verify_signatures(proof, n_queries=4) == (False, "shape")
    assert B.verify_proof_bound(proof, hash2=c_hash) == (True, "ok")
    # the unbound verifier does not know this AIR, and the siblings take no other
    assert stark.verify(proof) == (False, "malformed")
    assert stark.verify_ranges(proof) == (False, "malformed") and stark.verify_hashes(proof) == (False, "malformed")


@pytest.mark.parametrize("k", (1, 4, 16))
def test_ranges_round_trip(stark, range_proofs, k):
    values, proof = range_proofs[k]
    assert proof["air"] == "range_check_io" and proof["n"] == 128 * k and proof["public_inputs"] == values
    assert stark.verify_ranges(proof) == (True, "ok")
    assert stark.verify_ranges(proof, n_queries=3) == (True, "ok")
    assert stark.verify_ranges(proof, n_queries=2) == (False, "shape")
    assert B.verify_proof_bound(proof, hash2=c_hash) == (True, "ok")
    assert stark.verify(proof) == (False, "malformed") and stark.verify_signatures(proof) == (False, "malformed")


def test_unbound_proofs_are_refused_and_unchanged(stark):
    """prove_ecdsa / prove_range_checks still make the proofs stark.verify takes; the new verifiers refuse them."""
    sigs = signatures(1, 5)
    proof = stark.prove_ecdsa(*sigs, n_queries=2)
    assert proof["air"] == "ecdsa" and stark.verify(proof) == (True, "ok")
    assert stark.verify_signatures(proof) == (False, "malformed")
    # relabelled: the transcript, hence every challenge, is another one
    assert not stark.verify_signatures(dict(proof, air="ecdsa_io"))[0]
    proof = stark.prove_range_checks([5, 6], n_queries=2)
    assert proof["air"] == "range_check" and stark.verify(proof) == (True, "ok")
    assert stark.verify_ranges(proof) == (False, "malformed")
    assert not stark.verify_ranges(dict(proof, air="range_check_io"))[0]


def lying_claims(sigs, which):
    """The public inputs of `sigs` with one field of the first signature replaced by another admissible one."""
    zs, rs, ss, pubs = sigs
    claim = public_of(zs, rs, ss, pubs)
    if which == "z":
        claim[0] = claim[0] + 1 if claim[0] + 1 < 2**251 else claim[0] - 1
    elif which == "r":
        claim[1] = claim[1] + 1 if claim[1] + 1 < 2**251 else claim[1] - 1
    elif which == "s":
        s = claim[2]
        while True:  # another s with 1 <= s^-1 mod N < 2^251, as the statement rules ask
            s = s % (R.EC_ORDER - 1) + 1
            if s != claim[2] and pow(s, -1, R.EC_ORDER) < 2**251:
                break
        claim[2] = s
    else:
        claim[3], claim[4] = R.private_key_to_ec_point_on_stark_curve(0xC0FFEE)  # another curve point
    return claim


@pytest.mark.parametrize("which", ("z", "r", "s", "key"))
def test_the_gap_and_its_closing_for_signatures(stark, which):
    """The ladders run on signature A, the published tuple is B.  The unbound proof is accepted; the bound prover, as
    consistent about B as it can be (transcript, composition and FRI all use the claim), makes a quotient that is no
    polynomial, and the 16 top coefficients of the final layer vanish with probability p^-16: both verifiers say
    "final layer degree"."""
    sigs = signatures(1, 60)
    zs, rs, ss, pubs = sigs
    claim = lying_claims(sigs, which)
    assert claim != public_of(*sigs)
    ws = [pow(s, -1, R.EC_ORDER) for s in ss]
    trace = stark.ecdsa_trace(*(stark.felts_to_tensor(v) for v in (zs, rs, ws, [q[0] for q in pubs], [q[1] for q in pubs])))
    unbound = stark.prove_trace(trace, "ecdsa", n_queries=3, seed=1, public_inputs=claim)
    assert unbound["public_inputs"] == claim and stark.verify(unbound) == (True, "ok")
    proof = stark.prove_signatures(*sigs, n_queries=3, seed=1, claims=claim)
    assert proof["public_inputs"] == claim
    assert stark.verify_signatures(proof) == (False, "final layer degree")
    assert B.verify_proof_bound(proof, hash2=c_hash) == (False, "final layer degree")


def test_the_gap_and_its_closing_for_ranges(stark):
    values = [12345, (1 << 128) - 1, 0, 77]
    claim = [12345, (1 << 128) - 1, 1, 77]
    trace = stark.range_check_trace(stark.felts_to_tensor(values))
    unbound = stark.prove_trace(trace, "range_check", n_queries=3, seed=1, public_inputs=claim)
    assert stark.verify(unbound) == (True, "ok")
    proof = stark.prove_ranges(values, n_queries=3, seed=1, claims=claim)
    assert proof["public_inputs"] == claim
    assert stark.verify_ranges(proof) == (False, "final layer degree")
    assert B.verify_proof_bound(proof, hash2=c_hash) == (False, "final layer degree")


def tamperings(proof, per):
    """(name, tampered proof, the reason when it is certain) - those of test_gpu_hash_io.py, and the statement
    edited after the fact; `per` = public inputs per instance."""
    def edit(fn):
        bad = copy.deepcopy(proof)
        fn(bad)
        return bad

    def flip_trace(b): b["queries"][0]["trace"][0]["values"][0] ^= 1
    def flip_layer(b): b["queries"][1]["layers"][2][0]["value"] ^= 1
    def flip_final(b): b["final_layer"][5] ^= 1
    def flip_root(b): b["layer_roots"][0] ^= 1
    def bump_seed(b): b["seed"] += 1
    def one_input(b): b["public_inputs"] = [1]
    def other_first(b): b["public_inputs"][0] ^= 1
    def other_last(b): b["public_inputs"][-1 if per == 1 else -4] ^= 2   # a value | r of the last signature
    def swap(b): b["public_inputs"] = b["public_inputs"][per:2 * per] + b["public_inputs"][:per] + b["public_inputs"][2 * per:]
    def short_list(b): b["public_inputs"] = b["public_inputs"][:-per]
    def long_list(b): b["public_inputs"] = b["public_inputs"] + b["public_inputs"][:per]
    return [("trace value", edit(flip_trace), "trace path"), ("layer value", edit(flip_layer), None),
            ("final layer", edit(flip_final), "final layer degree"), ("layer root", edit(flip_root), None),
            ("seed", edit(bump_seed), None), ("one public input", edit(one_input), "public inputs"),
            ("another first input", edit(other_first), None), ("another last input", edit(other_last), None),
            ("swapped instances", edit(swap), None), ("short list", edit(short_list), "public inputs"),
            ("long list", edit(long_list), "public inputs")]


def test_tampered_signature_proofs_are_rejected_with_the_reference_reason(stark, sig_proofs):
    _, proof = sig_proofs[2]
    cases = tamperings(proof, 5)
    off_curve = copy.deepcopy(proof)
    off_curve["public_inputs"][4] ^= 1
    cases.append(("a key off the curve", off_curve, "public inputs"))
    for name, bad, reason in cases:
        got = stark.verify_signatures(bad)
        want = B.verify_proof_bound(bad, hash2=c_hash)
        assert not got[0] and got == want, (name, got, want)
        if reason:
            assert got[1] == reason, (name, got)


def test_tampered_range_proofs_are_rejected_with_the_reference_reason(stark, range_proofs):
    _, proof = range_proofs[4]
    cases = tamperings(proof, 1)
    wide = copy.deepcopy(proof)
    wide["public_inputs"][2] = 1 << 128
    cases.append(("a value of 129 bits", wide, "public inputs"))
    for name, bad, reason in cases:
        got = stark.verify_ranges(bad)
        want = B.verify_proof_bound(bad, hash2=c_hash)
        assert not got[0] and got == want, (name, got, want)
        if reason:
            assert got[1] == reason, (name, got)


@pytest.mark.parametrize("which", ("signatures", "ranges"))
def test_malformed_inputs_never_raise(stark, sig_proofs, range_proofs, which):
    proof = sig_proofs[1][1] if which == "signatures" else range_proofs[4][1]
    verify = stark.verify_signatures if which == "signatures" else stark.verify_ranges
    period = 1024 if which == "signatures" else 128
    n_cols = 10 if which == "signatures" else 1

    class Hostile(dict):
        def get(self, *a):
            raise RuntimeError("inspected")
    cases = [None, 7, [], {}, Hostile(proof), {"air": proof["air"]}, dict(proof, air=None), dict(proof, n=proof["n"] + 1),
             dict(proof, n=period // 2), dict(proof, n=str(proof["n"])), dict(proof, shift=0), dict(proof, shift=1),
             dict(proof, shift=P), dict(proof, seed=-1), dict(proof, trace_root=P), dict(proof, public_inputs=None),
             dict(proof, public_inputs=[1.5, 2, 3]), dict(proof, public_inputs=[1 << 256, 2, 3]),
             dict(proof, final_layer=[P] * 64), dict(proof, queries=None), dict(proof, queries=[{}]),
             {k: v for k, v in proof.items() if k != "layer_roots"}]
    bad = copy.deepcopy(proof)
    bad["queries"][0]["trace"][2]["values"] = bad["queries"][0]["trace"][2]["values"] + [1]
    assert len(bad["queries"][0]["trace"][2]["values"]) == n_cols + 1
    cases.append(bad)
    bad = copy.deepcopy(proof)
    bad["queries"][2]["layers"][1][1]["path"].append(5)
    cases.append(bad)
    bad = copy.deepcopy(proof)
    bad["queries"][1]["layers"].pop()
    cases.append(bad)
    for i, case in enumerate(cases):
        assert verify(case) == (False, "malformed"), i
    assert verify(proof, final_log="6") == (False, "malformed")
    assert verify(dict(proof, layer_roots=proof["layer_roots"][:-1])) == (False, "shape")
    assert verify(proof, final_log=5) == (False, "shape")


def test_a_proof_of_256_signatures(stark):
    """n = 2^18 rows: accepted, and rejected once a published r is another one."""
    sigs = signatures(256, 23)
    proof = stark.prove_signatures(*sigs, n_queries=4, seed=3)
    assert proof["n"] == 1 << 18 and len(proof["public_inputs"]) == 5 * 256 and len(proof["layer_roots"]) == 14
    assert stark.verify_signatures(proof, n_queries=4) == (True, "ok")
    bad = dict(proof, public_inputs=list(proof["public_inputs"]))
    bad["public_inputs"][5 * 200 + 1] ^= 1
    assert not stark.verify_signatures(bad)[0]
