"""Pedersen proofs that bind their statement, on the GPU: the two kernels of csrc/hash_io.hip against the integers of
tests/hash_io_ref.py (dense column at every index, points at every position, coefficient arrays below, at and above
one block's stride, statuses, argument edges), and stark.prove_hashes / verify_hashes end to end - round trips that
the integer verifier accepts too, a consistently lying prover, tampered and malformed proofs."""
import copy
import ctypes
import random

import pytest

import hash_io_ref as H
import workloads as wl
from oracle import ref_py as R
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
P = S.P
SIZES = (512, 1024, 2048)
OTHER_SHIFT = 0x5A17C0FFEE5A17C0FFEE5A17C0FFEE5A17C0FFEE
FILL = int("aa" * 32, 16)


@pytest.fixture(scope="module")
def stark():
    from starkperp import stark as st
    return st


def c_hash(a, b):
    from oracle import cref
    return cref.pedersen_hash_many([a], [b])[0][0]


def hash_inputs(k, seed):
    rng = random.Random(seed)
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(k)]


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


@pytest.fixture(scope="module")
def honest(stark):
    """n -> what the dense and points tests share, computed once: an honest trace LDE (device and integers), its public
    inputs, the three boundary challenges and the integer boundary column at the default shift."""
    out = {}
    for n in SIZES:
        inputs = hash_inputs(n // 512, n)
        trace = stark.pedersen_trace(stark.felts_to_tensor([x for x, _ in inputs]),
                                     stark.felts_to_tensor([y for _, y in inputs]))
        pub = H.public_inputs(inputs, stark.tensor_to_felts(trace[1, 511::512]))
        trace_lde = stark.lde(trace)
        ints = host_cols(stark, trace_lde)
        alphas = [random.Random(n + 1).randrange(P) for _ in range(3)]
        want = H.boundary_on_coset(ints, H.public_columns_lde(pub, n), n, alphas)
        out[n] = {"inputs": inputs, "pub": pub, "trace_lde": trace_lde, "ints": ints, "alphas": alphas, "want": want}
    return out


# ---- the dense call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_public_columns_and_dense_boundary_on_an_honest_trace(stark, honest, n):
    h = honest[n]
    assert h["pub"][2::3] == [c_hash(x, y) for x, y in h["inputs"]]  # px at row 512 i + 511 is the hash
    pub_lde = stark.hash_io_public_lde(h["pub"], n)
    assert host_cols(stark, pub_lde) == H.public_columns_lde(h["pub"], n)
    got = stark.hash_io_boundary(h["trace_lde"], pub_lde, n, h["alphas"])
    assert stark.tensor_to_felts(got) == h["want"]


@pytest.mark.parametrize("n", SIZES)
def test_dense_boundary_acc_modes(stark, honest, n):
    """acc NULL is the test above; here acc distinct from out (and left as it was) and acc aliased to out."""
    h = honest[n]
    pub_lde = stark.hash_io_public_lde(h["pub"], n)
    acc = mixed(4 * n, n + 2)
    summed = [(a + b) % P for a, b in zip(acc, h["want"])]
    acc_t = stark.felts_to_tensor(acc)
    got = stark.hash_io_boundary(h["trace_lde"], pub_lde, n, h["alphas"], acc=acc_t)
    assert stark.tensor_to_felts(got) == summed and stark.tensor_to_felts(acc_t) == acc
    same = stark.hash_io_boundary(h["trace_lde"], pub_lde, n, h["alphas"], acc=acc_t, out=acc_t)
    assert same.data_ptr() == acc_t.data_ptr() and stark.tensor_to_felts(acc_t) == summed


@pytest.mark.parametrize("n,shift", [(n, s) for n in SIZES for s in (S.GEN, OTHER_SHIFT)])
def test_dense_boundary_on_arbitrary_columns(stark, n, shift):
    """The column is a pointwise function of whatever the arrays hold: extreme limb patterns in the trace columns, the
    public columns, acc and the challenges; the default and another shift."""
    cols, pub_lde = [mixed(4 * n, 10 * n + c) for c in range(2)], [mixed(4 * n, 10 * n + 2 + c) for c in range(3)]
    alphas, acc = mixed(3, 10 * n + 5), mixed(4 * n, 10 * n + 6)
    want = H.boundary_on_coset(cols, pub_lde, n, alphas, shift)
    got = stark.hash_io_boundary(dev_cols(stark, cols), dev_cols(stark, pub_lde), n, alphas, shift,
                                 acc=stark.felts_to_tensor(acc))
    assert stark.tensor_to_felts(got) == [(a + b) % P for a, b in zip(acc, want)]


def test_dense_boundary_with_a_shifted_honest_trace(stark, honest):
    """A non-default shift end to end: public columns extended with it, the trace LDE on the same coset."""
    n, h = 1024, honest[1024]
    inputs = h["inputs"]
    trace = stark.pedersen_trace(stark.felts_to_tensor([x for x, _ in inputs]), stark.felts_to_tensor([y for _, y in inputs]))
    trace_lde = stark.lde(trace, shift=OTHER_SHIFT)
    pub_lde = stark.hash_io_public_lde(h["pub"], n, OTHER_SHIFT)
    want = H.boundary_on_coset(host_cols(stark, trace_lde), H.public_columns_lde(h["pub"], n, OTHER_SHIFT), n, h["alphas"],
                               OTHER_SHIFT)
    assert stark.tensor_to_felts(stark.hash_io_boundary(trace_lde, pub_lde, n, h["alphas"], OTHER_SHIFT)) == want
    assert S.poly_degree_bound_check(want, OTHER_SHIFT, n - 1)


# ---- the points call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_points_equal_the_dense_column_at_every_position(stark, honest, n):
    import torch
    h = honest[n]
    M = 4 * n
    pos = torch.arange(M, dtype=torch.int64, device="cuda")
    cur = h["trace_lde"].permute(1, 0, 2).contiguous()
    out, status = stark.hash_io_boundary_points(n, stark.hash_io_coefficients(h["pub"], n), h["alphas"], S.GEN, pos, cur)
    assert status.cpu().tolist() == [stark.POINT_OK] * M
    assert stark.tensor_to_felts(out) == h["want"]


def test_public_coefficients_are_the_interpolants(stark, honest):
    for n in SIZES:
        assert host_cols(stark, stark.hash_io_coefficients(honest[n]["pub"], n)) == H.public_coefficients(honest[n]["pub"], n)


@pytest.mark.parametrize("k", (1, 2, 64, 128, 256, 512, 2048, 1 << 15))
def test_points_from_coefficient_arrays_alone(stark, k):
    """No trace: coefficient arrays below, at and above one block's stride of 256 against Horner in integers, eight
    points each (both ends of the coset among them), extreme limb patterns in the coefficients."""
    import torch
    n = 512 * k
    coeffs = [mixed(k, 3 * k + c) for c in range(3)]
    rng = random.Random(k)
    alphas = [rng.randrange(P) for _ in range(3)]
    pos = [0, 1, 4 * n - 1, 2 * n] + [rng.randrange(4 * n) for _ in range(4)]
    cur = [mixed(4, 7 * k + i) for i in range(8)]
    out, status = stark.hash_io_boundary_points(n, dev_cols(stark, coeffs), alphas, OTHER_SHIFT,
                                                torch.tensor(pos, dtype=torch.int64, device="cuda"),
                                                dev_cols(stark, cur))
    assert status.cpu().tolist() == [stark.POINT_OK] * 8
    assert stark.tensor_to_felts(out) == [H.boundary_at(n, coeffs, alphas, OTHER_SHIFT, p, c) for p, c in zip(pos, cur)]


def test_points_status_and_neighbours(stark):
    import torch
    n = 1024
    coeffs = [mixed(2, c) for c in range(3)]
    alphas = [2, 3, 4]
    pos = [5, 4 * n, 6, -1, 7, 8, 9]          # -1 is 2^64 - 1 to the library
    cur = [[1, 2, 3, 4] for _ in pos]
    cur[5] = [1, 2, 3, P]                      # a felt of the row that the value does not even use
    cur[6] = [(1 << 256) - 1, 2, 3, 4]
    out, status = stark.hash_io_boundary_points(n, dev_cols(stark, coeffs), alphas, S.GEN,
                                                torch.tensor(pos, dtype=torch.int64, device="cuda"), dev_cols(stark, cur))
    ok, bad = stark.POINT_OK, stark.POINT_OUT_OF_RANGE
    assert status.cpu().tolist() == [ok, bad, ok, bad, ok, bad, bad]
    got = stark.tensor_to_felts(out)
    for i in (0, 2, 4):
        assert got[i] == H.boundary_at(n, coeffs, alphas, S.GEN, pos[i], cur[i])
    assert [got[i] for i in (1, 3, 5, 6)] == [0] * 4


# ---- argument edges of both C calls -------------------------------------------------------------------------------------
def test_argument_edges(stark, honest):
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    h = honest[512]
    M = 2048
    pack = _lib.pack_felts
    trace, pub = h["trace_lde"], stark.hash_io_public_lde(h["pub"], 512)
    out = stark.felts_to_tensor([FILL] * M)
    on_domain = S.root_of_unity(11)  # w_4n at n = 512: shift^(4n) = 1

    def dense(log_n=9, shift=3, trace_p=trace.data_ptr(), stride=M, pub_p=pub.data_ptr(), alphas=pack([1, 2, 3]),
              out_p=out.data_ptr()):
        return lib.sp_hash_io_boundary_dev(trace_p, stride, pub_p, log_n, alphas, None if shift is None else pack([shift]),
                                           None, out_p, stark._stream())
    for kwargs, word in (({"log_n": 8}, "log_n"), ({"log_n": 25}, "log_n"), ({"shift": 0}, "shift"), ({"shift": 1}, "shift"),
                         ({"shift": on_domain}, "shift"), ({"shift": P}, "shift"), ({"shift": None}, "shift_host"),
                         ({"trace_p": None}, "trace_lde"), ({"pub_p": None}, "pub_lde"), ({"alphas": None}, "alphas_host"),
                         ({"out_p": None}, "out"), ({"stride": M - 1}, "col_stride")):
        assert dense(**kwargs) == -3, kwargs
        err = _lib.last_error()
        assert err.startswith("sp_hash_io_boundary_dev") and word in err, (kwargs, err)
    torch.cuda.synchronize()
    assert set(stark.tensor_to_felts(out)) == {FILL}

    coef = stark.hash_io_coefficients(h["pub"], 512)
    pos = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    cur = dev_cols(stark, [[1, 2, 3, 4], [5, 6, 7, 8]])
    pout = stark.felts_to_tensor([FILL] * 2)
    status = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")

    def points(log_n=9, shift=3, n_points=2, coef_p=coef.data_ptr(), alphas=pack([1, 2, 3]), pos_p=pos.data_ptr(),
               cur_p=cur.data_ptr(), out_p=pout.data_ptr(), status_p=status.data_ptr()):
        return lib.sp_hash_io_boundary_points_dev(log_n, coef_p, alphas, None if shift is None else pack([shift]), n_points,
                                                  pos_p, cur_p, out_p, status_p, stark._stream())
    for kwargs, word in (({"log_n": 8}, "log_n"), ({"log_n": 31}, "log_n"), ({"shift": 0}, "shift"), ({"shift": P - 1}, "shift"),
                         ({"shift": on_domain}, "shift"), ({"shift": None}, "shift_host"), ({"coef_p": None}, "coef"),
                         ({"alphas": None}, "alphas_host"), ({"pos_p": None}, "pos"), ({"cur_p": None}, "cur"),
                         ({"out_p": None}, "out"), ({"status_p": None}, "status"), ({"n_points": (1 << 30) + 1}, "n_points")):
        assert points(**kwargs) == -3, kwargs
        err = _lib.last_error()
        assert err.startswith("sp_hash_io_boundary_points_dev") and word in err, (kwargs, err)
    # nothing to do is SP_OK, whatever the pointers
    assert points(n_points=0, coef_p=None, pos_p=None, cur_p=None, out_p=None, status_p=None) == 0
    torch.cuda.synchronize()
    assert set(stark.tensor_to_felts(pout)) == {FILL} and status.cpu().tolist() == [0xEE, 0xEE]


# ---- prove_hashes / verify_hashes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proofs(stark):
    """k -> (inputs, proof) with three queries, proved once."""
    out = {}
    for k in (1, 2, 4):
        inputs = hash_inputs(k, 40 + k)
        proof = stark.prove_hashes(stark.felts_to_tensor([x for x, _ in inputs]), stark.felts_to_tensor([y for _, y in inputs]),
                                   n_queries=3, seed=7 + k)
        out[k] = (inputs, proof)
    return out


@pytest.mark.parametrize("k", (1, 2, 4))
def test_round_trip(stark, proofs, k):
    inputs, proof = proofs[k]
    assert proof["air"] == "pedersen_io" and proof["n"] == 512 * k and len(proof["queries"]) == 3
    assert proof["public_inputs"] == H.public_inputs(inputs)  # h_i = R.pedersen_hash(x_i, y_i)
    for i, (x, y) in enumerate(inputs):
        assert proof["public_inputs"][3 * i + 2] == R.pedersen_hash(x, y)
    assert stark.verify_hashes(proof) == (True, "ok")
    assert stark.verify_hashes(proof, n_queries=3) == (True, "ok")
    assert stark.verify_hashes(proof, n_queries=4) == (False, "shape")
    assert H.verify_proof_io(proof, hash2=c_hash) == (True, "ok")
    # the unbound verifier does not know this AIR, and this verifier takes no other
    assert stark.verify(proof) == (False, "malformed")


def test_verify_hashes_refuses_an_unbound_proof(stark):
    inputs = hash_inputs(1, 5)
    proof = stark.prove(stark.felts_to_tensor([inputs[0][0]]), stark.felts_to_tensor([inputs[0][1]]), n_queries=2)
    assert stark.verify(proof) == (True, "ok")
    assert stark.verify_hashes(proof) == (False, "malformed")
    assert stark.verify_hashes(dict(proof, air="pedersen_io")) == (False, "public inputs")


@pytest.mark.parametrize("k,which", ((1, 0), (2, 1), (4, 2)))
def test_binding_a_lying_prover_is_caught(stark, k, which):
    """The prover claims an output that is off by one and is consistent about it: transcript, composition and FRI all
    use the claim.  The quotient (px - H) / (x^k - g^-k) is then no polynomial, and the 16 top coefficients of the
    final layer vanish with probability p^-16: both verifiers say "final layer degree"."""
    inputs = hash_inputs(k, 60 + k)
    outs = [R.pedersen_hash(x, y) for x, y in inputs]
    outs[which % k] = (outs[which % k] + 1) % P
    proof = stark.prove_hashes(stark.felts_to_tensor([x for x, _ in inputs]), stark.felts_to_tensor([y for _, y in inputs]),
                               n_queries=3, seed=1, outs=outs)
    assert proof["public_inputs"] == H.public_inputs(inputs, outs)
    assert stark.verify_hashes(proof) == (False, "final layer degree")
    assert H.verify_proof_io(proof, hash2=c_hash) == (False, "final layer degree")


def tamperings(proof):
    """(name, tampered proof, the reason when it is certain) - those of test_prove_then_verify_small, and the
    statement edited after the fact."""
    def edit(fn):
        bad = copy.deepcopy(proof)
        fn(bad)
        return bad

    def flip_trace(b): b["queries"][0]["trace"][0]["values"][1] ^= 1
    def flip_layer(b): b["queries"][1]["layers"][2][0]["value"] ^= 1
    def flip_final(b): b["final_layer"][5] ^= 1
    def flip_root(b): b["layer_roots"][0] ^= 1
    def bump_seed(b): b["seed"] += 1
    def one_input(b): b["public_inputs"] = [1]
    def other_output(b): b["public_inputs"][2] = (b["public_inputs"][2] + 1) % P
    def other_input(b): b["public_inputs"][0] = (b["public_inputs"][0] + 1) % P
    def swap_triples(b): b["public_inputs"] = b["public_inputs"][3:6] + b["public_inputs"][0:3] + b["public_inputs"][6:]
    def short_list(b): b["public_inputs"] = b["public_inputs"][:-3]
    def long_list(b): b["public_inputs"] = b["public_inputs"] + b["public_inputs"][:3]
    return [("trace value", edit(flip_trace), "trace path"), ("layer value", edit(flip_layer), None),
            ("final layer", edit(flip_final), "final layer degree"), ("layer root", edit(flip_root), None),
            ("seed", edit(bump_seed), None), ("one public input", edit(one_input), "public inputs"),
            ("another output", edit(other_output), None), ("another input", edit(other_input), None),
            ("swapped triples", edit(swap_triples), None), ("short list", edit(short_list), "public inputs"),
            ("long list", edit(long_list), "public inputs")]


def test_tampering_is_rejected_with_the_reference_reason(stark, proofs):
    _, proof = proofs[2]
    for name, bad, reason in tamperings(proof):
        got = stark.verify_hashes(bad)
        want = H.verify_proof_io(bad, hash2=c_hash)
        assert not got[0] and got == want, (name, got, want)
        if reason:
            assert got[1] == reason, (name, got)


def test_malformed_inputs_never_raise(stark, proofs):
    _, proof = proofs[1]

    class Hostile(dict):
        def get(self, *a):
            raise RuntimeError("inspected")
    cases = [None, 7, [], {}, Hostile(proof), {"air": "pedersen_io"}, dict(proof, air=None), dict(proof, n=513),
             dict(proof, n="512"), dict(proof, shift=0), dict(proof, shift=1), dict(proof, shift=P), dict(proof, seed=-1),
             dict(proof, trace_root=P), dict(proof, public_inputs=None), dict(proof, public_inputs=[1.5, 2, 3]),
             dict(proof, public_inputs=[1 << 256, 2, 3]), dict(proof, final_layer=[P] * 64), dict(proof, queries=None),
             dict(proof, queries=[{}]), {k: v for k, v in proof.items() if k != "layer_roots"}]
    bad = copy.deepcopy(proof)
    bad["queries"][0]["trace"][2]["values"] = bad["queries"][0]["trace"][2]["values"][:3]
    cases.append(bad)
    bad = copy.deepcopy(proof)
    bad["queries"][2]["layers"][1][1]["path"].append(5)
    cases.append(bad)
    bad = copy.deepcopy(proof)
    bad["queries"][1]["layers"].pop()
    cases.append(bad)
    for i, case in enumerate(cases):
        assert stark.verify_hashes(case) == (False, "malformed"), i
    assert stark.verify_hashes(proof, final_log="6") == (False, "malformed")
    # well-formed, but not a statement of this AIR: an entry that is an integer below 2^256 and no felt
    assert stark.verify_hashes(dict(proof, public_inputs=[P, 2, 3])) == (False, "public inputs")
    assert stark.verify_hashes(dict(proof, layer_roots=proof["layer_roots"][:-1])) == (False, "shape")
    assert stark.verify_hashes(proof, final_log=5) == (False, "shape")


def test_full_size_smoke(stark):
    """k = 2048 hashes, the 2^20-row trace of the benchmark: accepted on the GPU and, with the C oracle's hash, by
    the integer verifier - as test_prove_then_verify_full_size does for the unbound proof."""
    import torch
    k = 2048
    g = torch.Generator().manual_seed(23)
    xs = torch.randint(0, 2**62, (k, 4), dtype=torch.int64, generator=g)
    ys = torch.randint(0, 2**62, (k, 4), dtype=torch.int64, generator=g)
    xs[:, 3] &= (1 << 58) - 1
    ys[:, 3] &= (1 << 58) - 1
    proof = stark.prove_hashes(xs.cuda(), ys.cuda(), n_queries=4, seed=3)
    assert len(proof["public_inputs"]) == 3 * k and len(proof["layer_roots"]) == 16 and len(proof["final_layer"]) == 64
    x0, y0 = stark.tensor_to_felts(xs[:1])[0], stark.tensor_to_felts(ys[:1])[0]
    assert proof["public_inputs"][:3] == [x0, y0, c_hash(x0, y0)]
    assert stark.verify_hashes(proof, n_queries=4) == (True, "ok")
    assert H.verify_proof_io(proof, hash2=c_hash) == (True, "ok")
