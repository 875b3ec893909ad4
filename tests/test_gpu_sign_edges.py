"""The signer on the inputs random batches cannot reach (tests/sign_cases.py, proven against the oracle by
tests/test_sign_cases_cpu.py): nonces the attempt rejects, the host loops that draw the next nonce, the compacted nonce
pipeline against the reference's own signatures at every chunk / grid / threshold edge, and the fixed-base walks (gathered
at 21- and 16-bit windows, masked) on patterned scalars.  Every comparison is integer equality.

NOT covered, because it cannot be: the first rejection of sign_attempt, r = x(k G) outside [1, 2^251).  An input for it is
a k whose k G has a chosen x coordinate - a discrete logarithm.  The two other rejections (t = z + r d = 0 and
w = k / t outside [1, 2^251)) are solved for z or d.  The device's own next-seed loops (ecdsa_sign_rfc6979_kernel and
its redo twin) cannot be entered from outside either: their nonce depends on z, so z cannot be solved for after it."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import sign_cases as C
from oracle import ref_py as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TWO251 = C.N, C.TWO251
GUARD = 64
IN_PROCESS_SIZES = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)  # 4096 = C.COMPACT_MIN: the one-kernel signer below
GRID_STRIDE_N = 16421
CHILDREN = {
    # name: (environment, sizes)
    "chunk": ({"STARKPERP_SIGN_CHUNK": "4096"}, (4096, 4097, 8192, 12325)),
    "compact_min": ({"STARKPERP_SIGN_COMPACT_MIN": "1"}, (1, 64, 129)),
    "masked": ({"STARKPERP_SIGN_MASKED": "1"}, ()),
}


# ---- helpers (the children import this module and use the same ones) -----------------------------------------------
def felts(values):
    from starkperp import stark as st
    return st.felts_to_tensor(values)


def ints(t):
    from starkperp import stark as st
    return st.tensor_to_felts(t)


def seed_tensor(seeds):
    import numpy as np
    import torch
    return torch.from_numpy(np.asarray(seeds, dtype=np.uint64).view(np.int64)).cuda()


def guarded_outputs(n, columns=2):
    """Output tensors with GUARD rows behind n, every row the sentinel, every status byte 0xEE."""
    import torch
    row = felts([C.SENTINEL])
    outs = [row.repeat(n + GUARD, 1).contiguous() for _ in range(columns)]
    status = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    return outs, status


def raw_call(fn, inputs, n, columns=2):
    """One device-pointer entry point of the library on sentinel-filled outputs: (status list, [column ints])."""
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    outs, status = guarded_outputs(n, columns)
    args = [None if t is None else t.data_ptr() for t in inputs] + [t.data_ptr() for t in outs]
    _lib.check(getattr(lib, fn)(*args, status.data_ptr(), n, torch.cuda.current_stream().cuda_stream), fn)
    torch.cuda.synchronize()
    return status.cpu().tolist(), [ints(t) for t in outs]


def check_guarded(n, want_status, want_rows, status, columns):
    """Rows of OK items hold the expected values; rows of the others and the guard rows keep the sentinel; every status
    byte below n is rewritten and none behind it."""
    assert status[:n] == want_status
    assert status[n:] == [0xEE] * GUARD
    for c, col in enumerate(columns):
        want = [row[c] if st == C.OK else C.SENTINEL for st, row in zip(want_status, want_rows)] + [C.SENTINEL] * GUARD
        bad = [i for i in range(n + GUARD) if col[i] != want[i]]
        assert not bad, "column %d, first wrong rows %s of %d" % (c, bad[:5], n)


def digest(status, *columns):
    """sha256 over a status list and columns of ints: what a child prints and the parent recomputes from the pool."""
    h = hashlib.sha256(bytes(status))
    for col in columns:
        h.update(b"".join(int(v).to_bytes(32, "little") for v in col))
    return h.hexdigest()


class Pool:
    """The nonce pool on the GPU: rows of pool + INVALID_ITEMS, gathered by a pattern's index list."""

    def __init__(self):
        self.pool = C.nonce_pool()
        rows = [(z, d, seed or 0, C.OK, sig) for z, d, seed, _, sig in self.pool]
        rows += [(z, d, seed or 0, C.BAD_INPUT, (0, 0)) for z, d, seed in C.INVALID_ITEMS]
        self.z, self.d = felts([r[0] for r in rows]), felts([r[1] for r in rows])
        self.seed = seed_tensor([r[2] for r in rows])
        self.rows = rows

    def gather(self, idx):
        import torch
        i = torch.as_tensor(idx, dtype=torch.int64, device="cuda")
        return self.z[i].contiguous(), self.d[i].contiguous(), self.seed[i].contiguous()

    def expected(self, idx):
        return ([self.rows[i][3] for i in idx], [self.rows[i][4][0] for i in idx], [self.rows[i][4][1] for i in idx])

    def sign_raw(self, idx):
        """sp_ecdsa_sign_rfc6979_batch_dev on sentinel-filled outputs, checked for what it must leave alone; returns
        (status, r, s) of the n items with the untouched rows of rejected items read as zero."""
        n = len(idx)
        z, d, seeds = self.gather(idx)
        status, (r, s) = raw_call("sp_ecdsa_sign_rfc6979_batch_dev", [z, d, seeds], n)
        assert status[n:] == [0xEE] * GUARD and r[n:] == s[n:] == [C.SENTINEL] * GUARD, "wrote behind the batch"
        for i in range(n):
            if status[i] != C.OK:
                assert r[i] == s[i] == C.SENTINEL, "row %d of a rejected item was written" % i
                r[i] = s[i] = 0
        return status[:n], r[:n], s[:n]


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.fixture(scope="module")
def cases():
    """attempt_cases() with an invalid item last and a length that is no multiple of the block: the kernels clone the last
    item into the idle lanes of the last block."""
    cs = C.attempt_cases()
    last = [c for c in cs if c[3].startswith("precedence z+N")][:2]
    cs = cs + last[:1]
    if len(cs) % 128 == 0:
        cs = cs + last[1:]
    assert len(cs) % 128 and C.attempt(*cs[-1][:3])[0] == C.BAD_INPUT
    C.prime_r([c[1] for c in cs])
    want = [C.attempt(z, d, k) for z, d, k, _ in cs]
    return cs, want


# ---- (a) single attempts on every entry point -----------------------------------------------------------------------
def test_attempts_staged(cases):
    """sp_ecdsa_sign_batch: status and (r, s) of every crafted case; rows of items that are not OK are zero."""
    from starkperp import batch
    cs, want = cases
    rs, ss, st = batch.sign_attempt_many([c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs])
    for i, (c, w) in enumerate(zip(cs, want)):
        assert (st[i], rs[i], ss[i]) == w, (i, c[3])
    assert st.count(C.RETRY) >= 40 and st.count(C.BAD_INPUT) >= 20


def test_attempts_on_device_pointers(cases):
    """sp_ecdsa_sign_batch_dev called directly: rows of rejected items and 64 guard rows keep their sentinel, every
    status byte below n is rewritten, none behind it; then through batch.sign_dev(k=...), whose rejected rows are zero."""
    import torch
    from starkperp import batch
    cs, want = cases
    n = len(cs)
    z, d, k = felts([c[0] for c in cs]), felts([c[1] for c in cs]), felts([c[2] for c in cs])
    status, columns = raw_call("sp_ecdsa_sign_batch_dev", [z, d, k], n)
    check_guarded(n, [w[0] for w in want], [w[1:] for w in want], status, columns)
    r, s, st = batch.sign_dev(z, d, k=k)
    torch.cuda.synchronize()
    assert list(zip(st.cpu().tolist(), ints(r), ints(s))) == want
    # a batch of one rejected item, and one that ends inside the first wave
    for m in (1, 37):
        sub = [i for i, w in enumerate(want) if w[0] == C.RETRY][:m]
        status, columns = raw_call("sp_ecdsa_sign_batch_dev", [t[sub].contiguous() for t in (z, d, k)], m)
        check_guarded(m, [C.RETRY] * m, [(0, 0)] * m, status, columns)


def test_accepted_attempts_verify(cases):
    """Every accepted attempt verifies under d G on the ladder and through the key tables (z = 0 is signable but never
    verifies, signature.py:251-257)."""
    from oracle import cref
    from starkperp import batch
    cs, want = cases
    ok = [i for i, w in enumerate(want) if w[0] == C.OK]
    zs, rs, ss = [cs[i][0] for i in ok], [want[i][1] for i in ok], [want[i][2] for i in ok]
    pubs = cref.public_keys_many([cs[i][1] for i in ok])
    expect = [1 if z else 0 for z in zs]
    assert expect.count(1) >= 1000
    assert batch.verify_codes(zs, rs, ss, pubs, key_tables=False) == expect
    assert batch.verify_codes(zs, rs, ss, pubs, key_tables=True) == expect


# ---- (b) public keys on the scalar patterns -----------------------------------------------------------------------
def check_public_keys():
    """{entry point: digest} of d G for the scalar patterns; asserts nothing itself."""
    import torch
    from starkperp import batch
    ds = [k for k, _ in C.scalar_patterns()]
    out = {"staged": digest([], *zip(*batch.public_keys_many(ds)))}
    dd = ds + [0, N]  # two invalid keys last; the length is no multiple of the block
    if len(dd) % 128 == 0:
        dd.append(0)
    status, (qx, qy) = raw_call("sp_public_key_batch_dev", [felts(dd)], len(dd))
    out["dev"] = digest(status, qx, qy)
    qx2, qy2, st2 = batch.public_keys_dev(felts(dd), want_y=False)
    torch.cuda.synchronize()
    out["dev_x_only"] = digest(st2.cpu().tolist(), ints(qx2)) if qy2 is None else "y was returned"
    return out


def expected_public_keys():
    from oracle import cref
    ds = [k for k, _ in C.scalar_patterns()]
    pts = cref.public_keys_many(ds)
    for i in range(0, len(ds), 97):
        assert pts[i] == R.private_key_to_ec_point_on_stark_curve(ds[i])
    bad = 2 + (1 if (len(ds) + 2) % 128 == 0 else 0)
    st = [C.OK] * len(ds) + [C.BAD_INPUT] * bad
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    guard = [C.SENTINEL] * (bad + GUARD)
    return {"staged": digest([], xs, ys),
            "dev": digest(st + [0xEE] * GUARD, xs + guard, ys + guard),
            "dev_x_only": digest(st, xs + [0] * bad)}


def test_public_keys_of_the_scalar_patterns():
    """sp_public_key_batch and sp_public_key_batch_dev (with and without y) against the C oracle / R on every scalar
    pattern; invalid keys answer BAD_INPUT, their rows and the guard rows keep the sentinel."""
    assert check_public_keys() == expected_public_keys()


# ---- (c) the host loops that draw the next nonce ----------------------------------------------------------------------
def successor(seed, m):
    for _ in range(m):
        seed = 1 if seed is None else seed + 1
    return seed


class StubbornNonces:
    """generate_k_rfc6979 that answers an item's rejected nonce k0 for its first m calls, then the real one."""

    def __init__(self, items):
        from starkperp import signature
        self.real = signature.generate_k_rfc6979
        self.plan = {(z, d): [k0, m] for z, d, k0, m, _ in items}
        self.trail = {(z, d): [] for z, d, _, _, _ in items}

    def __call__(self, z, d, seed=None):
        self.trail[(z, d)].append(seed)
        plan = self.plan[(z, d)]
        if plan[1] > 0:
            plan[1] -= 1
            return plan[0]
        return self.real(z, d, seed)


def retry_items(seeds):
    """(z, d, k0, m, seed) for m = 0, 1, 2 and every seed: distinct t = 0 cases, so (z, d) names the item."""
    t0 = [c for c in C.attempt_cases() if c[3] == "t=0"]
    assert len({c[:2] for c in t0}) == len(t0) >= 3 * len(seeds)
    items = [(z, d, k0, m, seed) for (z, d, k0, _), (m, seed) in zip(t0, [(m, s) for s in seeds for m in (0, 1, 2)])]
    assert all(C.attempt(z, d, k0)[0] == C.RETRY for z, d, k0, _, _ in items)
    return items


def check_retry_run(items, got, stub):
    for i, (z, d, k0, m, seed) in enumerate(items):
        k = R.generate_k_rfc6979(z, d, successor(seed, m))
        status, r, s = C.attempt(z, d, k)
        assert status == C.OK and got[i] == (r, s), (i, m, seed)
        assert stub.trail[(z, d)] == [successor(seed, j) for j in range(m + 1)], (i, m, seed)


def test_host_nonce_loop_draws_the_next_seed(monkeypatch):
    """_sign_many_host_nonces with nonces rejected 0, 1 and 2 times in one mixed batch: the `again` list, the seed trail
    None -> 1 -> 2 and s -> s + 1 (signature.py:146-148), results at the right indices."""
    import starkperp.signature
    from starkperp import batch
    items = retry_items([None, 0, 7, 255])
    stub = StubbornNonces(items)
    monkeypatch.setattr(starkperp.signature, "generate_k_rfc6979", stub)
    got = batch._sign_many_host_nonces([i[0] for i in items], [i[1] for i in items], [i[4] for i in items])
    check_retry_run(items, got, stub)
    assert stub.trail[items[2][:2]] == [None, 1, 2] and stub.trail[items[5][:2]] == [0, 1, 2]
    assert stub.trail[items[11][:2]] == [255, 256, 257]


def test_sign_many_hands_wide_seeds_to_the_host_loop(monkeypatch):
    """sign_many with seeds >= 2^64 (the host path) between items the device signs: rejected host nonces are redrawn, the
    device's items are untouched by the stub, every result lands at its index."""
    import starkperp.signature
    from starkperp import batch
    items = retry_items([2**64, 2**64 + 255, 2**200 + 3])
    stub = StubbornNonces(items)
    monkeypatch.setattr(starkperp.signature, "generate_k_rfc6979", stub)
    pool = C.nonce_pool()[:9]
    zs, ds, seeds, want = [], [], [], []
    for j, (z, d, k0, m, seed) in enumerate(items):  # host item, device item, host item, ...
        zs += [z, pool[j][0]]
        ds += [d, pool[j][1]]
        seeds += [seed, pool[j][2]]
        want += [None, tuple(pool[j][4])]
    got = batch.sign_many(zs, ds, seeds)
    assert [tuple(g) for g in got[1::2]] == want[1::2]
    check_retry_run(items, got[0::2], stub)


# ---- (d) the compacted pipeline against the reference's signatures ------------------------------------------------
def run_patterns(pool, sizes, names=None):
    """{"n/pattern": digest of (status, r, s)} through sp_ecdsa_sign_rfc6979_batch_dev for every pattern of every size."""
    out = {}
    for n in sizes:
        for name, idx in C.batch_patterns(n, pool.pool).items():
            if names is None or name in names:
                out["%d/%s" % (n, name)] = digest(*pool.sign_raw(idx))
    return out


def expected_patterns(pool, sizes, names=None):
    out = {}
    for n in sizes:
        for name, idx in C.batch_patterns(n, pool.pool).items():
            if names is None or name in names:
                out["%d/%s" % (n, name)] = digest(*pool.expected(idx))
    return out


@pytest.mark.parametrize("n", IN_PROCESS_SIZES)
def test_signer_against_the_reference_at_every_pattern(pool, n):
    """sp_ecdsa_sign_rfc6979_batch_dev (sentinel-filled outputs, then batch.sign_dev) and batch_np.sign_many on every
    batch pattern over the nonce pool; expected status and signatures are the pool's R.sign values."""
    import numpy as np
    import torch
    from starkperp import batch, batch_np as bn
    for name, idx in C.batch_patterns(n, pool.pool).items():
        want = pool.expected(idx)
        got = pool.sign_raw(idx)
        bad = [i for i in range(n) if (got[0][i], got[1][i], got[2][i]) != (want[0][i], want[1][i], want[2][i])]
        assert not bad, "%s: first wrong items %s (pool rows %s)" % (name, bad[:5], [idx[i] for i in bad[:5]])
        z, d, seeds = pool.gather(idx)
        r, s, st = batch.sign_dev(z, d, seeds)
        torch.cuda.synchronize()
        assert (st.cpu().tolist(), ints(r), ints(s)) == want, name
        zn, dn = bn.felts_from_ints([pool.rows[i][0] for i in idx]), bn.felts_from_ints([pool.rows[i][1] for i in idx])
        sn = np.asarray([pool.rows[i][2] for i in idx], dtype=np.uint64)
        if C.BAD_INPUT in want[0]:
            with pytest.raises(AssertionError):
                bn.sign_many(zn, dn, sn)
        else:
            rn, ss = bn.sign_many(zn, dn, sn)
            assert (bn.ints_from_felts(rn), bn.ints_from_felts(ss)) == want[1:], name


def test_retry_lists_longer_than_their_grids(pool):
    """16 421 copies of the item with 11 rejected candidates: from round 1 on n / 2^(j+1) + n / 2^(j+3) + 8192 < n, so
    every retry launch has more list entries than threads (the grid-stride loop), and every item reaches the straggler
    launch, whose grid is (n >> 11) + 8192 threads."""
    import numpy as np
    from starkperp import batch_np as bn
    n = GRID_STRIDE_N
    for j in range(1, C.ROUNDS):
        assert (n >> (j + 1)) + (n >> (j + 3)) + 8192 < n
    assert (n >> (C.ROUNDS + 1)) + 8192 < n
    idx = C.batch_patterns(n, pool.pool)["uniform_11"]
    assert pool.pool[idx[0]][3] == 11 == C.ROUNDS + 1
    want = pool.expected(idx)
    assert pool.sign_raw(idx) == want
    row = pool.rows[idx[0]]
    rn, sn = bn.sign_many(bn.felts_from_ints([row[0]] * n), bn.felts_from_ints([row[1]] * n),
                          np.full(n, row[2], dtype=np.uint64))
    assert (bn.ints_from_felts(rn), bn.ints_from_felts(sn)) == want[1:]


def masked_run():
    """The attempts of (a) and the keys of (b), as digests."""
    import torch
    from starkperp import batch
    cs = C.attempt_cases()
    z, d, k = [c[0] for c in cs], [c[1] for c in cs], [c[2] for c in cs]
    rs, ss, st = batch.sign_attempt_many(z, d, k)
    out = {"attempts_staged": digest(st, rs, ss)}
    r, s, st = batch.sign_dev(felts(z), felts(d), k=felts(k))
    torch.cuda.synchronize()
    out["attempts_dev"] = digest(st.cpu().tolist(), ints(r), ints(s))
    out.update(check_public_keys())
    return out


def masked_expected():
    cs = C.attempt_cases()
    C.prime_r([c[2] for c in cs])
    want = [C.attempt(z, d, k) for z, d, k, _ in cs]
    one = digest([w[0] for w in want], [w[1] for w in want], [w[2] for w in want])
    return dict(expected_public_keys(), attempts_staged=one, attempts_dev=one)


def child_main(name):
    """What a child process runs: 16-bit windows (a quick start, and the other width of the gathered walk), then the
    runs of its kind; one JSON line."""
    from starkperp import _lib
    lib = _lib.ensure_init(0, 16)
    out = {"table_bytes": int(lib.sp_table_bytes())}
    if name == "masked":
        out["digests"] = masked_run()
    else:
        out["digests"] = run_patterns(Pool(), CHILDREN[name][1])
    print("CHILD " + json.dumps(out))


def test_chunks_tiny_pipelines_and_the_masked_walk_in_fresh_processes(pool):
    """STARKPERP_SIGN_CHUNK / _COMPACT_MIN / _MASKED are read once per process, so each runs in a fresh child, one after
    another: (1) chunks of 4096 items - second and later iterations of the chunk loop, a last chunk of 37 items, the seeds
    and status of every chunk at its own offset; (2) the pipeline on batches smaller than a wave; (3) the attempts and
    the public keys through the masked walk.  The parent compares each child's digests with the pool / the oracle."""
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_sign_edges as T; T.child_main(sys.argv[1])" % (
        ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "stark-perpetual_amd"))
    tables = {}
    for name, (env, sizes) in CHILDREN.items():
        out = subprocess.run([sys.executable, "-c", code, name], capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, **env), cwd=ROOT)
        assert out.returncode == 0, "child %s: %s" % (name, out.stderr[-2000:])
        res = json.loads([line for line in out.stdout.splitlines() if line.startswith("CHILD ")][0][6:])
        want = masked_expected() if name == "masked" else expected_patterns(pool, sizes)
        wrong = sorted(key for key in want if res["digests"].get(key) != want[key])
        assert not wrong and set(res["digests"]) == set(want), "child %s: %s" % (name, wrong)
        tables[name] = res["table_bytes"]
    assert tables["chunk"] == tables["compact_min"]
    assert tables["masked"] == tables["chunk"] + 63 * 16 * 64  # the masked table was built, so the masked walk ran
