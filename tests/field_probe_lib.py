"""Shared by tests/test_field_probe_cpu.py and tests/test_gpu_field_probe.py: the Python-integer model of every
operation the device probe (tests/gpu/field_probe.hip) runs, the input generators, and the checks.

A check takes the probe's raw output limbs and compares them with Python integers; there is no tolerance anywhere.
The CPU test runs every lane-private check on the output of the HOST twin (tests/host/field_probe_twin.cpp: the same
op table compiled with g++ and the bound checks on), which verifies the model and the generators without a GPU; the
GPU test runs the same checks on what the device build of the same headers returns.

Limb conventions are those of csrc/fp29.hpp: nine signed 29-bit limbs, limbs 0..7 in [0, 2^29) and a signed limb 8
("N-form"); values that take part in multiplications carry the Montgomery factor R = 2^261."""
import ctypes
import glob
import itertools
import os
import random
import shutil
import subprocess

import numpy as np

from oracle import ref_py as R
import workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "stark-perpetual_amd", "csrc")
PROBE_SRC = os.path.join(HERE, "gpu", "field_probe.hip")
OPS_HDR = os.path.join(HERE, "gpu", "field_probe_ops.hpp")
PROBE_BIN = os.path.join(HERE, "gpu", "field_probe")
TWIN_SRC = os.path.join(HERE, "host", "field_probe_twin.cpp")
TWIN_SO = os.path.join(HERE, "host", "field_probe_twin.so")

P, N = R.FIELD_PRIME, R.EC_ORDER
NL, LB = 9, 29
MASK = (1 << LB) - 1
RM = 1 << (NL * LB)  # the Montgomery radix 2^261
L8 = 1 << 21
_W = np.array([1 << (LB * i) for i in range(NL)], dtype=object)


# ---------------------------------------------------------------- limbs
def nform(v):
    """The N-form limbs of the integer v (any sign): limbs 0..7 in [0, 2^29), limb 8 the signed rest."""
    return [(v >> (LB * i)) & MASK for i in range(8)] + [v >> (LB * 8)]


def values(arr):
    """Integer value of every element of an int32 array (..., 9), as an object array (...)."""
    return np.asarray(arr).astype(object).dot(_W)


def elems(items):
    """items: a list of items, each a list of limb lists -> int32 array (n, k, 9)."""
    return np.array(items, dtype=np.int64).astype(np.int32).reshape(len(items), -1, NL)


def is_nform(arr):
    low = np.asarray(arr)[..., :8]
    return bool(((low >= 0) & (low <= MASK)).all())


def mont(x, k=0, m=P):
    """N-form limbs of the Montgomery representative x R mod m, shifted by k m."""
    return nform(x * RM % m + k * m)


# ---------------------------------------------------------------- building and running
def hipcc():
    """The compiler of csrc/Makefile: $HIPCC, else hipcc on the PATH, else the default ROCm install.  build() in
    __graft_entry__.py builds the probe through probe_build_cmd() too, so there is one rule."""
    c = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return c if shutil.which(c) or os.path.exists(c) else None


def probe_sources():
    return [PROBE_SRC, OPS_HDR] + sorted(glob.glob(os.path.join(CSRC, "*.hpp")))


def probe_build_cmd(out):
    # the flags of csrc/Makefile
    return [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, PROBE_SRC, "-o", out]


def probe_is_fresh():
    return os.path.exists(PROBE_BIN) and os.path.getmtime(PROBE_BIN) >= max(os.path.getmtime(s) for s in probe_sources())


def ensure_probe():
    """The probe binary, rebuilt when missing or older than its sources.  Raises when that cannot be done."""
    if not probe_is_fresh():
        if hipcc() is None:
            raise RuntimeError("tests/gpu/field_probe is missing or out of date and there is no hipcc to build it")
        subprocess.run(probe_build_cmd(PROBE_BIN), check=True, timeout=900)
    return PROBE_BIN


def probe_shapes(binary=PROBE_BIN):
    """{op: (kin, kout, nflag, quad)} as the binary itself lists them (no GPU needed)."""
    out = subprocess.run([binary, "--list"], check=True, capture_output=True, text=True, timeout=60).stdout
    return {l.split()[0]: tuple(int(x) for x in l.split()[1:]) for l in out.splitlines()}


def split_records(raw, n, kout, nflag):
    rec = np.frombuffer(raw, dtype=np.int32).reshape(n, kout * NL + nflag)
    return rec[:, :kout * NL].reshape(n, kout, NL), rec[:, kout * NL:]


class ProbeDied(Exception):
    pass


class Probe:
    """Runs the device probe, one op per process, never two at a time.  After the first invocation that does not end
    with exit status 0 (a HIP error, a fault, an abort, a timeout) nothing further is started: every later run()
    raises, so the remaining tests of the module fail without touching the GPU again.  The same holds when there is
    neither an up-to-date binary nor a compiler."""

    def __init__(self, workdir, timeout=120):
        self.workdir, self.timeout, self.dead, self.calls, self.binary = str(workdir), timeout, None, 0, None

    def run(self, op, arr, n=None):
        """(limbs (n, KOUT, 9), flags (n, NFLAG)) of op on the first n records of arr."""
        if self.dead:
            raise ProbeDied("the GPU is not used again after: " + self.dead)
        if self.binary is None:  # inside the first test that needs it: no compiler and no binary FAILS that test
            try:
                self.binary = ensure_probe()
                self.shapes = probe_shapes(self.binary)
            except Exception as e:
                self.dead = "no probe binary: %s" % e
                raise ProbeDied(self.dead)
        kin, kout, nflag, _ = self.shapes[op]
        arr = np.ascontiguousarray(arr, dtype=np.int32).reshape(-1, kin, NL)
        n = len(arr) if n is None else n
        fin, fout = os.path.join(self.workdir, op + ".in"), os.path.join(self.workdir, op + ".out")
        arr.tofile(fin)
        if os.path.exists(fout):
            os.remove(fout)
        self.calls += 1
        try:
            r = subprocess.run([self.binary, op, fin, fout, str(n)], capture_output=True, text=True, timeout=self.timeout)
        except subprocess.TimeoutExpired:
            self.dead = "%s (n = %d) did not finish in %d s" % (op, n, self.timeout)
            raise ProbeDied(self.dead)
        if r.returncode != 0:
            self.dead = "%s (n = %d) ended with status %d: %s" % (op, n, r.returncode, r.stderr.strip()[-500:])
            raise ProbeDied(self.dead)
        with open(fout, "rb") as f:
            return split_records(f.read(), n, kout, nflag)


class Twin:
    """The host twin: the op table of the probe under g++ with SP_CHECK_BOUNDS (an overflow aborts the process)."""

    def __init__(self):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I" + CSRC, "-o", TWIN_SO, TWIN_SRC])
        self.lib = ctypes.CDLL(TWIN_SO)
        self.lib.probe_run.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
        self.lib.probe_shape.argtypes = [ctypes.c_char_p, ctypes.c_void_p]

    def shape(self, op):
        s = (ctypes.c_int * 3)()
        assert self.lib.probe_shape(op.encode(), s) == 0, op
        return tuple(s)

    def run(self, op, arr, n=None):
        kin, kout, nflag = self.shape(op)
        arr = np.ascontiguousarray(arr, dtype=np.int32).reshape(-1, kin, NL)
        n = len(arr) if n is None else n
        out = np.zeros((n, kout * NL + nflag), dtype=np.int32)
        assert self.lib.probe_run(op.encode(), arr.ctypes.data, out.ctypes.data, n) == 0, op
        return split_records(out.tobytes(), n, kout, nflag)


# ---------------------------------------------------------------- a. pack / unpack
def pack_words():
    rng = random.Random(2911)
    vals = wl.extreme_felts() + [0, 1, P - 1, 1 << 251, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(512)]
    arr = np.zeros((len(vals), 1, NL), dtype=np.int64)
    for i, v in enumerate(vals):
        arr[i, 0, :8] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    return vals, arr.astype(np.uint32).view(np.int32)


def check_pack(vals, packed, unpacked):
    words = packed[:, 0, :8].astype(np.int64) & 0xFFFFFFFF
    got = [sum(int(w) << (32 * k) for k, w in enumerate(row)) for row in words]
    assert got == vals  # fe_pack(fe_unpack(u)) == u
    assert [list(r) for r in unpacked[:, 0].tolist()] == [nform(v) for v in vals]  # the limbs themselves
    return len(vals)


# ---------------------------------------------------------------- b. multiplications
MUL_OPS = ("fe_mul", "fe_sqr", "fe_mul_sub_mul", "fe_mul_add_mul", "fe_mul3_add")  # outputs 2k (column), 2k + 1 (scan)


def mul_patterns():  # the six extreme patterns of tests/test_field_scan_host.py
    ones, zero = [MASK] * 8, [0] * 8
    return [ones + [MASK], zero + [0], zero + [-L8], ones + [-L8], zero + [L8], ones + [L8]]


def mul_tuples():
    """Every 6-tuple of the six patterns: 46 656 items, each pattern in every operand position of every form."""
    pats = np.array(mul_patterns(), dtype=np.int32)
    idx = np.array(list(itertools.product(range(6), repeat=6)), dtype=np.int64)
    return pats[idx]


def mul_random(n=8192, seed=2912):
    """n random N-form elements (limb 8 in [-2^21, 2^21]); item i multiplies elements i .. i + 5 (cyclic)."""
    rng = random.Random(seed)
    el = np.array([[rng.getrandbits(LB) for _ in range(8)] + [rng.randint(-L8, L8)] for _ in range(n)], dtype=np.int32)
    return el[(np.arange(n)[:, None] + np.arange(6)[None, :]) % n]


def check_mul(inp, out):
    v = values(inp)
    a, b, c, d, e, f = (v[:, k] for k in range(6))
    exp = [a * b, a * a, a * b - c * d, a * b + c * d, a * b + c * d + e * f]
    assert is_nform(out)
    got = values(out)
    for k, op in enumerate(MUL_OPS):
        bad = np.nonzero((out[:, 2 * k] != out[:, 2 * k + 1]).any(axis=1))[0]
        assert len(bad) == 0, "%s: scan limbs differ from column limbs, first at item %d" % (op, bad[0])
        bad = np.nonzero((got[:, 2 * k] * RM - exp[k]) % P != 0)[0]
        assert len(bad) == 0, "%s: wrong value, first at item %d" % (op, bad[0])
    return len(inp)


# ---------------------------------------------------------------- c. small ops
def lazy_limbs(rng, v):
    """The value v with one unit of a limb moved to its neighbour: unnormalised limbs, same value."""
    l = nform(v)
    i = rng.randrange(8)
    s = rng.choice((1, -1))
    l[i] += s << LB
    l[i + 1] -= s
    return l


def small_inputs():
    """{op: (int32 inputs, expected)} for fe_carry, fe_canon, fe_half, fe_to_mont, fe_from_mont, fe_is_zero, fe_eq, fe_is_qr."""
    rng = random.Random(2913)
    kp = [k * P + d for k in range(-15, 16) for d in (-1, 0, 1)]
    res = {}
    # fe_carry: any lazy limbs whose running carry stays inside 32 bits; the value must not change
    lazy = [[rng.randint(-(1 << 30), 1 << 30) for _ in range(NL)] for _ in range(300)]
    lazy += [nform(v) for v in kp] + [lazy_limbs(rng, v) for v in kp]
    res["carry"] = (elems([[l] for l in lazy]), [sum(x << (LB * i) for i, x in enumerate(l)) for l in lazy])
    # fe_canon: N-form or lazy, |value| < 16 p (|limb 8| < 2^28): the inputs of test_field_host's raw-limb test
    vals = [k * P + d for k in range(-15, 16) for d in (-2, -1, 0, 1, 2, 1 << 29, -(1 << 29), 17 << 192, 1 << 250)]
    vals += [rng.randrange(-16 * P + 1, 16 * P) for _ in range(600)]
    canon = [nform(v) for v in vals] + [lazy_limbs(rng, v) for v in vals]
    res["canon"] = (elems([[l] for l in canon]), [v % P for v in vals] * 2)
    # fe_half: N-form, value in (-p, 2p) -> N-form of value / 2 mod p: v / 2 in (-p/2, p) for an even v, (v + p) / 2
    # in (0, 3p/2) for an odd one
    vals = [-P + 1, -P + 2, -1, 0, 1, 2, P - 1, P, P + 1, 2 * P - 2, 2 * P - 1] + [rng.randrange(-P + 1, 2 * P) for _ in range(500)]
    res["half"] = (elems([[nform(v)] for v in vals]), vals)
    # fe_to_mont: canonical -> N-form of x R; fe_from_mont: Montgomery N-form (|value| < 16 p) -> canonical x / R
    vals = wl.extreme_felts() + [rng.randrange(P) for _ in range(300)]
    res["to_mont"] = (elems([[nform(v)] for v in vals]), vals)
    vals = kp + [rng.randrange(-16 * P + 1, 16 * P) for _ in range(400)] + wl.extreme_felts()
    res["from_mont"] = (elems([[nform(v)] for v in vals]), vals)
    # fe_is_zero / fe_eq: k p and k p +- 1, k = -15 .. 15, as N-form limbs
    res["is_zero"] = (elems([[nform(v)] for v in kp]), [v % P == 0 for v in kp])
    base = [0] * len(kp) + [rng.randrange(P) for _ in kp]
    res["eq"] = (elems([[nform(b + v), nform(b)] for b, v in zip(base, kp + kp)]), [v % P == 0 for v in kp + kp])
    # fe_is_qr: non-zero, Montgomery form
    edge = [1, 2, P - 1, P - 2, 1 << 251, 1 << 192, (1 << 29) - 1, 1 << 232, (P - 1) // 2]  # test_field_host.EDGE without 0
    vals = edge + [rng.randrange(1, P) for _ in range(256)]
    res["is_qr"] = (elems([[mont(v, rng.choice((-1, 0, 1)))] for v in vals]), [pow(v, (P - 1) // 2, P) == 1 for v in vals])
    return res


def check_small(op, inp, exp, out, flags):
    n = len(exp)
    if op in ("is_zero", "eq", "is_qr"):
        assert flags[:, 0].tolist() == [int(e) for e in exp], op
        return n
    got = values(out[:, 0]).tolist()
    if op == "carry":
        assert is_nform(out) and got == exp
    elif op == "canon":
        assert got == exp and out.min() >= 0 and out.max() <= MASK
    elif op == "half":
        assert is_nform(out)
        assert all(g == (e + P * (e & 1)) // 2 for g, e in zip(got, exp))  # exact, hence in (-p/2, 3p/2)
    elif op == "to_mont":
        assert is_nform(out) and all((g - e * RM) % P == 0 for g, e in zip(got, exp))
    elif op == "from_mont":
        assert out.min() >= 0 and out.max() <= MASK
        assert all(0 <= g < P and (g * RM - e) % P == 0 for g, e in zip(got, exp))
    else:
        raise KeyError(op)
    return n


# ---------------------------------------------------------------- points
_POINTS = []


def points():
    """48 seeded multiples of EC_GEN and of the Pedersen constant points (oracle.ref_py)."""
    if not _POINTS:
        rng = random.Random(2914)
        bases = [tuple(R.EC_GEN)] + [tuple(R.CONSTANT_POINTS[i]) for i in (0, 2, 250, 254, 502)]
        for i in range(48):
            _POINTS.append(R.ec_mult(rng.randrange(1, N), bases[i % len(bases)]))
        assert len(set(p[0] for p in _POINTS)) == len(_POINTS)
    return _POINTS


def neg(pt):
    return (pt[0], (P - pt[1]) % P)


def xyzz_limbs(pt, z, ks):
    """(x, y) scaled by z into X, Y, ZZ, ZZZ Montgomery limbs, representative number ks[i] of each (x + k p)."""
    z2, z3 = z * z % P, z * z * z % P
    return [mont(pt[0] * z2, ks[0]), mont(pt[1] * z3, ks[1]), mont(z2, ks[2]), mont(z3, ks[3])]


def jac_limbs(pt, z, ks):
    return [mont(pt[0] * z * z, ks[0]), mont(pt[1] * z * z * z, ks[1]), mont(z, ks[2])]


def aff_limbs(pt, ks):
    return [mont(pt[0], ks[0]), mont(pt[1], ks[1])]


def point_pairs(rng, n):
    """n pairs (P1, P2, kind): distinct points, then P2 = P1 and P2 = -P1 (the exceptional additions)."""
    pts = points()
    pairs = []
    for i in range(n):
        a, b = rng.sample(pts, 2)
        pairs.append((a, b, "add"))
    for i in range(16):
        a = pts[(5 * i) % len(pts)]
        pairs.append((a, a, "same"))
        pairs.append((a, neg(a), "opposite"))
    return pairs


GROUP_OPS = ("xyzz_madd", "xyzz_madd_x_only", "xyzz_mmadd", "xyzz_add", "xyzz_add_x_only", "jac_dbl", "jac_madd", "jac_add")


def group_inputs(op):
    """(int32 inputs, [(expected affine point or None, kind)]).  165 items: two full waves and a partial one."""
    rng = random.Random(2915 + GROUP_OPS.index(op))
    ks = lambda k: [rng.choice((-1, 0, 1)) for _ in range(k)]
    z = lambda: rng.randrange(1, P)
    items, exp = [], []
    if op.startswith("jac"):
        for a, b, _ in point_pairs(rng, 165)[:165]:
            if op == "jac_dbl":
                items.append(jac_limbs(a, z(), ks(3)) + [mont(R.ALPHA, rng.choice((-1, 0, 1)))])
                exp.append((R.ec_double(a), "add"))
            elif op == "jac_madd":
                items.append(jac_limbs(a, z(), ks(3)) + aff_limbs(b, ks(2)))
                exp.append((R.ec_add(a, b), "add"))
            else:
                items.append(jac_limbs(a, z(), ks(3)) + jac_limbs(b, z(), ks(3)))
                exp.append((R.ec_add(a, b), "add"))
        return elems(items), exp
    for a, b, kind in point_pairs(rng, 133):
        if op in ("xyzz_madd", "xyzz_madd_x_only"):
            items.append(xyzz_limbs(a, z(), ks(4)) + aff_limbs(b, ks(2)))
        elif op == "xyzz_mmadd":
            items.append(aff_limbs(a, ks(2)) + aff_limbs(b, ks(2)))
        else:
            items.append(xyzz_limbs(a, z(), ks(4)) + xyzz_limbs(b, z(), ks(4)))
        exp.append((R.ec_add(a, b) if kind == "add" else None, kind))
    return elems(items), exp


def _inv(v):
    return pow(int(v), -1, P)


def check_group(op, exp, out, flags):
    """Affine result of both forms against the oracle; the exceptional additions must give ZZ3 = 0 (mod p), and
    fe_is_zero(ZZ3), taken where the addition ran, must say so.  Returns (items, exceptional items)."""
    assert is_nform(out), op
    v = values(out)
    if op.startswith("jac"):
        for i, (pt, _) in enumerate(exp):
            X, Y, Z = (int(t) * _inv(RM) % P for t in v[i])
            zi = _inv(Z)
            assert (X * zi * zi % P, Y * zi * zi * zi % P) == pt, (op, i)
        return len(exp), 0
    x_only = op.endswith("x_only")
    half = out.shape[1] // 2
    bad = np.nonzero((out[:, :half] != out[:, half:]).any(axis=(1, 2)))[0]
    assert len(bad) == 0, "%s: scan limbs differ from column limbs, first at item %d" % (op, bad[0])
    exceptional = 0
    for i, (pt, kind) in enumerate(exp):
        for form in (0, 1):
            r = v[i, form * half:(form + 1) * half]
            zz = int(r[1] if x_only else r[2])
            if kind != "add":
                assert zz % P == 0 and flags[i, form] == 1, (op, i, kind, form)
                continue
            assert zz % P != 0 and flags[i, form] == 0, (op, i, form)
            assert int(r[0]) * _inv(zz) % P == pt[0], (op, i, form)
            if not x_only:
                assert int(r[1]) * _inv(r[3]) % P == pt[1], (op, i, form)
                assert pow(zz, 3, P) == pow(int(r[3]), 2, P) * RM % P, (op, i, form)  # ZZ^3 = ZZZ^2 (Montgomery form)
        exceptional += kind != "add"
    return len(exp), exceptional


# ---------------------------------------------------------------- e / f. inversions: value classes and wave layouts
# The seed of class R.  test_field_probe_cpu.py shows on the HOST twin that lehmer_bezout converges for every value it
# yields (layouts 1 and 4 and the R lanes of layout 2), so "no fallback in layout 1" does not rest on the device.
SEED_R = 2916


def class_r(n, m=P, seed=SEED_R):
    rng = random.Random(seed)
    return [rng.randrange(1, m) for _ in range(n)]


def class_s(m=P):
    """Values on which the double-steered inversion asks for the divsteps fallback: some batch starts with
    min < 2^-27 max (a partial quotient no int32 matrix holds)."""
    rng = random.Random(2917)
    vals = list(range(1, 65))
    vals += [1 << k for k in sorted(set(LB * i + d for i in range(NL) for d in (-1, 0, 1))) if 0 <= k and (1 << k) < m]
    vals += [m - 1, m - 2, (m + 1) // 2, (m - 1) // 2]
    vals += [(1 << 224) - 1] + [rng.randrange(1, 1 << 224) for _ in range(16)] + [rng.randrange(1, 1 << k) for k in (30, 64, 128, 200)]
    return sorted(set(vals))


def class_z(m=P, kmax=15):
    return [k * m for k in range(-kmax, kmax + 1)]


def class_u(m=P, ks=(-2, -1, 0, 1, 2, 3), n=64):
    return [x + k * m for k in ks for x in class_r(n, m)]


LAYOUTS = (1, 2, 3, 4)
PARTIAL = 37  # every layout runs with n = 64 m and again with n = 64 m + 37: a last wave with lanes off


def layout(which, m=P, group=1, unreduced=True, kmax=15, u_ks=(-2, -1, 0, 1, 2, 3)):
    """The values of wave layout `which`, as (values, class letter of every value), for 64 / group values per wave
    (group = 4: one value per DPP quad).  The list ends with the partial wave.
      1  every lane from R            2  one lane of every wave from S, the rest from R
      3  every lane from S or Z       4  unreduced representatives x + k m of R values
    unreduced = False: the op takes canonical input only (no layout 4, and Z is the single value 0);
    kmax, u_ks: the multiples of m that Z and U reach (the op's input range)."""
    per, part = 64 // group, -(-PARTIAL // group)
    s = class_s(m)
    if which == 1:
        n = 4 * per + part
        return class_r(n, m), "R" * n
    if which == 2:
        waves = len(s)  # every S value gets a wave of its own; the partial wave takes the first again
        r = iter(class_r(64 * (waves + 1), m))
        vals, cls = [], ""
        for w in range(waves + 1):
            size = per if w < waves else part
            at = (7 * w + 5) % size
            vals += [s[w % len(s)] if i == at else next(r) for i in range(size)]
            cls += "".join("S" if i == at else "R" for i in range(size))
        return vals, cls
    if which == 3:
        z = class_z(m, kmax) if unreduced else [0]
        pool = [(v, "S") for v in s]
        for i, v in enumerate(z):  # spread out: every wave, of 16 quads too, keeps an S value (an all-Z wave converges)
            pool.insert(min(len(pool), 5 * i + 2), (v, "Z"))
        n = -(-len(pool) // per) * per + part
        pool = [pool[i % len(pool)] for i in range(n)]
        return [v for v, _ in pool], "".join(c for _, c in pool)
    if which == 4:
        assert unreduced
        u = class_u(m, u_ks, per)
        u = u + u[:part]
        return u, "U" * len(u)
    raise KeyError(which)


# family -> (ops, op that reports lehmer_bezout's flag on the same input, modulus, keyword arguments of layout())
INV_FAMILIES = {
    # Montgomery-form field inversions: the raw limbs ARE the integer that enters the gcd (any representative)
    "mont": (("fe_inv", "fe_inv_lehmer", "fe_inv_gcd", "fe_inv_gcd_var"), "lehmer_bezout", P, {}),
    # plain inversions: canonical input
    "plain": (("fe_inv_plain_lehmer", "fe_inv_plain_gcd", "fe_inv_plain_gcd_var"), "lehmer_bezout", P, {"unreduced": False}),
    # modulo the curve order: a Montgomery-form input in (-p, 2p), brought to [0, N) before the gcd, so only k = -1, 0, 1
    # of U and 0, +-N of Z (lehmer_bezout states D = 0 for a multiple of the modulus: the answer is 0).
    "order": (("fn_inv", "fn_inv_var"), "lehmer_bezout_n", N, {"kmax": 1, "u_ks": (-1, 0, 1)}),
}


def inv_input(family, which):
    """(int32 inputs (n, 1, 9), values, classes) of one family and layout; None when the family has no such layout."""
    _, _, m, kw = INV_FAMILIES[family]
    if which == 4 and not kw.get("unreduced", True):
        return None
    vals, cls = layout(which, m, **kw)
    return elems([[nform(v)] for v in vals]), vals, cls


def check_inv(op, vals, out):
    """out: the op's limbs for the first len(out) values.  Exact: pow(x, -1, m) with the Montgomery factor applied."""
    got = values(out[:, 0]).tolist()
    for i, (g, v) in enumerate(zip(got, vals)):
        if op.startswith("fn_"):  # input V = a R mod N, output N-form of a^-1 R = R^2 / V mod N
            assert (g - (pow(v, -1, N) * RM * RM if v % N else 0)) % N == 0, (op, i, hex(v))
        elif "plain" in op:  # canonical in, canonical out, 0 -> 0
            assert g == (pow(v, -1, P) if v % P else 0), (op, i, hex(v))
        else:  # input V = a R, output N-form of a^-1 R = R^2 / V
            assert (g - (pow(v, -1, P) * RM * RM if v % P else 0)) % P == 0, (op, i, hex(v))
    if "plain" in op:
        assert out.min() >= 0 and out.max() <= MASK, op
    else:
        assert is_nform(out), op
    return len(got)


def check_bezout(op, vals, out, flags):
    """lehmer_bezout itself: where it answers true, D sign is the inverse (0 for a multiple of the modulus)."""
    m = N if op.endswith("_n") else P
    got = values(out[:, 0]).tolist()
    for i, (d, v) in enumerate(zip(got, vals)):
        if flags[i, 0]:
            sign = -1 if flags[i, 1] else 1
            assert (d * sign * v - (1 if v % m else 0)) % m == 0 and abs(d) < 2 * m, (op, i, hex(v))


# quad inversions: one value per quad, on all four lanes
QUAD_INV = {  # op -> (keyword arguments of layout(), output form)
    "inv_plain_quad": ({}, "plain"),
    "inv_plain_quad_divsteps": ({"unreduced": False}, "plain"),
    "inv_quad": ({}, "mont"),
    "inv_quad_plain": ({}, "mont_plain"),
}


def quad_inv_input(op, which):
    kw, _ = QUAD_INV[op]
    if which == 4 and not kw.get("unreduced", True):
        return None
    vals, cls = layout(which, P, group=4, **kw)
    return elems([[nform(v)] for v in vals for _ in range(4)]), vals, cls


def check_quad_inv(op, vals, out):
    """out: (4 * quads, 1, 9); every one of the four lanes must hold the inverse."""
    form = QUAD_INV[op][1]
    got = values(out[:, 0]).tolist()
    assert len(got) % 4 == 0
    for i, g in enumerate(got):
        v = vals[i // 4]
        inv = pow(v, -1, P) if v % P else 0
        if form == "plain":
            assert g == inv, (op, i, hex(v))
        else:  # fe_mul(plain inverse, R^3 or R^2): V^-1 R^2, or V^-1 R without the Montgomery factor
            assert (g - inv * (RM * RM if form == "mont" else RM)) % P == 0, (op, i, hex(v))
    assert is_nform(out), op
    return len(got) // 4


# ---------------------------------------------------------------- g. shared quad inversion
def shared_quad_input(log_distinct):
    """Montgomery-form non-zero values, 2 or 4 distinct ones per quad: quads that hold x, p - x, 1, p - 1 together,
    then seeded ones.  41 quads: two full waves and a partial one.  Returns (inputs, the plain value of every lane)."""
    rng = random.Random(2918 + log_distinct)
    x = class_r(8, P, seed=2919)
    quads = []
    for a in x:
        quads += [[a, P - a, 1, P - 1], [1, P - 1, a, P - a], [P - a, a, P - 1, 1], [a, 1, P - a, P - 1]]
    while len(quads) < 41:
        quads.append(rng.sample(class_r(64, P, seed=2920), 4))
    if log_distinct == 1:  # lanes {0, 1} one value, lanes {2, 3} another
        quads = [[q[0], q[0], q[1], q[1]] for q in quads]
    vals = [v for q in quads for v in q]
    return elems([[mont(v, rng.choice((-1, 0, 1)))] for v in vals]), vals


def check_shared_quad(plain, vals, out):
    got = values(out[:, 0]).tolist()
    for i, (g, v) in enumerate(zip(got, vals)):  # each lane its OWN inverse: Montgomery form, or plain
        assert (g - pow(v, -1, P) * (1 if plain else RM)) % P == 0, (plain, i, hex(v))
    assert is_nform(out)
    return len(got) // 4


# ---------------------------------------------------------------- h. quad additions
def quad_add_input(op):
    """(inputs, [(expected sum of lanes 0,1 / of lanes 2,3 ..., kind)] per quad).  A different pair in every quad.
    qadd / qadd_x_only: lanes 0,1 carry P1 and lanes 2,3 carry P2 (a = X | Y, b = ZZ | ZZZ); both pairs get P1 + P2.
    qmmadd: lanes 0,1 add the affine pair A, lanes 2,3 the pair B; every other quad passes the second point of a pair
    as -(-Q): the entry of -Q with its y limbs negated, the B = 2 case of the formula's comment."""
    rng = random.Random(2921 + len(op))
    ks = lambda k: [rng.choice((-1, 0, 1)) for _ in range(k)]
    z = lambda: rng.randrange(1, P)
    lanes, exp = [], []
    pairs = point_pairs(rng, 41)  # 41 + 32 quads = 292 lanes: four full waves and a partial one
    if op == "qmmadd":
        for i, (a, b, kind) in enumerate(pairs):
            c, d, kind2 = pairs[(i + 7) % len(pairs)]
            recs = []
            for (p1, p2) in ((a, b), (c, d)):
                l1, l2 = aff_limbs(p1, ks(2)), aff_limbs(p2, ks(2))
                if i % 2:
                    l2 = [l2[0], [-t for t in mont(P - p2[1], 0)]]  # -(y of -Q): the same point, limbs in (-2^29, 0]
                recs.append(l1 + l2)
            lanes += [recs[0], recs[0], recs[1], recs[1]]
            exp.append(((R.ec_add(a, b) if kind == "add" else None, kind), (R.ec_add(c, d) if kind2 == "add" else None, kind2)))
        return elems(lanes), exp
    for a, b, kind in pairs:
        p1, p2 = xyzz_limbs(a, z(), ks(4)), xyzz_limbs(b, z(), ks(4))
        lanes += [[p1[0], p1[2]], [p1[1], p1[3]], [p2[0], p2[2]], [p2[1], p2[3]]]
        s = (R.ec_add(a, b) if kind == "add" else None, kind)
        exp.append((s, s))
    return elems(lanes), exp


def check_quad_add(op, exp, out, flags):
    """Per lane a / b is an affine coordinate of the sum: x on even lanes, y on odd ones (x on every lane for the
    x-only form).  Exceptional quads: b = 0 (mod p) on every lane, and fe_is_zero(b) taken on the device says so."""
    assert is_nform(out[:, 1]), op  # b is a product; a may be the lazy difference Y3
    v = values(out)
    exceptional = 0
    for q, halves in enumerate(exp):
        for lane in range(4):
            pt, kind = halves[lane >> 1]
            a, b = int(v[4 * q + lane, 0]), int(v[4 * q + lane, 1])
            if kind != "add":
                assert b % P == 0 and flags[4 * q + lane, 0] == 1, (op, q, lane, kind)
                continue
            assert b % P != 0 and flags[4 * q + lane, 0] == 0, (op, q, lane)
            want = pt[0] if (op == "qadd_x_only" or lane % 2 == 0) else pt[1]
            assert a * _inv(b) % P == want, (op, q, lane)
        exceptional += halves[0][1] != "add" or halves[1][1] != "add"
    return len(exp), exceptional
