"""The case tables of the dense AIR tests (tests/air_cases.py) checked without a GPU: the literal tables are what they
claim, every operand builds its oracle trace and a valid trace's composition is a polynomial of the AIR's degree, every
listed (shift, n) has four nonzero denominators, the rc16 product lengths hit every class of the launch plan restated from
csrc/builtins.hip, and the builders are seeded and below p.  With -s it prints the plan classes, the denominators and the
oracle time of every case list (the numbers in the comment block of air_cases.py)."""
import os
import re
import time

import numpy as np

import air_cases as cases
import transform_cases as tc
import workloads as wl
from oracle import cref
from oracle import ref_py as R
from oracle import stark_ref as S

P = S.P
CSRC = os.path.join(cases.ROOT, "stark-perpetual_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_tables_are_the_literal_ones():
    ext = set(wl.extreme_felts())
    assert cases.ITEM_COUNTS == (1, 64, 65) and cases.BATCH == 65 and sorted(cases.REUSE_ORDER) == [1, 64, 65]
    assert cases.REUSE_ORDER == (65, 1, 64)
    # Pedersen: the listed pairs, two pairs of extreme felts, edges on lanes 0, 63 and 64, random pairs elsewhere
    ped = cases.pedersen_batch()
    listed = [(0, 0), (0, 1), (1, 0), (P - 1, P - 1), (2**251, 2**251 - 1), (2**247, 2**248),
              (2**248 - 1, 2**251 + 17 * 2**192), (2**250, 2**249)]
    assert [ped[lane] for lane in range(8)] == listed and 2**251 + 17 * 2**192 == P - 1
    assert all(v in ext for lane in (63, 64) for v in ped[lane]) and ped[63] != ped[64]
    assert len(ped) == 65 and all(0 <= x < P and 0 <= y < P for x, y in ped)
    assert {0, 63, 64} <= set(cases.PEDERSEN_EDGES) and len(set(ped)) == 65
    assert sum(x >= 2**251 or y >= 2**251 for x, y in ped) >= 4           # bit 251, still below p
    # ladders: six scalars x three base points, on lanes 0 .. 14, 62, 63, 64
    lad = cases.ladder_batch()
    edges = cases.ladder_edges()
    assert sorted(edges) == list(range(15)) + [62, 63, 64] and len(lad) == 65
    assert cases.LADDER_SCALARS[:4] == (1, 2, 2**250, 2**251 - 1)
    assert cases.LADDER_SCALARS[4] == sum(1 << k for k in range(0, 251, 2))
    assert cases.LADDER_SCALARS[5] == sum(1 << k for k in range(1, 251, 2))
    seeded = R.ec_mult(cases.LADDER_SEEDED_MULTIPLE, cases.EC_GEN)
    assert set(edges.values()) == {(m, q) for m in cases.LADDER_SCALARS
                                   for q in (cases.EC_GEN, cases.MINUS_EC_GEN, seeded)}
    assert {m for m, q in edges.values() if q == cases.EC_GEN} >= {1, 2**250, 2**251 - 1}
    assert cases.MINUS_EC_GEN == (R.EC_GEN[0], P - R.EC_GEN[1]) and 0 < cases.LADDER_SEEDED_MULTIPLE < cases.N
    assert all(0 < m < 2**251 and R.is_point_on_curve(*q) for m, q in lad)
    assert all(lad[lane] == edges[lane] for lane in edges) and len(set(lad)) == 65
    # ECDSA: four hashes x four keys, none excluded, on lanes 0 .. 12, 62, 63, 64; 13 seeded signatures elsewhere
    assert cases.ECDSA_HASHES[:3] == (1, 2**251 - 1, 2**248) and cases.ECDSA_KEYS[:3] == (1, 2, cases.N - 1)
    assert 0 < cases.ECDSA_HASHES[3] < 2**251 and 2 < cases.ECDSA_KEYS[3] < cases.N - 1 and cases.ECDSA_EXCLUDED == ()
    sig = cases.ecdsa_batch()
    sig_edges = cases.ecdsa_edges()
    assert sorted(sig_edges) == list(range(13)) + [62, 63, 64] and len(sig) == 65 and len(set(sig_edges.values())) == 16
    assert {(z, q) for z, _, _, q in sig_edges.values()} == {(z, R.ec_mult(d, cases.EC_GEN)) for z in cases.ECDSA_HASHES
                                                           for d in cases.ECDSA_KEYS}
    assert all(sig[lane] == sig_edges[lane] for lane in sig_edges)
    assert len(set(sig)) == 16 + cases.ECDSA_PADDING == 29
    assert all(sig[a] != sig[b] for a in range(13, 62) for b in range(a + 1, 62) if (b - a) & (b - a - 1) == 0)
    # range check and rc16
    assert cases.RANGE_CHECK_VALUES == (0, 1, 2**64 - 1, 2**64, 2**127, 2**128 - 1)
    assert cases.RANGE_CHECK_OUT_OF_RANGE == (2**128, 2**192 + 5, P - 1)
    rc = cases.range_check_batch()
    assert len(rc) == 11 and rc[:9] == cases.RANGE_CHECK_VALUES + cases.RANGE_CHECK_OUT_OF_RANGE and 128 * len(rc) % 256
    assert cases.RC16_VALUES[:5] == (0, 2**128 - 1, 2**64, 0xFFFF, 0x10000)
    assert len({(cases.RC16_VALUES[5] >> (16 * k)) & 0xFFFF for k in range(8)}) == 8
    r16 = cases.rc16_batch()
    assert len(r16) == 35 and r16[:6] == cases.RC16_VALUES and all(0 <= v < 2**128 for v in r16) and 256 < 8 * len(r16) < 512


def test_composition_tables_against_the_kernel_sources():
    assert cases.COMPOSITION_LOG_N == {"pedersen": (9, 10, 12), "ec_ladder": (8, 9, 11), "ecdsa": (10, 11),
                                       "range_check": (7, 8, 11), "rc16": (3, 4, 5, 8)}
    stark, builtins = _source("stark.hip"), _source("builtins.hip")
    # the index masks of the periodic tables: 4 * period points each
    masks = {"pedersen": "(gi & 2047)", "ec_ladder": "(i & 1023)", "ecdsa": "(i & 4095)", "range_check": "(i & 511)"}
    for air, sizes in cases.COMPOSITION_LOG_N.items():
        period = S.AIRS[air]["period"] if air != "rc16" else 8
        assert 1 << cases.PERIOD_LOG[air] == period and sizes[0] == cases.PERIOD_LOG[air]   # M = the table's length
        # four table lengths or more; two for ecdsa, whose table is the longest: the table index wraps there too
        assert sizes[-1] >= cases.PERIOD_LOG[air] + (1 if air == "ecdsa" else 2)
        assert cases.REFUSED_LOG_N[air] == (sizes[0] - 1, 31)
        if air == "rc16":
            assert "(i & 31)" in builtins and cases.N_COLS[air] == 3 and cases.N_ALPHAS[air] == S.N_RC16_CONSTRAINTS
        else:
            assert masks[air] in stark and "%d" % (4 * period - 1) in masks[air]
            assert cases.N_COLS[air] == S.AIRS[air]["n_cols"] and cases.N_ALPHAS[air] == S.AIRS[air]["n_constraints"]
    assert cases.RC16_LIMB_RANGES == ((0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF), (300, 419))
    assert cases.KINDS == ("random", "extreme") and len(cases.SHIFT_IDS) == len(cases.SHIFTS)
    assert cases.SHARD_LOG_N == 10 and cases.SHARD_WORLDS == (1, 2, 8)
    assert (cases.FOLD_SHARD_LOG_M, cases.FOLD_SHARDS, cases.FOLD_TABLE_LOG) == (12, (1, 4, 16), 14)


def test_every_listed_shift_has_nonzero_denominators():
    assert cases.SHIFTS[:2] == (3, 5) and cases.SHIFTS[3] == P - 3 and 1 < cases.RANDOM_SHIFT < P - 1
    sizes = sorted({n for v in cases.COMPOSITION_LOG_N.values() for n in v})
    for shift, name in zip(cases.SHIFTS, cases.SHIFT_IDS):
        assert 0 < shift < P
        for log_n in sizes:
            dens = cases.denominators(shift, log_n)
            assert all(d != 0 for d in dens), (name, log_n)
            assert (pow(shift, 4 << log_n, P) != 1) == all(d != 0 for d in dens)
            print("shift %-6s log_n %2d  x^n - 1 at i mod 4: %s" % (name, log_n, " ".join("%016x.." % (d >> 188) for d in dens)))
    # and the shifts the library must refuse have a zero among them at every size
    w_4n = S.root_of_unity(9 + 2)
    for log_n in sizes:
        for shift in cases.REFUSED_SHIFTS[1:]:
            assert 0 in cases.denominators(shift, log_n), (shift, log_n)
    assert 0 in cases.denominators(w_4n, 9) and cases.REFUSED_SHIFTS == (0, 1, P - 1)


# ---- the operands build their traces, and valid traces compose to polynomials -----------------------------------------------
def _pow2_items(items):
    count = 1 << (len(items) - 1).bit_length()
    return [items[i % len(items)] for i in range(count)]


def _composition_is_low_degree(air, cols, max_deg_of_n):
    n = len(cols[0])
    lde = cref.lde_dense(tc.felts_from_ints([v for c in cols for v in c]).reshape(len(cols), n, 4), 2, S.GEN)
    lde = [tc.ints_from_felts(c) for c in lde]
    alphas = cases.felts("random", cases.N_ALPHAS[air], 31)
    comp = S.composition_on_coset(lde, S.periodic_lde(n, air=air), n, alphas, air=air)
    return S.poly_degree_bound_check(comp, S.GEN, max_deg_of_n(n))


def test_edge_operands_build_valid_witnesses():
    """The bound is the one tests/test_gpu_stark.py checks the same AIR's composition against: 3n - 1 (for ecdsa and
    range_check, which it checks through verify_proof's final layer, the same 3n - 1).  Only the listed edge operands are
    composed, repeated up to the next power of two: the seeded padding of the 65-item batches is traced (below) but adds
    nothing to this check."""
    deg = lambda n: 3 * n - 1
    ped = [cases.pedersen_batch()[lane] for lane in sorted(cases.PEDERSEN_EDGES)]
    assert _composition_is_low_degree("pedersen", cases.oracle_trace("pedersen", _pow2_items(ped)), deg)
    lad = [cases.ladder_edges()[lane] for lane in sorted(cases.ladder_edges())]
    assert _composition_is_low_degree("ec_ladder", cases.oracle_trace("ec_ladder", _pow2_items(lad)), deg)
    sig = [cases.ecdsa_edges()[lane] for lane in sorted(cases.ecdsa_edges())]
    assert len(sig) == 16
    assert _composition_is_low_degree("ecdsa", cases.oracle_trace("ecdsa", sig), deg)
    assert _composition_is_low_degree("range_check", S.range_check_trace(_pow2_items(list(cases.RANGE_CHECK_VALUES))), deg)
    # a value of 2^128 or more has a trace, which the GPU test compares cell by cell, but no valid one
    for v in cases.RANGE_CHECK_OUT_OF_RANGE:
        assert not _composition_is_low_degree("range_check", S.range_check_trace([v] * 8), deg), hex(v)


def test_every_batch_builds_its_oracle_trace():
    for gen, batch in cases.BATCHES.items():
        cols = cases.oracle_trace(gen, batch())
        assert len(cols) == cases.N_COLS[gen] == len(cases.COLUMN_NAMES[gen])
        assert all(len(c) == 65 * cases.ROWS[gen] for c in cols)
        # a batch's trace is its items' traces one behind the other
        assert cases.oracle_trace(gen, batch()[:2]) == cases._ITEM_TRACE[gen](list(batch()[:2]))
    ped = cases.oracle_trace("pedersen", cases.pedersen_batch())
    assert all(v == 0 for v in ped[3][:512]) and ped[1][511] == R.SHIFT_POINT[0]        # (0, 0): no addition row
    assert ped[1][512 * 3 + 511] == R.pedersen_hash(P - 1, P - 1)
    rc = S.range_check_trace(list(cases.range_check_batch()))
    assert len(rc[0]) == 128 * 11 and rc[0][128 * 8 + 127] == (P - 1) >> 127
    r16 = S.rc16_trace(list(cases.rc16_batch()))
    assert len(r16[0]) == 280 and r16[1][8 * 5 + 7] == cases.RC16_VALUES[5]


def _rc16_composition_is_low_degree(values):
    """The rc16 composition of the padded trace of `values` against the bound of tests/test_gpu_builtins.py, 2n."""
    limbs = {(v >> (16 * k)) & 0xFFFF for v in values for k in range(8)}
    holes = max(limbs) - min(limbs) + 1 - len(limbs)
    total = 1 << (len(values) + -(-holes // 8) - 1).bit_length()
    padded, lo, hi = S.rc16_fill(list(values), total)
    a, acc, s = S.rc16_trace(padded)
    n = len(a)
    z = cases.felts("random", 1, 41)[0]
    p = S.rc16_product_column(a, s, z)
    assert p[-1] == 1
    comp = S.rc16_composition_on_coset([S.lde(c) for c in (a, acc, s)], S.lde(p), n, cases.felts("random", 8, 42), z, lo, hi)
    return S.poly_degree_bound_check(comp, S.GEN, 2 * n)


def test_rc16_edge_values_build_valid_witnesses():
    """Composed in the groups whose limb ranges stay small: a trace must hold every limb between its smallest and its
    largest, so 0xFFFF (limbs 0 and 0xFFFF) alone needs 2^16 cells - 2^17 rows, 2^19 composition points, about 20 s of
    oracle.  That value is checked on the trace domain instead: every constraint of oracle/stark_ref.py
    rc16_constraint_values vanishes on the rows it applies to, which is what the degree bound says of the composition."""
    v = cases.RC16_VALUES
    assert _rc16_composition_is_low_degree([v[0], v[2], v[4], v[5]])     # limbs 0 .. 8
    assert _rc16_composition_is_low_degree([v[1]])                       # limbs 0xFFFF only: rc_min = rc_max
    padded, lo, hi = S.rc16_fill([v[3]], 1 << 14)
    assert (lo, hi) == (0, 0xFFFF)
    a, acc, s = S.rc16_trace(padded)
    n, z = len(a), cases.felts("random", 1, 43)[0]
    p = S.rc16_product_column(a, s, z)
    per = S.rc16_periodic_columns()
    for i in range(n):
        j = (i + 1) % n
        c = S.rc16_constraint_values((a[i], acc[i], s[i]), (a[j], acc[j], s[j]), (per[0][i % 8], per[1][i % 8]), p[i], p[j], z,
                                     lo, hi)
        assert c[0] == 0 and c[1] == 0 and (i == n - 1 or (c[2] == 0 and c[3] == 0)), i
        assert i != 0 or (c[4] == 0 and c[6] == 0)
        assert i != n - 1 or (c[5] == 0 and c[7] == 0)


# ---- the rc16 product's launch plan -------------------------------------------------------------------------------------------
def test_product_lengths_hit_every_plan_class():
    src = _source("builtins.hip")
    assert "constexpr int INV_K = 16;" in src and cases.INV_K == 16
    assert "constexpr int SCAN_L = 64;" in src and cases.SCAN_L == 64
    assert re.search(r"static int scan_mul\(.*?\{\s*if \(n <= 256\) \{\s*hipLaunchKernelGGL\(felt_scan_serial_kernel", src, re.S)
    assert cases.SCAN_SERIAL == 256
    assert "const size_t chunks = (n + SCAN_L - 1) / SCAN_L;" in src
    assert "int rc = scan_mul(scratch, chunks, scratch + 4 * chunks, st);" in src
    assert "const int cnt = (int)(n - first < (size_t)INV_K ? n - first : (size_t)INV_K);" in src
    assert cases.PRODUCT_LENGTHS == (8, 16, 24, 256, 264, 16384, 16392, 16448)
    plans = {n: cases.product_plan(n) for n in cases.PRODUCT_LENGTHS}
    for n, plan in plans.items():
        print("rc16 product of %5d cells: %s, last group of 16 %s, last chunk of 64 %s" % (
            n, ("one thread", "one level of chunks", "two levels of chunks")[plan[0]], "partial" if plan[1] else "full",
            {None: "-", True: "partial", False: "full"}[plan[2]]))
    for cls, n in cases.PRODUCT_CLASSES.items():
        assert plans[n] == cls, (n, plans[n])
    assert {p[0] for p in plans.values()} == {0, 1, 2}
    for level in (0, 1, 2):
        assert {p[1] for p in plans.values() if p[0] == level} == {True, False}, level     # partial and full last group
    for level in (1, 2):
        assert {p[2] for p in plans.values() if p[0] == level} == {True, False}, level     # partial and full last chunk
    # both sides of each edge, exactly one extra chunk
    assert plans[256][0] == 0 and plans[264][0] == 1 and plans[16384][0] == 1 and plans[16392][0] == 2
    assert cases.product_plan(257)[0] == 1 and cases.product_plan(16385)[0] == 2 and 16448 == 16384 + cases.SCAN_L
    assert plans[24][:2] == (0, True) and 264 % 64 == 16392 % 64 == 8
    for kind in cases.KINDS:
        for n in cases.PRODUCT_LENGTHS:
            a, s, z = cases.product_inputs(n, kind)
            assert len(a) == len(s) == n and 0 < z < P and z not in s


# ---- builders ------------------------------------------------------------------------------------------------------------------
def test_builders():
    ext = set(wl.extreme_felts())
    for kind in cases.KINDS:
        a = cases.felts(kind, 4096, 5)
        assert a == cases.felts(kind, 4096, 5) and a != cases.felts(kind, 4096, 6) and all(0 <= v < P for v in a)
        share = sum(v in ext for v in a) / 4096
        assert (0.80 < share < 0.90 and len(ext & set(a)) > 0.9 * len(ext)) if kind == "extreme" else share == 0
    assert sum(v >> 250 for v in cases.felts("random", 4096, 5)) > 512          # the top bits are drawn too
    for air, sizes in cases.COMPOSITION_LOG_N.items():
        got = cases.composition_inputs(air, sizes[0], "extreme")
        assert len(got[0]) == cases.N_COLS[air] and all(len(c) == 4 << sizes[0] for c in got[0])
        assert len(got[1]) == cases.N_ALPHAS[air] and len(got) == (4 if air == "rc16" else 2)
        assert got[0][0] != got[0][-1] or cases.N_COLS[air] == 1
        assert got[0] != cases.composition_inputs(air, sizes[1], "extreme")[0][: len(got[0])]
    per = cases.rc16_periodic_lde(3, 5)
    assert len(per) == 2 and len(per[0]) == 32
    assert cases.FELT_ADD_LENGTHS == (1, 255, 256, 257)
    for n in cases.FELT_ADD_LENGTHS:
        pairs = cases.felt_add_operands(n)
        assert len(pairs) == n and all(a in ext and b in ext for a, b in pairs)
        sums = {a + b for a, b in pairs}
        assert 2 * P - 2 in sums
        if n > 1:
            assert P in sums and min(sums) == 0 and any(0 < v < P for v in sums) and any(P < v < 2 * P - 2 for v in sums)
    assert cases.REGRESSIONS == ()


# ---- oracle times ---------------------------------------------------------------------------------------------------------------
def test_oracle_times():
    """Measured, printed, never asserted on: the numbers of the comment block of air_cases.py."""
    def timed(label, fn):
        t0 = time.perf_counter()
        out = fn()
        print("oracle time  %-48s %6.2f s" % (label, time.perf_counter() - t0))
        return out

    # the witnesses: air_cases.oracle_trace keeps the time of every item it traces (once per process, whichever test asks first)
    for gen, batch in cases.BATCHES.items():
        cases.oracle_trace(gen, batch())
    distinct = {gen: len({k for k in cases._trace_cache if k[0] == gen}) for gen in cases.BATCHES}
    for gen in cases.BATCHES:
        print("oracle time  %-48s %6.2f s" % ("%s witness, %d distinct items" % (gen, distinct[gen]), cases.ORACLE_SECONDS[gen]))
    print("oracle time  %-48s %6.2f s" % ("ecdsa: signing and ecdsa_instance, 29 signatures", cases.ORACLE_SECONDS["ecdsa instances"]))
    assert distinct["ecdsa"] == 29 and distinct["pedersen"] >= 65 and distinct["ec_ladder"] >= 65
    timed("pedersen_hash of the 65 pairs", lambda: [R.pedersen_hash(x, y) for x, y in cases.pedersen_batch()])
    timed("range_check + rc16 witnesses", lambda: (S.range_check_trace(list(cases.range_check_batch())),
                                                   S.rc16_trace(list(cases.rc16_batch()))))
    for air, sizes in cases.COMPOSITION_LOG_N.items():
        for log_n in sizes:
            n = 1 << log_n
            if air == "rc16":
                cols, alphas, p, z = cases.composition_inputs(air, log_n, "extreme")
                out = timed("composition rc16 log_n %d, one limb range" % log_n,
                            lambda: S.rc16_composition_on_coset(cols, p, n, alphas, z, 0, 0xFFFF, shift=5))
            else:
                cols, alphas = cases.composition_inputs(air, log_n, "extreme")
                per = timed("periodic tables %s log_n %d" % (air, log_n), lambda: S.periodic_lde(n, 5, air=air))
                out = timed("composition %s log_n %d" % (air, log_n),
                            lambda: S.composition_on_coset(cols, per, n, alphas, shift=5, air=air))
            assert len(out) == 4 * n
    for kind in cases.KINDS:
        timed("rc16 product, all eight lengths, %s" % kind,
              lambda: [S.rc16_product_column(*cases.product_inputs(n, kind)) for n in cases.PRODUCT_LENGTHS])
    assert np.array_equal(tc.felts_from_ints([1, P - 1])[:, 0], np.array([1, (P - 1) & (2**64 - 1)], dtype=np.uint64))
