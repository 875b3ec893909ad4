"""Cases of the dense AIR tests (tests/test_gpu_air_dense.py, checked without a GPU by tests/test_air_cases_cpu.py): the item
counts and edge operands of the witness generators of csrc/stark.hip and csrc/builtins.hip, the sizes, shifts and columns
the composition kernels run on, the lengths of the rc16 product with the launch plan sp_rc16_product_dev takes at each of
them (restated from scan_mul, SCAN_L and INV_K of builtins.hip), the operands of sp_felt_add_dev and the shard shapes.
Pure Python on oracle/stark_ref.py, oracle/ref_py.py and workloads.extreme_felts: neither torch nor the library is
imported here.  A change of INV_K, SCAN_L or the serial limit of scan_mul moves the plan edges:
test_air_cases_cpu.py fails until PRODUCT_LENGTHS is redone.

Oracle time of every case list (seconds of one CPU core, printed by test_air_cases_cpu.py::test_oracle_times with -s; a
GPU test pays its list's time plus the launches):
    pedersen witness, 65 pairs                      1.0    (1, 64 and 65 items share it: a batch's trace is its items' traces)
    pedersen_hash of the 65 pairs                   0.6
    ec_ladder witness, 65 ladders                   1.6
    ecdsa witness, 65 instances of 29 distinct      4.3    2.3 the traces, 2.0 signing and ecdsa_instance (the reference's verify)
    range_check + rc16 witnesses                    0.0
    composition pedersen  log_n 9 / 10 / 12         0.05 / 0.06 / 0.25   per (shift, kind), extreme columns; random ones 0.17 at 12
    composition ec_ladder log_n 8 / 9 / 11          0.02 / 0.04 / 0.15
    composition ecdsa     log_n 10 / 11             0.14 / 0.26          random columns 0.3 / 0.35
    composition range_check log_n 7 / 8 / 11        0.00 / 0.00 / 0.04
    composition rc16      log_n 3 / 4 / 5 / 8       0.00 / 0.00 / 0.01 / 0.05   per limb range
    periodic tables, once per (AIR, n, shift)       pedersen 0.13, ec_ladder 0.02, ecdsa 0.5, range_check 0.01
    rc16 product, all eight lengths                 1.0 random, 1.1 extreme
Dropped for time: 65 DISTINCT ecdsa instances cost 9.6 s (0.15 s each with the signing), above the five seconds a list may
take, so lanes 13 .. 61 of the ecdsa batch cycle through ECDSA_PADDING = 13 seeded signatures (13 is prime: no two lanes a power
of two apart hold the same instance).  The counts stay 1, 64 and 65.  Nothing else is thinned: every (size, shift, kind) of
the tables below runs; all 167 tests of test_gpu_air_dense.py take 15 s on an MI355X box, the slowest 2 s."""
import functools
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "stark-perpetual_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import workloads as wl  # noqa: E402
from oracle import ref_py as R  # noqa: E402
from oracle import stark_ref as S  # noqa: E402

P = S.P
N = R.EC_ORDER
EC_GEN = tuple(R.EC_GEN)
MINUS_EC_GEN = (EC_GEN[0], P - EC_GEN[1])

# ---- witness generators: one item per lane, 64 lanes per block ------------------------------------------------------------
ITEM_COUNTS = (1, 64, 65)   # one lane; a full block; a full block and one lane of a second
BATCH = 65                  # the edge batch: its first 1 and 64 items are the two smaller counts
REUSE_ORDER = (65, 1, 64)   # back to back on one stream: the scratch planes are [row][limb][item], the count is the stride
ROWS = {"pedersen": 512, "ec_ladder": 256, "ecdsa": 1024, "range_check": 128, "rc16": 8}
COLUMN_NAMES = {"pedersen": ("s", "px", "py", "lam"), "ec_ladder": ("m", "px", "py", "qx", "qy", "la", "ld"),
                "ecdsa": ("m", "px", "py", "qx", "qy", "la", "ld", "cx", "cy", "cr"), "range_check": ("v",),
                "rc16": ("a", "acc")}

_FULL = (1 << 232) - 1                                                   # limbs 0 .. 7 all 2^29 - 1
_ALT = sum(((1 << 29) - 1) << (29 * k) for k in range(0, 8, 2))          # full and empty limbs alternating
# lane -> (x, y).  Lanes 0, 63 and 64 - the first lane, the last lane of block 0 and the only lane of block 1 - are edges.
PEDERSEN_EDGES = {
    0: (0, 0),                                   # no addition row at all: every lambda is 0, both batched inversions invert 1
    1: (0, 1),
    2: (1, 0),
    3: (P - 1, P - 1),
    4: (2**251, 2**251 - 1),                     # bit 251 alone (the last point of the second base); every bit below it
    5: (2**247, 2**248),                         # the last bit of the first base point, the first bit of the second
    6: (2**248 - 1, 2**251 + 17 * 2**192),       # all of the first base's bits; p - 1
    7: (2**250, 2**249),                         # single high bits
    63: (_FULL, _ALT + (((1 << 19) - 1) << 232)),   # two pairs of workloads.extreme_felts()
    64: (P - 2, (P + 1) // 2),
}
LADDER_SCALARS = (1, 2, 2**250, 2**251 - 1, int("5" * 63, 16) % 2**251, int("a" * 63, 16) % 2**251)
LADDER_SEEDED_MULTIPLE = 0x2F0B7E1D3C5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF  # Q = this * EC_GEN
# the 18 pairs (scalar, base point), base point fastest, sit at lanes 0 .. 14, then 62, 63, 64
LADDER_EDGE_LANES = tuple(range(15)) + (62, 63, 64)
ECDSA_HASHES = (1, 2**251 - 1, 2**248, 0x5A3C0F96E1D2B4788796A5B4C3D2E1F00112233445566778899AABBCCDDEEF)
ECDSA_KEYS = (1, 2, N - 1, 0x1C6E2F0B7E1D3C5A69788796A5B4C3D2E1F00112233445566778899AABBCC01)
# (z, d) pairs oracle/stark_ref.py ecdsa_trace cannot build a witness for (test_air_cases_cpu.py decides): none.  d = 1 makes
# the second ladder run on EC_GEN like the first, d = N - 1 on -EC_GEN; both build.
ECDSA_EXCLUDED = ()
# the 16 (z, d) pairs, key fastest, sit at lanes 0 .. 12, then 62, 63, 64
ECDSA_EDGE_LANES = tuple(range(13)) + (62, 63, 64)
ECDSA_PADDING = 13          # distinct seeded signatures cycled through the other lanes (see the time table above)
RANGE_CHECK_VALUES = (0, 1, 2**64 - 1, 2**64, 2**127, 2**128 - 1)
RANGE_CHECK_OUT_OF_RANGE = (2**128, 2**192 + 5, P - 1)   # the trace kernel shifts across all four words
RANGE_CHECK_COUNT = 11      # 1408 rows: five blocks of 256 and a half
RC16_VALUES = (0, 2**128 - 1, 2**64, 0xFFFF, 0x0001_0000, 0x0001_0002_0003_0004_0005_0006_0007_0008)
RC16_COUNT = 35             # 280 rows: one block of 256 and 24 rows


def _padded(edges, count, fill):
    """`count` items: edges (lane -> item) in place, fill(lane) elsewhere."""
    return [edges[lane] if lane in edges else fill(lane) for lane in range(count)]


@functools.lru_cache(maxsize=None)
def pedersen_batch():
    rng = random.Random(7001)
    pad = [(rng.randrange(P), rng.randrange(P)) for _ in range(BATCH)]
    return tuple(_padded(PEDERSEN_EDGES, BATCH, lambda lane: pad[lane]))


@functools.lru_cache(maxsize=None)
def ladder_edges():
    seeded = R.ec_mult(LADDER_SEEDED_MULTIPLE, EC_GEN)
    combos = [(m, q) for m in LADDER_SCALARS for q in (EC_GEN, MINUS_EC_GEN, seeded)]
    return dict(zip(LADDER_EDGE_LANES, combos))


@functools.lru_cache(maxsize=None)
def ladder_batch():
    rng = random.Random(7002)
    pad = [(rng.randrange(1, 2**251), R.ec_mult(rng.randrange(1, N), EC_GEN)) for _ in range(BATCH)]
    return tuple(_padded(ladder_edges(), BATCH, lambda lane: pad[lane]))


def ecdsa_instance_of(z, d):
    """(z, r, w, Q) of the oracle's signature of z under the key d, as oracle/stark_ref.py ecdsa_instance admits it."""
    t0 = time.perf_counter()
    r, s = R.sign(z, d)
    inst = S.ecdsa_instance(z, r, s, R.ec_mult(d, EC_GEN))
    ORACLE_SECONDS["ecdsa instances"] = ORACLE_SECONDS.get("ecdsa instances", 0.0) + time.perf_counter() - t0
    return inst


@functools.lru_cache(maxsize=None)
def ecdsa_edges():
    pairs = [(z, d) for z in ECDSA_HASHES for d in ECDSA_KEYS if (z, d) not in ECDSA_EXCLUDED]
    return dict(zip(ECDSA_EDGE_LANES, [ecdsa_instance_of(z, d) for z, d in pairs]))


@functools.lru_cache(maxsize=None)
def ecdsa_batch():
    rng = random.Random(7003)
    pad = [ecdsa_instance_of(rng.randrange(1, 2**251), rng.randrange(1, N)) for _ in range(ECDSA_PADDING)]
    return tuple(_padded(ecdsa_edges(), BATCH, lambda lane: pad[lane % ECDSA_PADDING]))


def range_check_batch():
    rng = random.Random(7004)
    edges = RANGE_CHECK_VALUES + RANGE_CHECK_OUT_OF_RANGE
    return edges + tuple(rng.randrange(2**128) for _ in range(RANGE_CHECK_COUNT - len(edges)))


def rc16_batch():
    rng = random.Random(7005)
    return RC16_VALUES + tuple(rng.randrange(2**128) for _ in range(RC16_COUNT - len(RC16_VALUES)))


BATCHES = {"pedersen": pedersen_batch, "ec_ladder": ladder_batch, "ecdsa": ecdsa_batch}
_ITEM_TRACE = {"pedersen": S.pedersen_trace, "ec_ladder": S.ec_ladder_trace, "ecdsa": S.ecdsa_trace}
_trace_cache = {}
ORACLE_SECONDS = {}   # generator -> seconds the oracle has spent on its witnesses in this process (every item is traced once)


def oracle_trace(gen, items):
    """The oracle's witness columns of `items`.  Every generator works item by item - an item owns ROWS[gen] consecutive rows
    of every column - so the trace of a batch is its items' traces one behind the other, and an item is traced once."""
    cols = None
    for item in items:
        key = (gen, item)
        if key not in _trace_cache:
            t0 = time.perf_counter()
            _trace_cache[key] = _ITEM_TRACE[gen]([item])
            ORACLE_SECONDS[gen] = ORACLE_SECONDS.get(gen, 0.0) + time.perf_counter() - t0
        part = _trace_cache[key]
        cols = [list(c) for c in part] if cols is None else [c + p for c, p in zip(cols, part)]
    return cols


# ---- compositions -------------------------------------------------------------------------------------------------------------
# log_n per AIR: the AIR's period (M = the periodic table's length, (i + 4) & (M - 1) wraps inside one period), one size above
# it, and at least four table lengths - two for ecdsa - where the table index wraps and the row index does not
COMPOSITION_LOG_N = {"pedersen": (9, 10, 12), "ec_ladder": (8, 9, 11), "ecdsa": (10, 11), "range_check": (7, 8, 11),
                     "rc16": (3, 4, 5, 8)}
PERIOD_LOG = {"pedersen": 9, "ec_ladder": 8, "ecdsa": 10, "range_check": 7, "rc16": 3}
N_COLS = {"pedersen": 4, "ec_ladder": 7, "ecdsa": 10, "range_check": 1, "rc16": 3}
N_ALPHAS = {"pedersen": 11, "ec_ladder": 12, "ecdsa": 26, "range_check": 2, "rc16": 8}
RANDOM_SHIFT = 0x3D2E1F00112233445566778899AABBCCDDEEFF5A3C0F96E1D2B4788796A5B4C
SHIFTS = (3, 5, RANDOM_SHIFT, P - 3)   # p - 3: every limb but the lowest at its top
SHIFT_IDS = ("3", "5", "random", "p-3")
KINDS = ("random", "extreme")
RC16_LIMB_RANGES = ((0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF), (300, 419))
# Argument edges: shifts every composition call must refuse (x^n - 1 vanishes on the coset), and the log_n on either side
REFUSED_SHIFTS = (0, 1, P - 1)
REFUSED_LOG_N = {"pedersen": (8, 31), "ec_ladder": (7, 31), "ecdsa": (9, 31), "range_check": (6, 31), "rc16": (2, 31)}


def denominators(shift, log_n):
    """shift^n * w4^k - 1 for k = 0 .. 3: what the composition divides by at the points i = k mod 4 of the coset."""
    w4 = S.root_of_unity(2)
    sn = pow(shift, 1 << log_n, P)
    return [(sn * pow(w4, k, P) - 1) % P for k in range(4)]


def felts(kind, count, seed):
    """`count` felts below p: "random" - seeded uniform; "extreme" - each one of workloads.extreme_felts() with probability
    0.85, otherwise random (the mix of test_gpu_stark.py::test_prover_kernels_on_extreme_limb_patterns)."""
    rng = random.Random("%s/%d/%d" % (kind, count, seed))
    if kind == "random":
        return [rng.randrange(P) for _ in range(count)]
    ext = wl.extreme_felts()
    return [rng.choice(ext) if rng.random() < 0.85 else rng.randrange(P) for _ in range(count)]


def composition_inputs(air, log_n, kind, seed=0):
    """(columns of 4n felts, alphas) - and for rc16 the p column, z and nothing else: a composition is a pointwise function
    of whatever its columns hold, so no LDE is taken and the oracle's cost is the composition alone."""
    m = 4 << log_n
    base = 100000 * (sorted(COMPOSITION_LOG_N).index(air) + 1) + 1000 * log_n + seed
    cols = [felts(kind, m, base + c) for c in range(N_COLS[air])]
    alphas = felts(kind, N_ALPHAS[air], base + 50)
    if air != "rc16":
        return cols, alphas
    return cols, alphas, felts(kind, m, base + 60), felts("random", 1, base + 70)[0]


def rc16_periodic_lde(log_n, shift):
    """What oracle/stark_ref.py rc16_composition_on_coset builds for itself: the two period-8 tables on the coset."""
    return [S.lde(col, S.BLOWUP, pow(shift, (1 << log_n) // 8, P)) for col in S.rc16_periodic_columns()]


# ---- the rc16 product: sp_rc16_product_dev's launch plan ------------------------------------------------------------------
INV_K = 16         # felt_batch_inverse_kernel: one inversion per group of 16 consecutive cells
SCAN_L = 64        # felt_scan_chunks_kernel: one thread per chunk of 64 consecutive cells
SCAN_SERIAL = 256  # scan_mul: up to 256 cells one thread scans them all
PRODUCT_LENGTHS = (8, 16, 24, 256, 264, 16384, 16392, 16448)


def product_plan(n):
    """(levels of chunked scanning, the last inversion group is partial, the last chunk of the first level is partial -
    None where no chunk exists)."""
    levels, cells = 0, n
    while cells > SCAN_SERIAL:
        cells = (cells + SCAN_L - 1) // SCAN_L
        levels += 1
    return levels, n % INV_K != 0, (n % SCAN_L != 0) if levels else None


# every class the list must hit, and the length that hits it
PRODUCT_CLASSES = {
    (0, True, None): 8, (0, False, None): 16,
    (1, True, True): 264, (1, False, False): 16384,
    (2, True, True): 16392, (2, False, False): 16448,
}


def product_inputs(n, kind):
    """(a, s, z): full-width felts; z is seeded and differs from every s_j (sp_rc16_product_dev's unchecked precondition)."""
    a, s = felts(kind, n, 900001), felts(kind, n, 900002)
    return a, s, felts("random", 1, 900003 + n)[0]


# ---- sp_felt_add_dev ----------------------------------------------------------------------------------------------------------
FELT_ADD_LENGTHS = (1, 255, 256, 257)


def felt_add_operands(n):
    """n pairs (a, b) of workloads.extreme_felts(): pair 0 sums to 2p - 2, pair 1 to p, pair 2 to 0; then every extreme felt
    e against p - e where that is an extreme felt too (the sum is p), against itself and against p - 1."""
    ext = wl.extreme_felts()
    pairs = [(P - 1, P - 1), (1, P - 1), (0, 0)]
    for e in ext:
        pairs += [(e, P - e)] if e and P - e in ext else []
        pairs += [(e, e), (e, P - 1)]
    return [pairs[i % len(pairs)] for i in range(n)]


# ---- row shards -----------------------------------------------------------------------------------------------------------------
SHARD_LOG_N = 10               # the Pedersen composition, on the LDE of a real trace of two hashes
SHARD_WORLDS = (1, 2, 8)
FOLD_SHARD_LOG_M = 12
FOLD_SHARDS = (1, 4, 16)       # contiguous shards of the lower half
FOLD_TABLE_LOG = 14            # a fold of this size first: the twiddle table is then 4 times the layer's

# ---- regression cases: the smallest input on which a test of test_gpu_air_dense.py once failed ----------------------------
REGRESSIONS = ()               # none: every new test passed on the kernels as they were
