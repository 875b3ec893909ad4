"""Inputs and expected values of the launch-plan tests of the Pedersen dispatcher (tests/test_gpu_pedersen_plans.py,
tests/test_pedersen_plan_cases_cpu.py): a fixed table of distinct operand pairs hashed once by the C oracle, batches of
any size drawn from it (so every output of a 2-million-hash batch is checked bit for bit at the price of 4099 oracle
hashes), out-of-range operands injected at the positions where a kernel variant begins or ends, the batch sizes
at every size-class edge of enqueue_pedersen_impl, and the forest shapes that take sp_merkle_forest_dev through
ped_top_kernel and every class of level 0.  Run as a program it is the child process of the switch test: it checks a
size ladder with injection in a fresh interpreter, under whatever STARKPERP_* switches the parent put into the
environment, and exits non-zero on a mismatch."""
import ctypes
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "stark-perpetual_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

P = 2**251 + 17 * 2**192 + 1
HASH_OK, HASH_OUT_OF_RANGE = 0, 1
D = 4099  # a prime: positions of the table never line up with blocks of 64, 256 or 65 536 hashes
TABLE_SEED = 4099
ROUND = 65536  # hashes of one round of the chip (the default of STARKPERP_SPLIT_LANES)

# in range, and one step away from not being: a range check that is off by one or works on the wrong bits flags them
NEAR_MISSES = (P - 1, 2**251, 2**251 - 1)

# ---- batch sizes, each with the plan it takes under the default switches (the same for 21- and 26-bit windows) ----
SMALL = (
    1,      # eight quads per hash, one hash per wave (dup), a single block
    2,      # eight quads, two hashes
    3,      # eight quads, odd count: the last lane group of the launch is a clamped copy
    2047,   # eight quads, last odd size
    2048,   # eight quads, last size (STARKPERP_QUAD_MAX)
    2049,   # four quads, first size
    4096,   # four quads, last size
    4097,   # two quads, first size
    8192,   # two quads, last size
    8193,   # first size past the quad kernels: 4 lanes per hash, inversion fused (8 lanes would need 65 544 lanes)
    16384,  # 4 lanes fused, last size
    16385,  # 2 lanes fused, first size
    32768,  # 2 lanes fused, last size
    32769,  # 1 lane per hash, four hashes share a fused quad inversion, first size
    65535,  # 1 lane fused, ragged last block
    65536,  # 1 lane fused, last size: one whole round
)
MIXED = (
    ROUND + 1,      # mixed launch, remainder of ONE hash on 8 lanes
    ROUND + 8192,   # mixed, 8 lanes per remainder hash, last size
    ROUND + 8193,   # mixed, 4 lanes, first size
    ROUND + 16384,  # mixed, 4 lanes, last size
    ROUND + 16385,  # mixed, 2 lanes, first size
    ROUND + 32768,  # mixed, 2 lanes, last size (remainder = half a round)
    ROUND + 32769,  # remainder above half a round: plain bulk kernel, ragged last round
    131071,         # plain bulk, one hash short of two rounds
    131072,         # plain bulk, two whole rounds
    131073,         # mixed again: two rounds of bulk + ONE hash
)
LARGE = (
    524288,   # 8 whole rounds: finish kernel with prefix products AND ZZ in LDS, 8 elements per thread (its last size)
    524289,   # mixed, remainder 1; 9 elements per thread: finish kernel with the prefix products alone in LDS
    1048576,  # 16 whole rounds: LDS finish without ZZ, 16 elements per thread (its last size)
    1048580,  # mixed, remainder 4; 17 elements per thread: ped_finish_kernel (prefix products in HBM)
    2097153,  # mixed, remainder 1; 33 elements per thread capped to 32: 65 540 finish threads, above one round
    2175001,  # mixed, remainder 12 313 on 4 lanes; the cap again (34 -> 32), 67 972 finish threads, odd size
)

# ---- forest shapes (n_trees, height): level 0 has n_trees * 2^(height - 1) hashes ----
FOREST_SHAPES = (
    (1, 1),    # 1 hash; ped_top_kernel declines (n_in < 4)
    (1, 2),    # ped_top_kernel with 2 levels left, one block
    (3, 1),    # 3 hashes; ped_top_kernel declines (remaining < 2)
    (3, 2),    # top kernel, 2 levels, 3 blocks
    (3, 3),    # top kernel, 3 levels
    (3, 5),    # top kernel, 4 levels, then ONE level of 3 hashes through the dispatcher (remaining < 2)
    (5, 6),    # top kernel 4 levels, then top kernel 2 levels
    (5, 10),   # level 0 = 2560 hashes: four quads; then top kernel 4 + 4 + 1 level
    (3, 10),   # 1536 hashes, 3072 nodes: the top kernel takes level 0 (4 + 4 + 2 levels)
    (3, 11),   # 3072 hashes: four quads
    (3, 12),   # 6144 hashes: two quads, then four quads
    (5, 11),   # 5120 hashes: two quads
    (5, 12),   # 10 240 hashes: 4 lanes fused
    (5, 13),   # 20 480 hashes: 2 lanes fused
    (9, 13),   # 36 864 hashes: 1 lane fused
    (17, 13),  # 69 632 hashes: mixed, remainder 4096 on 8 lanes (the whole of tree 16)
    (5, 15),   # 81 920 hashes: mixed, remainder 16 384 on 4 lanes
    (3, 16),   # 98 304 hashes: mixed, remainder 32 768 on 2 lanes
    (7, 15),   # 114 688 hashes: plain bulk, ragged last round
)
# (n_trees, height, tree of the bad leaf, leaf inside that tree)
FOREST_BAD_LEAF = (
    (3, 5, 1, 9),         # top kernel (right operand of hash 4 of its tree)
    (3, 11, 1, 1026),     # four quads (left operand)
    (5, 13, 2, 4097),     # 2 lanes fused (right operand)
    (17, 13, 8, 5001),    # mixed: hash 35 268 of level 0, in the bulk part
    (17, 13, 16, 8190),   # mixed: hash 69 631 of level 0, the last one of the remainder
)
LADDER = (1, 3, 63, 257, 3000, 9000, 20000, 40000, 70000)  # the child process (main)


def felts_from_ints(values):
    raw = b"".join([int(v).to_bytes(32, "little") for v in values])
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).astype(np.uint64)


def ints_from_felts(arr):
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]


def table_pairs():
    """The D distinct (x, y) pairs as ints, in table order: every extreme-limb felt once on each side with a random
    partner, the near misses against each other, random pairs for the rest.  Entries [near_miss_rows()] are the
    pairs of two near misses."""
    import workloads as wl
    rng = random.Random(TABLE_SEED)
    pairs, seen = [], set()

    def add(pair):
        if pair not in seen:
            seen.add(pair)
            pairs.append(pair)

    for a in NEAR_MISSES:
        for b in NEAR_MISSES:
            add((a, b))
    for v in wl.extreme_felts():
        add((v, rng.randrange(P)))
        add((rng.randrange(P), v))
    while len(pairs) < D:
        add((rng.randrange(P), rng.randrange(P)))
    assert len(pairs) == D
    return pairs


def near_miss_rows():
    return range(len(NEAR_MISSES) ** 2)


@functools.lru_cache(maxsize=None)
def table():
    """(x, y, hash) of the D pairs as uint64[D, 4]; the hashes from ONE call of the optimised C oracle."""
    from oracle import cref
    pairs = table_pairs()
    got, st = cref.opt_pedersen_hash_many([p[0] for p in pairs], [p[1] for p in pairs])
    assert not any(st)
    arrays = felts_from_ints([p[0] for p in pairs]), felts_from_ints([p[1] for p in pairs]), felts_from_ints(got)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def inputs(n, seed):
    """x, y, expected as uint64[n, 4]: rows of the table picked by a seeded index vector."""
    tx, ty, th = table()
    idx = np.random.RandomState(seed).randint(0, D, size=n)
    return tx[idx], ty[idx], th[idx]


def bad_positions(n):
    """Where out-of-range operands go: both ends of the batch, of its first wave and of its first block, its middle, and
    (above one round) the last hash of the whole rounds and the first of the remainder."""
    pos = {0, 1, 63, 64, 255, 256, n // 2, n - 2, n - 1}
    if n > ROUND:
        m = (n - 1) // ROUND * ROUND  # the largest multiple of ROUND below n
        pos |= {m - 1, m}
    return sorted(p for p in pos if 0 <= p < n)


# (x, y) of an injected row; None keeps the in-range operand the row had
PATTERNS = (
    (P, None),
    (None, P),
    (P + 1, None),
    (None, 2**256 - 1),
    (2**252, None),  # all 252 window bits of x are zero: a check derived from the windows would not see it
    (P, P),
)


def inject(n, x, y, expected):
    """Copies of x, y, expected with an out-of-range operand at every bad_positions(n) row (the patterns in rotation,
    starting at pattern n mod 6 so that a position meets different patterns at different sizes) and, on the row after
    each where that row is free, a pair of in-range near misses with its table hash.  Returns (x, y, expected, status):
    status 1 on the injected rows, 0 elsewhere; `expected` of an injected row is meaningless."""
    tx, ty, th = table()
    x, y, expected = x.copy(), y.copy(), expected.copy()
    status = np.zeros(n, dtype=np.uint8)
    bad = bad_positions(n)
    near = list(near_miss_rows())
    for k, pos in enumerate(bad):
        px, py = PATTERNS[(k + n) % len(PATTERNS)]
        if px is not None:
            x[pos] = felts_from_ints([px])[0]
        if py is not None:
            y[pos] = felts_from_ints([py])[0]
        status[pos] = HASH_OUT_OF_RANGE
        nxt = pos + 1
        if nxt < n and nxt not in bad:
            row = near[(k + n) % len(near)]
            x[nxt], y[nxt], expected[nxt] = tx[row], ty[row], th[row]
    return x, y, expected, status


# ---- the library call and its checks (GPU) ----
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_batch(lib, x, y):
    """sp_pedersen_batch on NumPy buffers, without the Python-side range assertion of the batch modules.  `out` and
    `status` start from patterns no kernel writes, so a row that was left out shows.  Returns (rc, out, status)."""
    n = x.shape[0]
    x, y = np.ascontiguousarray(x, dtype=np.uint64), np.ascontiguousarray(y, dtype=np.uint64)
    out = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    status = np.full(n, 0xEE, dtype=np.uint8)
    rc = lib.sp_pedersen_batch(_ptr(x), _ptr(y), _ptr(out), _ptr(status), n)
    return rc, out, status


def _first(mask):
    rows = np.flatnonzero(mask)
    return "%d rows, first %s" % (rows.size, rows[:8].tolist())


def check_batch(lib, n, seed=None):
    """A clean batch of n (rc 0, every status 0, every row equal to the oracle's) and the same batch with injected
    rows (status exact on every row, every unflagged row equal to the oracle's)."""
    x, y, expected = inputs(n, n if seed is None else seed)
    rc, out, status = run_batch(lib, x, y)
    assert rc == 0, (n, rc)
    assert not status.any(), "n = %d, clean batch: status != 0 on %s" % (n, _first(status != 0))
    wrong = (out != expected).any(axis=1)
    assert not wrong.any(), "n = %d, clean batch: wrong hash on %s" % (n, _first(wrong))
    xi, yi, ei, si = inject(n, x, y, expected)
    rc, out, status = run_batch(lib, xi, yi)
    assert rc == 0, (n, rc)
    assert (status == si).all(), "n = %d, injected at %s: status differs on %s, got %s" % (
        n, bad_positions(n), _first(status != si), status[np.flatnonzero(status != si)[:8]].tolist())
    wrong = (out != ei).any(axis=1) & (si == 0)
    assert not wrong.any(), "n = %d, injected batch: wrong hash on unflagged %s" % (n, _first(wrong))


# ---- forests ----
def forest_offsets(n_trees, height):
    """Row of level j in the level-major buffer of sp_merkle_forest_dev (level j: n_trees << (height - j) rows, tree t
    owns rows [t << (height - j), (t + 1) << (height - j)) of it), and the row count of the buffer."""
    offs, pos = [], 0
    for j in range(height + 1):
        offs.append(pos)
        pos += n_trees << (height - j)
    return offs, pos


@functools.lru_cache(maxsize=None)
def forest(n_trees, height):
    """(leaves uint64[n_trees << height, 4], every node of the forest in the layout of sp_merkle_forest_dev as
    uint64[rows, 4]) - the nodes of each tree from cref.opt_merkle_levels.  Leaves are x operands of the table."""
    from oracle import cref
    tx = table()[0]
    n = 1 << height
    idx = np.random.RandomState(1000 * height + n_trees).randint(0, D, size=n_trees * n)
    leaves = tx[idx]
    offs, rows = forest_offsets(n_trees, height)
    want = np.zeros((rows, 4), dtype=np.uint64)
    for t in range(n_trees):
        levels = cref.opt_merkle_levels(ints_from_felts(leaves[t * n: (t + 1) * n]))
        for j, level in enumerate(levels):
            w = n >> j
            want[offs[j] + t * w: offs[j] + (t + 1) * w] = felts_from_ints(level)
    assert (want[: n_trees * n] == leaves).all()
    leaves.setflags(write=False)
    want.setflags(write=False)
    return leaves, want


def path_rows(n_trees, height, tree, leaf):
    """Rows of the nodes above leaf `leaf` of tree `tree`, up to that tree's root."""
    offs, _ = forest_offsets(n_trees, height)
    return [offs[j] + (tree << (height - j)) + (leaf >> j) for j in range(1, height + 1)]


def main():
    from starkperp import _lib
    lib = _lib.ensure_init()
    for n in LADDER:
        check_batch(lib, n)
    print("pedersen_plan child ok")


if __name__ == "__main__":
    main()
