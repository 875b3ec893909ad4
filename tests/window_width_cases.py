"""Inputs and expected values of the window-width tests (tests/test_gpu_window_widths.py, proven without a GPU by
tests/test_window_width_cases_cpu.py): sp_init accepts window_bits 4 .. 27, the width fixes the Pedersen window plan
(context.hip make_plan: 18 .. 101 windows) and the EC_GEN table (min(width, 22) bits, 12 .. 63 windows), and every hash
kernel cuts its windows out of x || y with code of its own.  Operands are aimed at the windows of ONE width:

  crafted(width)   for every window, one operand pair per extreme raw value of that window - index 0 and index all ones
                   on both signs - with the rest of the string seeded random, plus the range edges;
  tiled(width, n)  a batch of n rows of the width-independent table of pedersen_plan_cases with those pairs scattered
                   over it, so that every kernel of the dispatcher meets them;
  gen_scalars(w)   scalars that single out each window of the fixed-base walk, its partial top window included.

Everything is Python integers; the expected hashes come from ONE call of the C oracle per width, the expected points from
ec_point_cases.gmul."""
import functools
import random

import numpy as np

import ec_point_cases as E
import pedersen_plan_cases as PC

P, N = PC.P, E.N
BITS = 504  # x (252 bits) || y (252 bits)
HALF = 252
WIDTHS = range(4, 28)
DROP_CAP = 4  # patterns per width that no operand below p can carry (crafted)
MASK252 = (1 << HALF) - 1


def plan(width):
    """(start, bits) per window, as context.hip make_plan: as many signed (width + 1)-bit windows as fit below bit 504,
    the remaining low bits - at least one, at most width + 1 - as the unsigned window 0."""
    sw = width + 1
    k = BITS // sw
    w0 = BITS - k * sw
    if w0 == 0:
        k, w0 = k - 1, sw
    return [(0, w0)] + [(w0 + g * sw, sw) for g in range(k)]


def gen_plan(width):
    """(wbits, nwin) of the EC_GEN table, as context.hip init_locked."""
    wbits = min(width, 22)
    return wbits, (252 + wbits - 1) // wbits


def table_bytes(width):
    """What sp_table_bytes reports under this plan: 64 bytes per affine entry, 2^w0 + 2^width per signed window for the
    hash, nwin << wbits for EC_GEN (the optional masked-walk table of 63 * 16 entries not counted)."""
    w0 = plan(width)[0][1]
    wbits, nwin = gen_plan(width)
    return 64 * ((1 << w0) + ((len(plan(width)) - 1) << width) + (nwin << wbits))


def straddler(width):
    """Index of the window that holds bits of both x and y, or None."""
    for g, (s0, nb) in enumerate(plan(width)):
        if s0 < HALF < s0 + nb:
            return g
    return None


def window_of_bit(width, bit):
    return [g for g, (s0, nb) in enumerate(plan(width)) if s0 <= bit < s0 + nb][0]


def raw_window(x, y, s0, nb):
    """The window's bits, re-extracted with plain integer shifts."""
    return ((x | (y << HALF)) >> s0) & ((1 << nb) - 1)


def patterns(width, g):
    """[(raw value, label)] of window g: the four extremes of a signed window (sign bit clear = negative, the index is
    then the complement of the low bits), or of the unsigned window 0."""
    s0, nb = plan(width)[g]
    if g == 0:
        vals = [(0, "zero"), (1, "one"), ((1 << nb) - 1, "all ones"), (1 << (nb - 1), "top bit")]
    else:
        vals = [(0, "negative, index all ones"), ((1 << width) - 1, "negative, index 0"),
                (1 << width, "positive, index 0"), ((1 << nb) - 1, "positive, index all ones")]
    seen, out = set(), []
    for v, label in vals:  # a one-bit window 0 has two distinct values, not four
        if v not in seen:
            seen.add(v)
            out.append((v, label))
    return out


def _place(rng, s0, nb, raw):
    """(x, y) below p whose bits [s0, s0 + nb) of x || y are `raw`, or None when no operand below p can carry them.  The
    other bits are random; where the window sets bit 251 of an operand, that operand's other bits are cleared from the
    top - first bits 192 .. 250, then all of them: the smallest operand that carries the pattern is the last try."""
    mask = ((1 << nb) - 1) << s0
    keep = [MASK252 & ~(mask & MASK252), MASK252 & ~((mask >> HALF) & MASK252)]  # bits of x / y outside the window
    fixed = [(raw << s0) & MASK252, ((raw << s0) >> HALF) & MASK252]
    out = []
    for side in (0, 1):
        rest = rng.randrange(P)
        for clear in (0, ((1 << 251) - 1) ^ ((1 << 192) - 1), MASK252):
            v = fixed[side] | (rest & keep[side] & ~clear)
            if v < P:
                break
        else:
            return None
        out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def crafted(width):
    """(records, dropped): records = [(x, y, window or None, raw or None, label)], dropped = [(window, raw, label)] - the
    patterns no operand below p can carry (only windows that hold string bit 251 or 503 have any)."""
    rng = random.Random(20261020 + width)
    records, dropped = [], []
    pl = plan(width)
    for g, (s0, nb) in enumerate(pl):
        for raw, label in patterns(width, g):
            pair = _place(rng, s0, nb, raw)
            if pair is None:
                dropped.append((g, raw, label))
            else:
                records.append(pair + (g, raw, "window %d %s" % (g, label)))
    for a in PC.NEAR_MISSES:
        for b in PC.NEAR_MISSES:
            records.append((a, b, None, None, "near misses"))
    records.append((0, 0, None, None, "(0, 0)"))
    records.append((P - 1, P - 1, None, None, "(p - 1, p - 1)"))
    g = straddler(width)
    if g is not None:
        s0, nb = pl[g]
        lo = HALF - s0  # bits of the window that lie in x
        # all zeros; all ones where x < p allows it (the window starts at bit 251); and the largest value any operands
        # carry: the x part as in p - 1, the y part all ones
        wanted = [(0, "all zeros"), ((1 << nb) - 1, "all ones"),
                  (((P - 1) >> s0) | ((((1 << (nb - lo)) - 1)) << lo), "x part of p - 1, y part full")]
        for raw, label in wanted:
            pair = _place(rng, s0, nb, raw)
            if pair is not None:
                records.append(pair + (g, raw, "straddling window %d %s" % (g, label)))
    return tuple(records), tuple(dropped)


def crafted_pairs(width):
    return [(r[0], r[1]) for r in crafted(width)[0]]


@functools.lru_cache(maxsize=None)
def crafted_expected(width):
    """The hashes of crafted_pairs(width): one call of the optimised C oracle."""
    from oracle import cref
    pairs = crafted_pairs(width)
    assert len(pairs) <= 4 * 101 + 20
    got, st = cref.opt_pedersen_hash_many([p[0] for p in pairs], [p[1] for p in pairs])
    assert not any(st)
    return tuple(got)


@functools.lru_cache(maxsize=None)
def crafted_arrays(width):
    """(x, y, hash) of the crafted pairs as read-only uint64[m, 4]."""
    pairs = crafted_pairs(width)
    arrays = (PC.felts_from_ints([p[0] for p in pairs]), PC.felts_from_ints([p[1] for p in pairs]),
              PC.felts_from_ints(crafted_expected(width)))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def tiled(width, n, seed=None):
    """x, y, expected as uint64[n, 4]: rows of pedersen_plan_cases.table() with the crafted pairs of `width` once each at
    seeded positions (as many of them as n has rows)."""
    seed = n if seed is None else seed
    x, y, expected = (a.copy() for a in PC.inputs(n, seed))
    cx, cy, ch = crafted_arrays(width)
    m = min(n, cx.shape[0])
    pos = np.random.RandomState(seed + 7919 * width).choice(n, size=m, replace=False)
    x[pos], y[pos], expected[pos] = cx[:m], cy[:m], ch[:m]
    return x, y, expected


# ---- the EC_GEN walk ------------------------------------------------------------------------------------------------
def gen_windows(wbits):
    """(first bit, bits) of the windows of the fixed-base walk: ceil(252 / wbits), the last one partial unless
    wbits | 252."""
    nwin = (252 + wbits - 1) // wbits
    return [(i * wbits, min(wbits, 252 - i * wbits)) for i in range(nwin)]


@functools.lru_cache(maxsize=None)
def gen_scalars(wbits):
    """Scalars in [1, N) for the walk over wbits-bit windows of EC_GEN, distinct, in a fixed order."""
    wins = gen_windows(wbits)
    full = (1 << 252) - 1
    out = []
    for first, nb in wins:
        ones = ((1 << nb) - 1) << first
        out += [ones % N, (full ^ ones) % N, 1 << first]
    out += [1, N - 1, 2**251, 2**251 - 1]
    first, nb = wins[-1]
    top = N >> first  # the largest value of the top window below N: N has low bits set, so top << first < N
    out += [top << first, ((top - 1) << first) | ((1 << first) - 1)]
    out += E.edge_scalars()
    seen, uniq = set(), []
    for k in out:
        if 0 < k < N and k not in seen:
            seen.add(k)
            uniq.append(k)
    return tuple(uniq)


def gen_points(wbits):
    return [E.gmul(k) for k in gen_scalars(wbits)]


SIGN_Z = 0x3D1C8A6F0B5E7C2941F6A3D8E0B7C5A2F4E6D8C0A1B3957F2E4C6A8B0D1F3E5
SIGN_D = 0x3C1E9550E66958296D11B60F8E8E7A7AD990D07FA65D5F7652C4A6C87D4E3CC


@functools.lru_cache(maxsize=None)
def sign_items(wbits):
    """[(z, d, k)] for sp_ecdsa_sign_batch: every generator scalar as the nonce under a fixed z and d; then, on a few of
    them, the two rejections one can solve for (t = z + r d = 0 and w = k / t = 2^251: SP_SIGN_RETRY) and the bad inputs
    k = 0 and k = N.  The expected (status, r, s) is sign_cases.attempt."""
    import sign_cases as SC
    ks = list(gen_scalars(wbits))
    SC.prime_r(ks)
    items = [(SIGN_Z, SIGN_D, k) for k in ks]
    retries = 0
    for k in ks:
        r = SC.r_of(k)
        if not 1 <= r < SC.TWO251:
            continue
        for t in (0, k * pow(SC.TWO251, -1, N) % N):  # t = 0; w = k / t = 2^251
            z = (t - r * SIGN_D) % N
            if z < SC.TWO251:
                items.append((z, SIGN_D, k))
                retries += 1
        if retries >= 12:
            break
    items += [(SIGN_Z, SIGN_D, 0), (SIGN_Z, SIGN_D, N)]
    return tuple(items)


@functools.lru_cache(maxsize=None)
def verify_items(wbits):
    """([(z, r, s)], key) with u1 = z / s equal to every generator scalar in turn: a VALID signature under the key
    (R = u1 G + u2 Q with a drawn u2, r = x(R), s = r / u2, z = u1 s; u2 is redrawn until z, r and 1 / s fit 251 bits),
    and the same signature with r + 1, which must not verify.  The points u2 Q come from the C oracle in one call."""
    from oracle import cref
    d, q = E.golden_keys()[3]
    rng = random.Random(4242 + wbits)
    scalars = gen_scalars(wbits)
    found, todo, tries = {}, list(scalars), 4
    for _ in range(16):  # a draw fits with probability 1/4: rounds of four draws for the scalars still open
        u2s = [rng.randrange(1, N) for _ in range(tries * len(todo))]
        u2q = cref.public_keys_many([u2 * d % N for u2 in u2s])
        for i, u1 in enumerate(todo):
            a = E.gmul(u1)
            for j in range(i * tries, (i + 1) * tries):
                u2, b = u2s[j], tuple(u2q[j])
                if a[0] == b[0]:
                    continue
                r = E.add(a, b)[0]
                s = r * pow(u2, -1, N) % N
                z = u1 * s % N
                if 1 <= r < 2**251 - 1 and s and z < 2**251 and 1 <= pow(s, -1, N) < 2**251:
                    found[u1] = (z, r, s)
                    break
        todo = [u1 for u1 in todo if u1 not in found]
        if not todo:
            break
    assert not todo, "no signature with u1 = %#x" % todo[0]
    items = []
    for u1 in scalars:
        z, r, s = found[u1]
        items += [(z, r, s), (z, r + 1, s)]
    return tuple(items), q


def lincomb_items(wbits):
    """[(a, b, P, result or None)] of a EC_GEN + b P on P = t EC_GEN: a = every generator scalar, b = 1 and 0."""
    t, pt = E.golden_keys()[5]
    out = []
    for a in gen_scalars(wbits):
        for b in (1, 0):
            out.append((a, b, pt, E.gmul(a + b * t)))
    return out


# ---- sparse trees -----------------------------------------------------------------------------------------------------
SPARSE_BATCHES = (1, 40, 600, 3000, 5000)  # keys per update; 5000 puts 4097 .. 8192 hashes on a level (two quads)


def sparse_history(height, empty_leaf, sizes=SPARSE_BATCHES, seed=64):
    """[{key: leaf}] - one dict per update: random keys, dense runs of neighbours (a quarter of each batch, so the levels
    just above the leaves shrink at once), overwrites of keys of the batch before, and resets to the empty leaf."""
    rng = random.Random(seed + height + empty_leaf % 1000)
    size = 1 << height
    history, before = [], []
    for n in sizes:
        n = min(n, size)
        keys = set()
        if n >= 8:
            base = rng.randrange(size - n) if size > 2 * n else 0
            keys.update(range(base, base + n // 4))                      # a dense run
            keys.update(rng.sample(before, min(len(before), n // 8)))    # overwrites and resets
        while len(keys) < n:
            keys.add(rng.randrange(size))
        mods, known = {}, set(before)
        for i, k in enumerate(sorted(keys)):
            reset = k in known and i % 2 == 0
            mods[k] = empty_leaf if reset else rng.randrange(1, P)
        history.append(mods)
        before = sorted(mods)
    return history


@functools.lru_cache(maxsize=None)
def sparse_expected(height, empty_leaf, sizes=SPARSE_BATCHES):
    """(history, [(old root, new root)], the host twin after the last update) - state.SparseMerkleTree on the optimised C
    oracle, computed once."""
    from starkperp import state
    import witness_replay
    history = sparse_history(height, empty_leaf, sizes)
    twin = state.SparseMerkleTree(height, empty_leaf, hash_many=witness_replay.oracle_hash_many)
    roots = [twin.update(mods) for mods in history]
    return history, roots, twin
