"""The shared case table of tests/test_tree_scan_cpu.py and tests/test_gpu_tree_scan.py: tree states and the
(lo, hi, capacity) queries asked of them.  Seeded, as tests/witness_update_cases.py is.

The ground truth of every test is a PLAIN DICTIONARY of what the test wrote (key -> last value): `live` drops the
values equal to the empty leaf and sorts, `expected` cuts a range and a page out of it.  Neither owes anything to the
code under test.  The host twin (state.SparseMerkleTree.scan on the oracle hash) is compared with it on the CPU, the
library (sp_tree_scan) with the twin and with it on the GPU."""
import random

from oracle import ref_py as R

P = R.FIELD_PRIME


def distinct_keys(rng, height, n, forced=()):
    out = set(forced)
    room = min(n, 1 << height)
    while len(out) < room:
        out.add(rng.randrange(1 << height))
    return sorted(out)


def leaves_for(rng, keys):
    return {k: rng.randrange(1, P) for k in keys}


def live(written, empty_leaf=0):
    """What a full scan must return: the sorted (key, leaf) pairs whose last written value is not the empty leaf."""
    return sorted((k, v) for k, v in written.items() if v != empty_leaf)


def expected(pairs, lo=0, hi=None, capacity=None):
    """(page, more) of the sorted pairs `pairs` for one query, by list slicing."""
    inside = [(k, v) for k, v in pairs if k >= lo and (hi is None or k <= hi)]
    if capacity is None:
        return inside, False
    return inside[:capacity], len(inside) > capacity


def batches(height, sizes=(40, 7, 40), seed=0):
    """A sequence of updates: the first writes both ends of the key range, each later one overwrites two written keys,
    sets one written key BACK TO THE EMPTY LEAF (0) and writes the sibling of the largest key."""
    rng = random.Random(4000 + 100 * seed + height)
    top = (1 << height) - 1
    written, out = {}, []
    for r, n in enumerate(sizes):
        if r == 0:
            mods = leaves_for(rng, distinct_keys(rng, height, n, (0, top)))
        else:
            held = sorted(written)
            mods = leaves_for(rng, distinct_keys(rng, height, n, tuple(held[:2]) + (held[-1] ^ 1,)))
            if len(held) > 2:
                mods[held[len(held) // 2]] = 0
        written.update(mods)
        out.append(mods)
    return out


def queries(height, pairs, seed=0):
    """[(name, lo, hi, capacity)] for a state whose live pairs are `pairs`: the whole range, the edges of the key
    range, single keys written and not, bounds just beside written keys, small pages.  Only queries with
    0 <= lo <= hi < 2^height are produced."""
    rng = random.Random(77 + seed)
    top = (1 << height) - 1
    keys = [k for k, _ in pairs]
    out = [("everything", 0, top, None), ("[0, 0]", 0, 0, None), ("[top, top]", top, top, None),
           ("page of 1", 0, top, 1), ("page of 7", 0, top, 7), ("upper half", (top >> 1) + 1, top, None)]
    if keys:
        mid = keys[len(keys) // 2]
        out += [("one written key", mid, mid, None), ("one written key, page of 1", mid, mid, 1),
                ("from a written key", mid, top, 3), ("up to a written key", 0, mid, None),
                ("just above a written key", mid + 1, top, None), ("just below a written key", 0, mid - 1, None),
                ("between two written keys, both excluded", keys[0] + 1, keys[-1] - 1, None),
                ("exactly n", 0, top, len(keys)), ("n - 1", 0, top, max(1, len(keys) - 1)), ("n + 1", 0, top, len(keys) + 1)]
        free = [k for k in (mid ^ 1, mid ^ 2, rng.randrange(top + 1)) if k not in set(keys) and k <= top]
        out += [("one unwritten key", k, k, None) for k in free[:1]]
    a, b = sorted((rng.randrange(top + 1), rng.randrange(top + 1)))
    out.append(("a random interval", a, b, 5))
    return [(name, lo, hi, cap) for name, lo, hi, cap in out if 0 <= lo <= hi <= top]


def clustered_keys(n_cluster=600, n_far=100, seed=5):
    """Height-64 keys for the cut: `n_cluster` of them under ONE level-12 node (they share their top 52 bits), the rest
    far apart.  The upper frontiers are then short (about n_far + 1 nodes) and the lower ones long, so a page smaller
    than the answer is cut ABOVE level 0."""
    rng = random.Random(seed)
    base = rng.randrange(1 << 52) << 12
    near = {base | low for low in rng.sample(range(1 << 12), n_cluster)}
    far = set()
    while len(far) < n_far:
        k = rng.randrange(1 << 64)
        if k >> 12 != base >> 12:
            far.add(k)
    return sorted(near | far)


def pages(scan, lo, hi, capacity):
    """Pages through `scan(lo, hi, capacity)` by hand: returns (all pairs, the `more` of every call)."""
    got, mores = [], []
    while True:
        page, more = scan(lo, hi, capacity)
        got += page
        mores.append(more)
        if not more:
            return got, mores
        assert page, "more without a key to resume behind"
        lo = page[-1][0] + 1
