"""The shared case table of tests/test_tree_diff_cpu.py and tests/test_gpu_tree_diff.py: pairs of tree states and what
differs between them.  Seeded, as tests/tree_scan_cases.py is; its key helpers, query table and pager are used here.

The ground truth of every test is TWO PLAIN DICTIONARIES of what the test wrote into tree A and into tree B (key ->
last value): `differing` lists the keys where A.get(k, empty) != B.get(k, empty), sorted, with both values; `expected`
cuts a range and a page out of that list.  Neither owes anything to the code under test.  The host twin
(state.SparseMerkleTree.diff on the oracle hash) is compared with it on the CPU, the library (sp_tree_diff) with the twin
and with it on the GPU."""
import random

import tree_scan_cases as S

P = S.P
distinct_keys, leaves_for, clustered_keys, pages = S.distinct_keys, S.leaves_for, S.clustered_keys, S.pages


def differing(a, b, empty_leaf=0):
    """What a full diff of A against B must return: sorted (key, leaf in A, leaf in B) where the two differ; a key a
    dictionary lacks reads as the empty leaf."""
    out = []
    for k in sorted(set(a) | set(b)):
        va, vb = a.get(k, empty_leaf), b.get(k, empty_leaf)
        if va != vb:
            out.append((k, va, vb))
    return out


def swapped(triples):
    """The same diff asked the other way round."""
    return [(k, vb, va) for k, va, vb in triples]


def expected(triples, lo=0, hi=None, capacity=None):
    """(page, more) of the sorted triples for one query, by list slicing."""
    inside = [t for t in triples if t[0] >= lo and (hi is None or t[0] <= hi)]
    if capacity is None:
        return inside, False
    return inside[:capacity], len(inside) > capacity


def queries(height, triples, seed=0):
    """tree_scan_cases.queries with `pairs` = the differing keys."""
    return S.queries(height, [(k, va) for k, va, _ in triples], seed)


def pair_batches(height, sizes=(40, 7, 40), seed=0):
    """(start, [(mods_a, mods_b), ...]): both trees first receive `start` (both ends of the key range among its keys),
    then batch r gives A and B DIFFERENT random updates of sizes[r] keys each, and on top of them
      - overwrites a key both hold with two different values,
      - overwrites a key both hold with the same value in both,
      - sets a key both hold back to the empty leaf (0) in ONE tree only (A in even batches, B in odd ones),
      - writes a key in ONE tree only (B in even batches, A in odd ones).
    The four keys are distinct wherever the key space has room (height 1 has two keys: the roles share them there, a
    later role overriding an earlier one)."""
    rng = random.Random(5000 + 100 * seed + height)
    top = (1 << height) - 1
    start = leaves_for(rng, distinct_keys(rng, height, max(sizes[0] // 2, 4), (0, top)))
    a, b, out = dict(start), dict(start), []
    for r, n in enumerate(sizes):
        mods_a = leaves_for(rng, distinct_keys(rng, height, n))
        mods_b = leaves_for(rng, distinct_keys(rng, height, n))
        shared = sorted(set(a) & set(b))
        picks = rng.sample(shared, min(3, len(shared)))
        k_diff, k_same, k_reset = (picks[i % len(picks)] for i in range(3))
        free = [k for k in (k_diff ^ 1, k_same ^ 1, k_reset ^ 1, rng.randrange(top + 1))
                if k <= top and k not in (k_diff, k_same, k_reset)]
        k_only = free[0] if free else k_diff
        one, other = (mods_a, mods_b) if r % 2 == 0 else (mods_b, mods_a)
        mods_a[k_diff], mods_b[k_diff] = rng.randrange(1, P // 2), rng.randrange(P // 2, P)
        mods_a[k_same] = mods_b[k_same] = rng.randrange(1, P)
        one[k_reset] = 0
        other.pop(k_reset, None)
        other[k_only] = rng.randrange(1, P)
        one.pop(k_only, None)
        a.update(mods_a)
        b.update(mods_b)
        out.append((mods_a, mods_b))
    return start, out
