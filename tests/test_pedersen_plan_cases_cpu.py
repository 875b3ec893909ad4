"""The inputs and expectations of the launch-plan tests (tests/pedersen_plan_cases.py) checked without a GPU: the
table's hashes against the two independent restatements, the injected rows against the oracle's own range check, the
batch builder against a direct oracle call, and the size tables against the literal class thresholds."""
import random

import numpy as np

import pedersen_plan_cases as cases
from oracle import cref, ref_py as R

P = R.FIELD_PRIME


def test_constants():
    assert cases.P == P and cases.D == 4099
    assert all(cases.D % k for k in range(2, 65))  # a prime
    pairs = cases.table_pairs()
    assert len(set(pairs)) == cases.D and all(0 <= a < P and 0 <= b < P for a, b in pairs)
    import workloads as wl
    xs, ys = {a for a, _ in pairs}, {b for _, b in pairs}
    for v in list(wl.extreme_felts()) + [P - 1, 2**251, 2**251 - 1]:
        assert v in xs and v in ys, hex(v)
    for row in cases.near_miss_rows():
        assert pairs[row][0] in cases.NEAR_MISSES and pairs[row][1] in cases.NEAR_MISSES
    assert cases.NEAR_MISSES == (P - 1, 2**251, 2**251 - 1)


def test_table_hashes_agree_with_the_plain_restatements():
    pairs = cases.table_pairs()
    tx, ty, th = cases.table()
    assert cases.ints_from_felts(tx) == [a for a, _ in pairs] and cases.ints_from_felts(ty) == [b for _, b in pairs]
    hashes = cases.ints_from_felts(th)
    rng = random.Random(256)
    rows = sorted(set(cases.near_miss_rows()) | set(rng.sample(range(cases.D), 256)))
    got, st = cref.pedersen_hash_many([pairs[i][0] for i in rows], [pairs[i][1] for i in rows])
    assert not any(st)
    assert got == [hashes[i] for i in rows]
    for i in rows[:9] + rng.sample(rows, 16):
        assert R.pedersen_hash(*pairs[i]) == hashes[i], i


def test_inputs_equal_a_direct_oracle_call():
    n = 5000
    x, y, expected = cases.inputs(n, seed=5000)
    assert x.shape == y.shape == expected.shape == (n, 4) and x.dtype == np.uint64
    got, st = cref.opt_pedersen_hash_many(cases.ints_from_felts(x), cases.ints_from_felts(y))
    assert not any(st)
    assert (cases.felts_from_ints(got) == expected).all()
    assert len({tuple(r) for r in x.tolist()}) > 2500  # a draw over the whole table, not a few rows of it
    x2, _, _ = cases.inputs(n, seed=5001)
    assert (x2 != x).any()


def test_bad_positions():
    assert cases.bad_positions(1) == [0]
    assert cases.bad_positions(2) == [0, 1]
    assert cases.bad_positions(3) == [0, 1, 2]
    assert cases.bad_positions(300) == [0, 1, 63, 64, 150, 255, 256, 298, 299]
    assert cases.bad_positions(65536) == [0, 1, 63, 64, 255, 256, 32768, 65534, 65535]
    assert cases.bad_positions(65537) == [0, 1, 63, 64, 255, 256, 32768, 65535, 65536]
    assert cases.bad_positions(70000) == [0, 1, 63, 64, 255, 256, 35000, 65535, 65536, 69998, 69999]
    assert cases.bad_positions(131072) == [0, 1, 63, 64, 255, 256, 65535, 65536, 131070, 131071]
    assert cases.bad_positions(2175001) == [0, 1, 63, 64, 255, 256, 1087500, 2162687, 2162688, 2174999, 2175000]


def test_oracle_flags_exactly_the_injected_rows():
    n = 70000
    x, y, expected = cases.inputs(n, seed=n)
    xi, yi, ei, si = cases.inject(n, x, y, expected)
    bad = cases.bad_positions(n)
    assert np.flatnonzero(si).tolist() == bad and set(si.tolist()) == {0, 1}
    xs, ys = cases.ints_from_felts(xi), cases.ints_from_felts(yi)
    # every pattern is in the batch, the one whose window bits are all zero included
    seen = {(xs[p] if xs[p] >= P else None, ys[p] if ys[p] >= P else None) for p in bad}
    assert seen == set(cases.PATTERNS) and (2**252, None) in seen
    # the row after an injected row holds two near misses, in range by one
    after = [p + 1 for p in bad if p + 1 < n and p + 1 not in bad]
    assert after == [2, 65, 257, 35001, 65537]
    for p in after:
        assert xs[p] in cases.NEAR_MISSES and ys[p] in cases.NEAR_MISSES and si[p] == 0
    assert any(xs[p] == P - 1 for p in after) and any(ys[p] == P - 1 for p in after)
    got, st = cref.opt_pedersen_hash_many(xs, ys)
    assert [i for i, v in enumerate(st) if v] == bad and {st[i] for i in bad} == {1}
    good = si == 0
    assert (cases.felts_from_ints(got)[good] == ei[good]).all()
    # rows the injection did not touch are the rows of the clean batch
    touched = np.zeros(n, dtype=bool)
    touched[bad] = True
    touched[after] = True
    assert (xi[~touched] == x[~touched]).all() and (yi[~touched] == y[~touched]).all()
    assert (ei[~touched] == expected[~touched]).all()


def test_size_tables_hold_every_threshold_and_its_successor():
    assert set(cases.SMALL) >= {1, 2, 3, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 65535,
                                65536}
    assert set(cases.MIXED) >= {65537, 73728, 73729, 81920, 81921, 98304, 98305, 131071, 131072, 131073}
    assert set(cases.LARGE) >= {524288, 524289, 1048576, 1048580, 2097153, 2175001}
    assert max(cases.SMALL) == 65536 < min(cases.MIXED) and max(cases.MIXED) < min(cases.LARGE)
    assert set(cases.FOREST_SHAPES) >= {(1, 1), (1, 2), (3, 1), (3, 2), (3, 3), (3, 5), (5, 6), (5, 10), (3, 10), (3, 11),
                                        (3, 12), (5, 11), (5, 12), (5, 13), (9, 13), (17, 13), (5, 15), (3, 16), (7, 15)}
    level0 = {t << (h - 1) for t, h in cases.FOREST_SHAPES}
    assert level0 >= {69632, 81920, 98304, 114688}
    assert set(cases.LADDER) >= {1, 3, 63, 257, 3000, 9000, 20000, 40000, 70000}
    # the bad leaves of the forest test: (17, 13) once in the whole round, once in the remainder of level 0
    assert [c[:2] for c in cases.FOREST_BAD_LEAF] == [(3, 5), (3, 11), (5, 13), (17, 13), (17, 13)]
    halves = [((tree << 13) + leaf) // 2 < 65536 for t, h, tree, leaf in cases.FOREST_BAD_LEAF if (t, h) == (17, 13)]
    assert halves == [True, False]
    for t, h, tree, leaf in cases.FOREST_BAD_LEAF:
        assert 0 <= tree < t and 0 <= leaf < 1 << h


def test_forest_layout_and_path():
    leaves, want = cases.forest(3, 3)
    offs, rows = cases.forest_offsets(3, 3)
    assert offs == [0, 24, 36, 42] and rows == 45 == want.shape[0]
    got = cases.ints_from_felts(want)
    for t in range(3):
        tree = cases.ints_from_felts(leaves[8 * t: 8 * t + 8])
        levels = cref.merkle_levels(tree)
        for j in range(4):
            w = 8 >> j
            assert got[offs[j] + t * w: offs[j] + (t + 1) * w] == levels[j], (t, j)
        assert got[42 + t] == R.merkle_root(tree)
    assert cases.path_rows(3, 3, 1, 5) == [24 + 4 + 2, 36 + 2 + 1, 42 + 1]
