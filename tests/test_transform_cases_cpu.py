"""The case table of the dense transform tests (tests/transform_cases.py) checked without a GPU: its restatement of the
pass plan against the defaults and the functions of csrc/stark.hip, the literal table of plan classes, the sizes the
tests run against the class edges, and the column builders against their definitions."""
import os
import re

import numpy as np

import transform_cases as cases
import workloads as wl

STARK_HIP = os.path.join(cases.ROOT, "stark-perpetual_amd", "csrc", "stark.hip")


def _source():
    with open(STARK_HIP) as f:
        return f.read()


def test_defaults_are_those_of_the_kernel_source():
    src = _source()
    defaults = dict(re.findall(r"#ifndef (SP_NTT_\w+)\n#define \1 (.+?)(?:\s*//.*)?\n", src))
    assert defaults["SP_NTT_TILE_LOG"] == "11" and cases.TILE_LOG == 11
    assert defaults["SP_NTT_SMALL_TILE_LOG"] == "10" and cases.SMALL_TILE_LOG == 10
    assert defaults["SP_NTT_STRIDED_MAX"] == "(SP_NTT_TILE_LOG - 2)" and cases.STRIDED_MAX == cases.TILE_LOG - 2 == 9
    # the functions the table restates, as the source has them
    assert "return tile_log == TILE_LOG ? NTT_STRIDED_MAX : tile_log - 2;" in src
    assert "return 1 + (log_n - tile_log + smax - 1) / smax;" in src
    assert "if (log_n <= SMALL_TILE_LOG) return TILE_LOG;" in src
    assert "if (pad_log_b > SMALL_TILE_LOG) return TILE_LOG;" in src
    assert "return ntt_passes(log_n, SMALL_TILE_LOG) <= ntt_passes(log_n, TILE_LOG) ? SMALL_TILE_LOG : TILE_LOG;" in src
    assert "const int cnt = (rest - (lo - local) + (npass - pi) - 1) / (npass - pi);" in src
    assert "const int r = left == 4 ? 2 : (left >= 3 ? 3 : left);" in src
    assert "if (log_n + log_blowup > 26)" in src and cases.MAX_LOG == 26


def test_plan_classes_are_the_literal_table():
    assert cases.PLAN_CLASSES == (
        (0, 11, "big", 1, ((),) * 12),
        (12, 18, "small", 2, ((2,), (3,), (4,), (5,), (6,), (7,), (8,))),
        (19, 20, "big", 2, ((8,), (9,))),
        (21, 26, "small", 3, ((6, 5), (6, 6), (7, 6), (7, 7), (8, 7), (8, 8))),
    )
    covered = []
    for first, last, tile, passes, strided in cases.PLAN_CLASSES:
        assert len(strided) == last - first + 1
        for log_n, want in zip(range(first, last + 1), strided):
            tile_log, local, got = cases.pass_plan(log_n)
            assert tile_log == (cases.TILE_LOG if tile == "big" else cases.SMALL_TILE_LOG), log_n
            assert local == min(log_n, tile_log) and got == want and 1 + len(got) == passes, log_n
            assert cases.ntt_passes(log_n, tile_log) == passes and local + sum(got) == log_n
            assert all(2 <= c <= cases.strided_max_of(tile_log) for c in got), log_n
            covered.append(log_n)
    assert covered == list(range(cases.MAX_LOG + 1))


def test_stage_groups():
    want = {0: (), 1: (1,), 2: (2,), 3: (3,), 4: (2, 2), 5: (3, 2), 6: (3, 3), 7: (3, 2, 2), 8: (3, 3, 2), 9: (3, 3, 3),
            10: (3, 3, 2, 2), 11: (3, 3, 3, 2)}
    for nst, groups in want.items():
        assert cases.stage_groups(nst) == groups and sum(groups) == nst
    # every strided stage count from 2 to 9 is a grouping of its own: every size from 12 to 21 is its own plan
    plans = {log_n: tuple(cases.stage_groups(c) for c in cases.pass_plan(log_n)[2]) + (cases.pass_plan(log_n)[:2],)
             for log_n in range(12, 22)}
    assert len(set(plans.values())) == 10


def test_padding_keeps_the_big_tile_only_above_the_small_one():
    assert cases.pass_plan(14, 10) == (10, 10, (4,))   # LDE (4, 10): the padding IS the small tile's contiguous pass
    assert cases.pass_plan(18, 11) == (11, 11, (7,))   # LDE (7, 11): the same with the big tile, forced by the padding
    assert cases.pass_plan(18, 10)[0] == 10 and cases.pass_plan(18, 0) == (10, 10, (8,))
    assert cases.pass_plan(26, 12) == (11, 11, (8, 7))  # what a blowup above the tile would ask of the fused path
    assert cases.pass_plan(26) == (10, 10, (8, 8))      # and the plan the unfused path takes for LDE (14, 12)


def test_sizes_run_hold_every_class_edge_and_stage_count():
    assert cases.NTT_DENSE == (11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23)
    assert cases.STRUCTURED == (11, 12, 18, 19, 20, 21)
    assert set(cases.LDE_DENSE) == {(n, b) for n in (10, 11, 16, 17, 18, 19) for b in (1, 2)}
    assert {n + b for n, b in cases.LDE_DENSE} == {11, 12, 13, 17, 18, 19, 20, 21}
    assert cases.LDE_SHIFTS_AT == (17, 2) and cases.LDE_SHIFTS_AT in cases.LDE_DENSE
    assert cases.LDE_TINY_LOG_N == (0, 1, 2, 3) and cases.LDE_TINY_BLOWUPS == (0, 1, 3, 9, 10, 11, 12, 13)
    assert cases.LDE_EDGES == ((4, 10), (7, 11), (14, 12))
    assert cases.COSET_SIZES == (12, 19) and cases.FOLD_SIZES == (1, 2, 3, 9, 14)
    assert all(n + b <= cases.MAX_LOG for n, b in cases.LDE_EDGES + cases.LDE_DENSE)
    dense = cases.transform_sizes_run_densely()
    for first, last, _tile, _passes, _strided in cases.PLAN_CLASSES:
        assert first in dense, first
        assert last in dense, last  # 26 through the unfused LDE (14, 12)
    # the dense NTT and the structured columns, which run the DIF plans with their lazy stores, stop at 23 and 21
    assert max(cases.NTT_DENSE) == 23 and set(cases.NEVER_RUN) == {24, 25} and not dense & set(cases.NEVER_RUN)
    assert set(cases.SPARSE_ONLY) == {22, 26}
    assert {c for log_n in cases.NTT_DENSE for c in cases.pass_plan(log_n)[2]} == set(range(2, 10))
    assert {c for n, b in cases.LDE_DENSE for c in cases.pass_plan(n + b, b)[2]} == {2, 3, 5, 6, 7, 8, 9}  # DIT plans
    assert {c for log_n in cases.STRUCTURED for c in cases.pass_plan(log_n)[2]} == {2, 8, 9, 6, 5}
    # the first size with two lazy stores in a row is in every DIF list
    assert 21 in cases.NTT_DENSE and 21 in cases.STRUCTURED and len(cases.pass_plan(21)[2]) == 2
    assert cases.V_VALUES == (2**232 - 1, 2**251 - 1, cases.P - 1)


def test_builders():
    n = 1 << 12
    a, b = cases.random_column(n, 7), cases.random_column(n, 7)
    assert a.shape == (n, 4) and a.dtype == np.uint64 and a.flags.c_contiguous and np.array_equal(a, b)
    assert not np.array_equal(a, cases.random_column(n, 8))
    vals = cases.ints_from_felts(a)
    assert all(0 <= v < cases.P for v in vals) and len(set(vals)) == n
    assert sum(v >> 250 for v in vals) > n // 8            # the top bits are drawn too, not only 2^250 and below
    assert cases.felts_from_ints(vals).tolist() == a.tolist()
    edge = cases.felts_from_ints([cases.P - 1, cases.P, cases.P + 1, 2**251, 2**252 - 1, 0, 17 << 192])
    assert cases.is_canonical(edge).tolist() == [True, False, False, True, False, True, True]
    ext = set(wl.extreme_felts())
    e = cases.ints_from_felts(cases.extreme_column(n, 9))
    share = sum(v in ext for v in e) / n
    assert 0.80 < share < 0.90 and all(0 <= v < cases.P for v in e)
    assert len(ext & set(e)) > 0.9 * len(ext)              # the whole list is drawn from, not a corner of it
    assert np.array_equal(cases.extreme_column(n, 9), cases.extreme_column(n, 9))
    for v in cases.V_VALUES:
        cols = cases.structured_columns(5, v)
        assert cols.shape == (6, 32, 4) and cols.dtype == np.uint64
        assert cases.ints_from_felts(cols[0]) == [v] * 32
        for k in range(5):
            assert cases.ints_from_felts(cols[1 + k]) == [v if (i >> k) & 1 else 0 for i in range(32)]
