"""tests/window_width_cases.py without a GPU, for all 24 widths sp_init accepts: the plans and their window counts, every
crafted pair really carrying its claimed raw value in its claimed window (re-extracted with plain shifts), the cap on
dropped patterns and which windows they hit, the widths without a straddling window, and samples of the expected values
against the Python oracle."""
import random

import pytest

import ec_point_cases as E
import window_width_cases as W
from oracle import ref_py as R

P, N = W.P, W.N
# context.hip make_plan / init_locked, worked out by hand: widths 4 .. 27
PED_NWIN = (101, 84, 72, 63, 56, 51, 46, 42, 39, 36, 34, 32, 30, 28, 27, 26, 24, 23, 22, 21, 21, 20, 19, 18)
GEN_NWIN = (63, 51, 42, 36, 32, 28, 26, 23, 21, 20, 18, 17, 16, 15, 14, 14, 13, 12, 12, 12, 12, 12, 12, 12)
NO_STRADDLER = {5, 6, 8, 11, 13, 17, 20, 27}


def test_widths():
    assert list(W.WIDTHS) == list(range(4, 28)) and len(PED_NWIN) == len(GEN_NWIN) == 24
    assert P == R.FIELD_PRIME and N == R.EC_ORDER


@pytest.mark.parametrize("width", W.WIDTHS)
def test_plans(width):
    plan = W.plan(width)
    assert len(plan) == PED_NWIN[width - 4]
    assert plan[0][0] == 0 and 1 <= plan[0][1] <= width + 1
    assert all(nb == width + 1 for _, nb in plan[1:])
    assert all(plan[i][0] + plan[i][1] == plan[i + 1][0] for i in range(len(plan) - 1))
    assert plan[-1][0] + plan[-1][1] == W.BITS == sum(nb for _, nb in plan)
    assert (plan[0][1] == width + 1) == (504 % (width + 1) == 0)
    wbits, nwin = W.gen_plan(width)
    assert wbits == min(width, 22) and nwin == GEN_NWIN[width - 4]
    wins = W.gen_windows(wbits)
    assert len(wins) == nwin and sum(nb for _, nb in wins) == 252
    assert (wins[-1][1] == wbits) == (252 % wbits == 0)
    # the kernels' thresholds the issue reads off these counts
    assert (len(plan) > 64) == (width <= 6)
    assert (len(plan) >= 33) == (width <= 14)


def test_plan_is_the_cpu_models():
    import test_window_plan_cpu as T
    for width in W.WIDTHS:
        assert W.plan(width) == T.make_plan(width)


def test_widths_without_a_straddling_window():
    assert {w for w in W.WIDTHS if W.straddler(w) is None} == NO_STRADDLER
    assert NO_STRADDLER == {w for w in W.WIDTHS if 252 % (w + 1) == 0}
    for w in W.WIDTHS:
        g = W.straddler(w)
        if g is not None:
            s0, nb = W.plan(w)[g]
            assert s0 < 252 < s0 + nb and g == W.window_of_bit(w, 251) == W.window_of_bit(w, 252)
        else:
            assert W.window_of_bit(w, 251) + 1 == W.window_of_bit(w, 252)


@pytest.mark.parametrize("width", W.WIDTHS)
def test_crafted_pairs_carry_what_they_claim(width):
    records, dropped = W.crafted(width)
    plan = W.plan(width)
    assert len(records) <= 4 * 101 + 20
    carried = set()
    for x, y, g, raw, label in records:
        assert 0 <= x < P and 0 <= y < P, label
        if g is not None:
            s0, nb = plan[g]
            assert W.raw_window(x, y, s0, nb) == raw, label
            carried.add((g, raw))
    # every extreme of every window is there or is listed as dropped, and nothing is both
    wanted = {(g, raw) for g in range(len(plan)) for raw, _ in W.patterns(width, g)}
    gone = {(g, raw) for g, raw, _ in dropped}
    assert wanted <= carried | gone and not (carried & gone)
    log2e = width
    for g in range(1, len(plan)):
        raws = [raw for raw, _ in W.patterns(width, g)]
        assert raws == [0, 2**log2e - 1, 2**log2e, 2 ** (log2e + 1) - 1]
    w0 = plan[0][1]
    assert {raw for raw, _ in W.patterns(width, 0)} == {0, 1, 2**w0 - 1, 2 ** (w0 - 1)}
    # the extras
    pairs = set(W.crafted_pairs(width))
    assert {(a, b) for a in W.PC.NEAR_MISSES for b in W.PC.NEAR_MISSES} <= pairs
    assert (0, 0) in pairs and (P - 1, P - 1) in pairs
    g = W.straddler(width)
    if g is not None:
        labels = [r[4] for r in records if r[4].startswith("straddling")]
        assert any("all zeros" in s for s in labels) and any("p - 1" in s for s in labels)
        assert any("all ones" in s for s in labels) == (plan[g][0] == 251)


@pytest.mark.parametrize("width", W.WIDTHS)
def test_drop_cap_and_the_windows_it_hits(width):
    """A pattern is dropped only when the smallest operand that carries it is not below p - checked here from scratch -
    and only windows that hold string bit 251 or 503 have such patterns; at most DROP_CAP per width."""
    _, dropped = W.crafted(width)
    plan = W.plan(width)
    assert len(dropped) <= W.DROP_CAP == 4
    allowed = {W.window_of_bit(width, 251), W.window_of_bit(width, 503)}
    assert {g for g, _, _ in dropped} <= allowed
    assert W.window_of_bit(width, 503) == len(plan) - 1
    for g, raw, label in dropped:
        s0, nb = plan[g]
        smallest = raw << s0
        assert (smallest & W.MASK252) >= P or (smallest >> 252) >= P, label
    # the top window's positive half needs y >= 2^251: "index 0" is y = 2^251 + ..., kept; "index all ones" is dropped
    top = len(plan) - 1
    kept = {(g, raw) for _, _, g, raw, _ in W.crafted(width)[0]}
    assert (top, 1 << width) in kept and (top, 0) in kept and (top, (1 << width) - 1) in kept
    assert (top, (2 << width) - 1) in {(g, raw) for g, raw, _ in dropped}


@pytest.mark.parametrize("width", W.WIDTHS)
def test_crafted_expected_on_a_sample(width):
    pairs, want = W.crafted_pairs(width), W.crafted_expected(width)
    assert len(pairs) == len(want)
    for i in random.Random(width).sample(range(len(pairs)), 8):
        assert want[i] == R.pedersen_hash(*pairs[i]), (width, i)


def test_tiled_holds_every_crafted_pair_once():
    import numpy as np
    for width, n in ((4, 1500), (27, 3000), (9, 100)):
        x, y, expected = W.tiled(width, n)
        cx, cy, ch = W.crafted_arrays(width)
        tx, ty, th = W.PC.table()
        rows = {(a.tobytes(), b.tobytes()): c.tobytes() for a, b, c in zip(tx, ty, th)}
        rows.update({(a.tobytes(), b.tobytes()): c.tobytes() for a, b, c in zip(cx, cy, ch)})
        assert all(rows[(a.tobytes(), b.tobytes())] == c.tobytes() for a, b, c in zip(x, y, expected))
        have = {(a.tobytes(), b.tobytes()) for a, b in zip(x, y)}
        crafted = [(a.tobytes(), b.tobytes()) for a, b in zip(cx, cy)]
        assert sum(1 for c in crafted if c in have) >= min(n, len(crafted)) - 12  # table rows repeat the near misses
        again = W.tiled(width, n)
        assert all((a == b).all() for a, b in zip(again, (x, y, expected)))
        assert x.shape == y.shape == expected.shape == (n, 4) and x.dtype == np.uint64


@pytest.mark.parametrize("wbits", range(4, 23))
def test_generator_scalars(wbits):
    ks = W.gen_scalars(wbits)
    assert len(set(ks)) == len(ks) and all(0 < k < N for k in ks)
    have = set(ks)
    full = 2**252 - 1
    for first, nb in W.gen_windows(wbits):
        ones = (2**nb - 1) << first
        assert {ones % N, (full ^ ones) % N, 1 << first} - {0} <= have
    assert {1, N - 1, 2**251, 2**251 - 1} <= have and set(E.edge_scalars()) - {0} <= have
    first, nb = W.gen_windows(wbits)[-1]
    top = max(k >> first for k in ks)
    assert top == (N - 1) >> first and top < 2**nb and (top << first) in have
    for k in random.Random(wbits).sample(ks, 3):
        assert E.gmul(k) == tuple(R.ec_mult(k, tuple(R.EC_GEN))), hex(k)


@pytest.mark.parametrize("wbits", (4, 13, 22))
def test_signer_and_verifier_items(wbits):
    import sign_cases as SC
    items = W.sign_items(wbits)
    kinds = [SC.attempt_kind(*it)[3] for it in items]
    assert kinds.count("ok") >= len(W.gen_scalars(wbits)) // 3
    assert kinds.count("retry_t") >= 4 and kinds.count("retry_w") >= 4 and kinds.count("bad_input") == 2
    z, d, k = items[kinds.index("ok")]
    _, r, s = SC.attempt(z, d, k)
    assert r == R.ec_mult(k, tuple(R.EC_GEN))[0] and R.verify(z, r, s, tuple(R.ec_mult(d, tuple(R.EC_GEN))))
    sigs, q = W.verify_items(wbits)
    u1 = {z * pow(s, -1, N) % N for z, _, s in sigs}
    assert u1 == set(W.gen_scalars(wbits))
    for j in random.Random(wbits).sample(range(len(sigs)), 4):
        z, r, s = sigs[j]
        twin = j > 0 and sigs[j - 1][0] == z and sigs[j - 1][1] == r - 1  # the valid signature with r + 1
        assert R.verify(z, r, s, q) == (not twin), (wbits, j)


def test_sparse_history_shapes():
    """The batches of the height-64 history put 1 .. 2048, 2049 .. 4096 and 4097 .. 8192 hashes on a level, and hold
    overwrites and resets."""
    for empty in (0, 12345):
        history = W.sparse_history(64, empty)
        assert [len(m) for m in history] == list(W.SPARSE_BATCHES)
        widths = set()
        for mods in history:
            for level in range(1, 65):
                widths.add(len({k >> level for k in mods}))
        assert any(w <= 2048 for w in widths) and any(2048 < w <= 4096 for w in widths) and any(4096 < w <= 8192 for w in widths)
        for a, b in zip(history, history[1:]):
            if len(a) >= 8:
                assert set(a) & set(b) and any(b[k] == empty for k in set(a) & set(b))
    small = W.sparse_history(3, 0, sizes=(1, 3, 8, 5))
    assert [len(m) for m in small] == [1, 3, 8, 5]


# ---- would the crafted cases notice a one-bit error?  The kernels' extraction restated, and mutants of it ---------------
def field_from_memory(felt, bit, width):
    """pedersen.hip field_from_memory on a 256-bit operand: two 32-bit words, shifted, truncated to 32 bits, masked."""
    words = [(felt >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    wi, sh = bit >> 5, bit & 31
    two = words[wi] | ((words[wi + 1] << 32) if wi + 1 < 8 else 0)
    return ((two >> sh) & 0xFFFFFFFF) & ((1 << width) - 1)


def window_from_memory(x, y, start, width, mutant=None):
    """pedersen.hip window_from_memory; `mutant` names a one-bit error in its straddling case."""
    if start + width <= 252:
        return field_from_memory(x, start, width)
    if start >= 252:
        return field_from_memory(y, start - 252, width)
    lo_n = 252 - start - (1 if mutant == "lo_n one short" else 0)
    hi_n = width - lo_n - (1 if mutant == "y part one bit short" else 0)
    hi_bit = 1 if mutant == "y part from bit 1" else 0
    shift = lo_n + {"shift one more": 1, "shift one less": -1}.get(mutant, 0)
    return field_from_memory(x, start, lo_n) | (field_from_memory(y, hi_bit, hi_n) << shift)


STRADDLE_MUTANTS = ("lo_n one short", "y part one bit short", "y part from bit 1", "shift one more", "shift one less")


@pytest.mark.parametrize("width", W.WIDTHS)
def test_crafted_pairs_tell_a_one_bit_error_in_the_straddling_case(width):
    """The restated extraction gives every window of every crafted pair; each mutant of the straddling case gives a wrong
    raw value - another table entry or another sign, so another hash - on at least one crafted pair of every width that has
    a straddling window: tests/test_gpu_window_widths.py::test_crafted_pairs_alone_and_as_points and ::test_tiled_batches
    fail there."""
    plan = W.plan(width)
    pairs = W.crafted_pairs(width)
    for x, y in pairs:
        for s0, nb in plan:
            assert window_from_memory(x, y, s0, nb) == W.raw_window(x, y, s0, nb)
    g = W.straddler(width)
    if g is None:
        return
    s0, nb = plan[g]
    for mutant in STRADDLE_MUTANTS:
        assert any(window_from_memory(x, y, s0, nb, mutant) != W.raw_window(x, y, s0, nb) for x, y in pairs), mutant


def gen_windows_popped(k, wbits, nwin, right=0, left=0):
    """gen_mul.hpp gen_mul_gathered's pop on eight 32-bit words: the window values in order; right / left = an error of
    that many bits in the shift of a word, resp. of its neighbour's carried-in bits."""
    words = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    out = []
    for _ in range(nwin):
        out.append(words[0] & ((1 << wbits) - 1))
        for i in range(7):
            words[i] = ((words[i] >> (wbits + right)) | (words[i + 1] << (32 - wbits + left))) & 0xFFFFFFFF
        words[7] >>= wbits + right
    return out


@pytest.mark.parametrize("wbits", range(4, 23))
def test_generator_scalars_tell_a_one_bit_error_in_the_shift(wbits):
    """The restated pop gives the windows of every generator scalar; with a shift that is one bit off on either side some
    scalar selects another table entry: the four generator-walk tests of tests/test_gpu_window_widths.py fail at that
    width."""
    nwin = W.gen_plan(wbits)[1]
    ks = W.gen_scalars(wbits)
    want = {k: [(k >> (wbits * i)) & (2**wbits - 1) for i in range(nwin)] for k in ks}
    assert all(gen_windows_popped(k, wbits, nwin) == want[k] for k in ks)
    for right, left in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert any(gen_windows_popped(k, wbits, nwin, right, left) != want[k] for k in ks), (right, left)
