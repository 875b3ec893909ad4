"""GPU parity of the kernels that take the product-scanning field multiplication (csrc/fp29.hpp, selected per kernel
family in csrc/pedersen.hip) against the C oracle (oracle/cref.py), never against the library itself:

  * pedersen_hash_many at n = 131 072 - two whole rounds of the one-lane bulk kernel (ped_accumulate_kernel) + finish;
  * the same at n = 65 536 + 4 097 - the mixed kernel: one bulk round beside a lane-split remainder;
  * merkle_roots_many for 40 trees of height 12 - level 0 is 81 920 hashes (bulk + remainder) and every smaller level
    runs the latency kernels (split / quad / top): the parity test of any latency family that adopts the new form.
Inputs are seeded random felts with the operands 0, 1, p - 1 and 2^251 in the first 64 lanes (all 16 pairs, four
times over).  The whole batch is checked with the oracle's windowed comparator, the first 2 048 also with its
252-step affine loop."""
import json
import os
import random

import pytest

from oracle import cref
from oracle import ref_py as R

pytestmark = pytest.mark.gpu

P = R.FIELD_PRIME
EDGE = (0, 1, P - 1, 2**251)


@pytest.fixture(scope="module")
def batch():
    from starkperp import batch as b
    return b


def operands(n, seed):
    rng = random.Random(seed)
    xs = [rng.randrange(P) for _ in range(n)]
    ys = [rng.randrange(P) for _ in range(n)]
    for lane in range(64):
        xs[lane], ys[lane] = EDGE[(lane >> 2) & 3], EDGE[lane & 3]
    return xs, ys


@pytest.mark.parametrize("n", [131072, 65536 + 4097], ids=["two_bulk_rounds", "bulk_plus_remainder"])
def test_hash_batch_vs_c_oracle(batch, n):
    xs, ys = operands(n, seed=2950 + n % 7)
    exp, st = cref.opt_pedersen_hash_many(xs, ys)
    assert not any(st)
    slow, st_slow = cref.pedersen_hash_many(xs[:2048], ys[:2048])
    assert not any(st_slow) and slow == exp[:2048]
    got = batch.pedersen_hash_many(xs, ys)
    assert got[:2048] == slow
    assert got == exp


FOREST_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_scan_forest_roots.json")


def forest_trees():
    rng = random.Random(2960)
    trees = [[rng.randrange(P) for _ in range(1 << 12)] for _ in range(40)]
    for lane in range(64):  # the same edge operand pairs as sibling leaves of the first tree
        trees[0][2 * lane], trees[0][2 * lane + 1] = EDGE[(lane >> 2) & 3], EDGE[lane & 3]
    return trees


def test_forest_of_40_trees_of_height_12_vs_c_oracle(batch):
    """The expected roots are cref.merkle_levels on every tree.  That is 163 800 hashes by the 252-step affine loop,
    over a minute of CPU time, so they are RECORDED (tests/golden/field_scan_forest_roots.json, written by running this
    file as a script) and the test re-derives them live as far as a few seconds allow: cref.merkle_levels on the first
    tree (the one with the edge operands) and the oracle's windowed comparator on all 40."""
    trees = forest_trees()
    gold = json.load(open(FOREST_GOLD))
    assert gold["trees"] == 40 and gold["height"] == 12 and gold["seed"] == 2960
    exp = [int(v, 16) for v in gold["roots_by_cref_merkle_levels"]]
    assert cref.merkle_levels(trees[0])[-1][0] == exp[0]
    assert [cref.opt_merkle_levels(t)[-1][0] for t in trees] == exp
    assert batch.merkle_roots_many(trees) == exp


if __name__ == "__main__":
    roots = [cref.merkle_levels(t)[-1][0] for t in forest_trees()]
    json.dump({"trees": 40, "height": 12, "seed": 2960, "roots_by_cref_merkle_levels": [hex(r) for r in roots]},
              open(FOREST_GOLD, "w"), indent=1)
