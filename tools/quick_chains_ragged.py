#!/usr/bin/env python3
"""Message hashes of a mixed transaction batch, host-inclusive, three ways in one process (through starkperp.batch_np:
no Python-int packing in the timing): 4096 items - 70 % limit orders and 20 % transfers (5 words), 5 % conditional
transfers (6 words), 5 % withdrawals to an address (3 words), interleaved - plus 32 oracle prices (2 words).
  (a) one sp_pedersen_chains_ragged call (ped_fold_ragged_kernel, chain form);
  (b) the way before it: one pedersen_chains call per length class plus pedersen_hash_many for the 2-word items;
  (c) the floor: pedersen_chains on 4128 chains that all have the deepest length (6).
Median of the calls after a warm-up; prints a / b and a / c.
    python tools/quick_chains_ragged.py [calls=30] [output file]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-perpetual_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from starkperp import _lib, batch_np  # noqa: E402
from evidence_stamp import lib_hash  # noqa: E402

CALLS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
COUNTS = ((5, 2867 + 819), (6, 205), (3, 205), (2, 32))  # (words, chains): 4096 items + 32 prices


def felts(rng, n):
    a = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(6)  # below 2^249 < p
    return a


def median_ms(fn):
    for _ in range(5):
        fn()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    rng = np.random.default_rng(7)
    lengths = np.concatenate([np.full(n, k, dtype=np.uint32) for k, n in COUNTS])
    rng.shuffle(lengths)  # the batch interleaves its transaction types
    n = lengths.shape[0]
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lengths)
    words = felts(rng, int(off[-1]))
    # the same chains grouped by length, word-major, for the equal-depth calls
    groups = {}
    for k, _ in COUNTS:
        idx = np.flatnonzero(lengths == k)
        rows = off[idx][None, :] + np.arange(k, dtype=np.uint32)[:, None]  # [k, n_k] row numbers
        groups[k] = (idx, np.ascontiguousarray(words[rows]))
    deepest = felts(rng, 6 * n).reshape(6, n, 4)

    def by_class():
        out = np.empty((n, 4), dtype=np.uint64)
        for k, (idx, w) in groups.items():
            out[idx] = batch_np.pedersen_hash_many(w[0], w[1]) if k == 2 else batch_np.pedersen_chains(w)
        return out

    _lib.ensure_init()
    got, st = batch_np.pedersen_chains_ragged(words, off)
    assert not st.any() and (got == by_class()).all(), "the ragged call and the per-class calls disagree"
    a = median_ms(lambda: batch_np.pedersen_chains_ragged(words, off))
    b = median_ms(by_class)
    c = median_ms(lambda: batch_np.pedersen_chains(deepest))
    lines = [
        "tools/quick_chains_ragged.py: %d chains (%s), %d hashes, median of %d host-inclusive calls, window bits %d"
        % (n, ", ".join("%d x %d words" % (m, k) for k, m in COUNTS), int(off[-1]) - n, CALLS,
           _lib.load().sp_window_bits()),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "(a) one ragged call                          %8.3f ms" % a,
        "(b) one call per length class, summed        %8.3f ms" % b,
        "(c) %d chains, all of the deepest length 6 %8.3f ms" % (n, c),
        "a / b = %.3f    a / c = %.3f" % (a / b, a / c),
    ]
    if a >= b:
        lines.append("NOTE: the single call is NOT faster than the per-class calls on this run")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
