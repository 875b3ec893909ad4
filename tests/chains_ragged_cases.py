"""Inputs and expected values of the ragged-chain tests (tests/test_gpu_chains_ragged.py): seeded chains of
unequal length, their fold through the C oracle, and the per-chain status case.  Run as a program it is the child
process of the fallback test: it checks one batch and the status case in a fresh interpreter, under whatever
STARKPERP_* switches the parent put into the environment, and exits non-zero on a mismatch."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "stark-perpetual_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

P = 2**251 + 17 * 2**192 + 1
HASH_OUT_OF_RANGE = 1


def random_chains(lengths, seed):
    rng = random.Random(seed)
    return [[rng.randrange(P) for _ in range(k)] for k in lengths]


def random_lengths(n, longest, seed):
    rng = random.Random(seed)
    return [rng.randint(1, longest) for _ in range(n)]


def oracle_fold(chains):
    """Left fold of every chain through the C oracle, step by step: step j is one oracle batch over the chains
    that have a word j.  Words >= p are the caller's business (the oracle would flag them)."""
    from oracle import cref
    acc = [c[0] for c in chains]
    for j in range(1, max(len(c) for c in chains)):
        idx = [i for i, c in enumerate(chains) if len(c) > j]
        got, st = cref.pedersen_hash_many([acc[i] for i in idx], [chains[i][j] for i in idx])
        assert not any(st)
        for i, v in zip(idx, got):
            acc[i] = v
    return acc


def csr(chains):
    """(words uint64[total, 4], offsets uint32[n + 1]) of a list of chains."""
    import numpy as np
    from starkperp import batch_np
    flat = [w for c in chains for w in c]
    off = np.zeros(len(chains) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c in chains])
    return batch_np.felts_from_ints(flat), off


def status_case():
    """16 chains of 1 .. 6 words; the middle word of chain 5 (5 words) is p itself.
    Returns (chains, expected hashes with None for chain 5)."""
    lengths = [3, 1, 6, 2, 4, 5, 2, 6, 3, 1, 4, 2, 5, 3, 6, 2]
    chains = random_chains(lengths, seed=77)
    good = oracle_fold(chains)
    chains[5][2] = P
    good[5] = None
    return chains, good


def check_status_case(batch_np):
    chains, good = status_case()
    out, st = batch_np.pedersen_chains_ragged(*csr(chains))
    got = batch_np.ints_from_felts(out)
    assert [i for i in range(16) if st[i] & HASH_OUT_OF_RANGE] == [5], list(st)
    assert [int(v) for i, v in enumerate(st) if i != 5] == [0] * 15, list(st)
    assert [g for g, e in zip(got, good) if e is not None] == [e for e in good if e is not None]
    # a chain of one word is that word, and p in it is flagged like any other word
    lone = [[P], [1, 2, 3], [P - 1]]
    out, st = batch_np.pedersen_chains_ragged(*csr(lone))
    got = batch_np.ints_from_felts(out)
    assert list(st) == [HASH_OUT_OF_RANGE, 0, 0], list(st)
    assert got[0] == P and got[2] == P - 1 and got[1] == oracle_fold([lone[1]])[0]


def main():
    from starkperp import batch, batch_np
    chains = random_chains(random_lengths(300, 9, seed=300), seed=301)
    assert batch.pedersen_chains_ragged(chains) == oracle_fold(chains)
    check_status_case(batch_np)
    print("chains_ragged child ok")


if __name__ == "__main__":
    main()
