"""Cases of sp_builtins_eval_points_dev - the composition value of a prove_builtins proof at opened points - shared
by tests/test_builtins_verify_cpu.py (the g++ shim of csrc/verify_builtins.hpp, no GPU) and
tests/test_gpu_builtins_verify.py.  Seeded; the expectation per point is the oracle's own arithmetic, as
verify_builtins_proof does it (oracle/stark_ref.py, the loop over `layout` under "composition value"):
rc16_constraint_values + rc16_composition_value for rc16, AIRS[air]["constraints"] times 1 / Z_H for the other two,
summed mod p.  Neither torch nor the library is imported.

Sizes: all 7 segment sets, each at the smallest log_n its segments admit (rc16 alone: 3, so M = 32 and the rc16
periodic table is exactly M rows; any set with ecdsa: 10).
Oracle time on one CPU core: the periodic tables 1.3 s (cached per segment and n), the 7 x 257 expected values 0.5 s."""
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "stark-perpetual_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import stark_ref as S  # noqa: E402
from verify_cases import EXTREMES, NOT_FELTS, felts_np, ints_of  # noqa: E402,F401

P = S.P
SHIFT = S.GEN
SEG_NAMES = ("pedersen", "ecdsa", "rc16")  # the column order of a combined trace
SEG_BITS = {"pedersen": 1, "ecdsa": 2, "rc16": 4}
SEG_MIN_LOG_N = {"pedersen": 9, "ecdsa": 10, "rc16": 3}
SEGMENT_SETS = tuple(tuple(s for s in SEG_NAMES if mask & SEG_BITS[s]) for mask in range(1, 8))
ITEM_COUNTS = (1, 63, 64, 65, 257)
POINT_OK, POINT_OUT_OF_RANGE = 0, 1
RC_MIN, RC_MAX = 3, 40000


def mask_of(segments):
    return sum(SEG_BITS[s] for s in segments)


def min_log_n(segments):
    return max(SEG_MIN_LOG_N[s] for s in segments)


def max_log_n(segments):
    return 24 if "rc16" in segments else 30


@functools.lru_cache(maxsize=None)
def periodic_tables(seg, n):
    """The segment's periodic columns on the LDE coset, as verify_builtins_proof builds them."""
    if seg == "rc16":
        return [S.lde(c, S.BLOWUP, pow(SHIFT, n // 8, P)) for c in S.rc16_periodic_columns()]
    return S.periodic_lde(n, SHIFT, seg)


def edge_positions(M):
    """The first rows, the rows whose next row wraps, both sides of the middle of the domain, pos = 31 and 0 mod 32
    (the ends of the rc16 periodic table) away from the ends of the domain."""
    return [0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1, M // 2 - 1, M // 2, 31 % M, 32 % M, (M // 2 + 31) % M,
            (M // 2 + 32) % M]


class BuiltinsCase:
    """One segment set at its smallest size: dense columns [n_cols][M] and a phase-2 column [M] of seeded felts
    with rows of EXTREMES, the periodic tables, alphas, z, 257 points and the integer expectation at each.  The
    points are all M positions where M <= 257 (then repeated, each repeat with the same rows), else the edges and
    seeded positions."""

    def __init__(self, segments):
        rng = random.Random("builtins-points-" + "+".join(segments))
        self.segments = tuple(segments)
        self.mask = mask_of(segments)
        self.log_n = min_log_n(segments)
        self.n = n = 1 << self.log_n
        self.M = M = 4 * n
        self.layout = S.builtin_layout(list(segments))
        self.n_cols = sum(c for _, _, c, _, _ in self.layout)
        self.n_alpha = sum(a for *_, a in self.layout)
        self.has_rc = "rc16" in segments
        self.alphas = [rng.randrange(1, P) for _ in range(self.n_alpha)]
        self.z = rng.randrange(1, P)
        self.rc_min, self.rc_max = RC_MIN, RC_MAX
        self.cols = [[rng.randrange(P) for _ in range(M)] for _ in range(self.n_cols)]
        self.pcol = [rng.randrange(P) for _ in range(M)]
        total = ITEM_COUNTS[-1]
        if M <= total:
            self.positions = [i % M for i in range(total)]
            fill = list(range(4, M - 8))
        else:
            edges = list(dict.fromkeys(edge_positions(M)))
            fill = [rng.randrange(M) for _ in range(total - len(edges))]
            self.positions = edges + fill
        # rows of extreme patterns, shifted per column, at some positions and their next rows
        for t, r in enumerate(fill[:2 * len(EXTREMES)]):
            for c in range(self.n_cols):
                self.cols[c][r] = EXTREMES[(c + t) % len(EXTREMES)]
                if t % 2:
                    self.cols[c][(r + 4) % M] = EXTREMES[(2 * c + t) % len(EXTREMES)]
            self.pcol[r] = EXTREMES[(t + 3) % len(EXTREMES)]
        self.pers = {seg: periodic_tables(seg, n) for seg in segments}
        self.w = S.root_of_unity(M.bit_length() - 1)
        self.g_last = pow(S.root_of_unity(n.bit_length() - 1), n - 1, P)
        self.zinv = [pow((pow(SHIFT, n, P) * pow(self.w, n * k, P) - 1) % P, -1, P) for k in range(4)]
        self.expected = [self.value_at(p) for p in self.positions]

    def rows(self, pos):
        j = (pos + 4) % self.M
        return [c[pos] for c in self.cols], [c[j] for c in self.cols], self.pcol[pos], self.pcol[j]

    def parts(self, pos, cur, nxt, pcur, pnxt):
        """The composition value of every present segment at pos, in integers."""
        x = SHIFT * pow(self.w, pos, P) % P
        out = {}
        for air, c0, nc, a0, na in self.layout:
            al = self.alphas[a0: a0 + na]
            if air == "rc16":
                pv = [tab[pos % 32] for tab in self.pers[air]]
                cv = S.rc16_constraint_values(cur[c0: c0 + nc], nxt[c0: c0 + nc], pv, pcur, pnxt, self.z, self.rc_min,
                                              self.rc_max)
                out[air] = S.rc16_composition_value(al, cv, x, self.zinv[pos % 4], self.g_last)
            else:
                spec = S.AIRS[air]
                pv = [tab[pos % (4 * spec["period"])] for tab in self.pers[air]]
                cv = spec["constraints"](cur[c0: c0 + nc], nxt[c0: c0 + nc], pv)
                out[air] = sum(a * c for a, c in zip(al, cv)) % P * self.zinv[pos % 4] % P
        return out

    def value(self, pos, cur, nxt, pcur, pnxt):
        return sum(self.parts(pos, cur, nxt, pcur, pnxt).values()) % P

    def value_at(self, pos):
        return self.value(pos, *self.rows(pos))

    def pack(self, items):
        """items [(pos, cur, nxt, pcur, pnxt)] -> (pos u64 [k], cur [k * n_cols, 4], nxt, pcur [k, 4], pnxt)"""
        return (np.array([it[0] for it in items], dtype=np.uint64), felts_np([v for it in items for v in it[1]]),
                felts_np([v for it in items for v in it[2]]), felts_np([it[3] for it in items]),
                felts_np([it[4] for it in items]))

    def arrays(self, count):
        """The first `count` points packed, and their expected ints."""
        return self.pack([(p,) + tuple(self.rows(p)) for p in self.positions[:count]]) + (self.expected[:count],)

    def per_np(self, seg):
        return felts_np([v for tab in self.pers[seg] for v in tab]) if seg in self.segments else None

    def bad_items(self):
        """Items that must come back OUT_OF_RANGE with a zero value, good neighbours between them: (pos, cur, nxt,
        pcur, pnxt, expected value or None).  pos = M and 2^64 - 1 - the periodic tables must still be read inside -,
        p itself in each of the 2 n_cols felts of the rows (and with rc16 in pcur and in pnxt) in turn, and the
        other NOT_FELTS in felts spread over the rows."""
        good = self.positions[12 % len(self.positions)]
        neighbour = lambda: (good,) + tuple(self.rows(good)) + (self.value_at(good),)
        items = [neighbour()]
        for p in (self.M, 2**64 - 1):
            items.append((p,) + tuple(self.rows(p % self.M)) + (None,))
        items.append(neighbour())
        slots = [(which, col) for which in (0, 1) for col in range(self.n_cols)] + ([(2, 0), (3, 0)] if self.has_rc else [])
        for k, (which, col) in enumerate(slots):
            cur, nxt, pcur, pnxt = self.rows(good)
            if which < 2:
                (cur, nxt)[which][col] = P
            elif which == 2:
                pcur = P
            else:
                pnxt = P
            items.append((good, cur, nxt, pcur, pnxt, None))
            if k % 5 == 4:
                items.append(neighbour())
        for k, bad in enumerate(NOT_FELTS[1:]):
            which, col = slots[(3 * k + 1) % len(slots)]
            cur, nxt, pcur, pnxt = self.rows(good)
            if which < 2:
                (cur, nxt)[which][col] = bad
            elif which == 2:
                pcur = bad
            else:
                pnxt = bad
            items.append((good, cur, nxt, pcur, pnxt, None))
        items.append(neighbour())
        return items

    def n_bad(self):
        return 2 + 2 * self.n_cols + (2 if self.has_rc else 0) + len(NOT_FELTS) - 1


@functools.lru_cache(maxsize=None)
def builtins_case(segments):
    return BuiltinsCase(tuple(segments))


# the argument rules of the call that need no pointer: (what, expected word of the refusal, overrides of the good
# call's scalars).  `segments` a mask, log_n, rc_min, rc_max, z.
def refused_scalars():
    out = [("segments 0", "segments", {"mask": 0}), ("segments 8", "segments", {"mask": 8})]
    for segs in SEGMENT_SETS:
        name = "+".join(segs)
        out.append((name + " log_n below", "log_n", {"mask": mask_of(segs), "log_n": min_log_n(segs) - 1}))
        out.append((name + " log_n above", "log_n", {"mask": mask_of(segs), "log_n": max_log_n(segs) + 1}))
    out.append(("rc_min > rc_max", "limb range", {"mask": 4, "log_n": 3, "rc_min": 5, "rc_max": 4}))
    out.append(("rc_max 65536", "limb range", {"mask": 4, "log_n": 3, "rc_min": 0, "rc_max": 65536}))
    out.append(("z = p", "z", {"mask": 4, "log_n": 3, "z": P}))
    return out
