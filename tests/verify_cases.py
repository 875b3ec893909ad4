"""Cases of the verifier's two device calls (sp_air_eval_points_dev, sp_fri_check_queries_dev), shared by
tests/test_verify_cpu.py (the g++ shim of csrc/verify.hpp, no GPU) and tests/test_gpu_verify.py.  Seeded; the
expectations are Python integers on oracle/stark_ref.py: AIRS[air]["constraints"] for the composition values and the
fold formula of verify_proof (lines "FRI consistency") for the fold statuses.  Neither torch nor the library is imported.

Sizes: the smallest trace each AIR admits (n = its period), so M = 4 n LDE rows.
Oracle time on one CPU core: the four periodic tables 0.7 s (ecdsa 0.5), the four dense columns and their 257 expected
values 0.3 s, the three fold chains 0.1 s."""
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

P = S.P
SHIFT = S.GEN
AIR_IDS = {"pedersen": 0, "ec_ladder": 1, "ecdsa": 2, "range_check": 3}
AIR_N = {"range_check": 128, "ec_ladder": 256, "pedersen": 512, "ecdsa": 1024}
MIN_LOG_N = {"range_check": 7, "ec_ladder": 8, "pedersen": 9, "ecdsa": 10}
ITEM_COUNTS = (1, 63, 64, 65, 257)
POINT_OK, POINT_OUT_OF_RANGE = 0, 1
FOLD_OK, FOLD_MISMATCH, FOLD_OUT_OF_RANGE = 0, 1, 2
# 0, 1, p - 1, bit 251 alone, limbs aligned to 2^192 (the top 64-bit word alone, full; the words below it, full),
# every 29-bit limb full below bit 232
EXTREMES = (0, 1, P - 1, 2**251, ((1 << 59) - 1) << 192, (1 << 192) - 1, (1 << 232) - 1)
NOT_FELTS = (P, P + 1, 2**256 - 1, 2**255)


def felts_np(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).copy()


def ints_of(arr):
    raw = np.ascontiguousarray(arr).astype("<u8").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]


# ---- composition points -----------------------------------------------------------------------------------------------
def edge_positions(air):
    """The positions every AIR's case must hold: the first rows, the rows whose next row wraps, both sides of the
    periodic table's end and of the middle of the domain."""
    M, per_len = 4 * AIR_N[air], 4 * S.AIRS[air]["period"]
    return [0, 1, 2, 3, M - 4, M - 3, M - 2, M - 1, per_len - 1, per_len % M, M // 2 - 1, M // 2]


class AirCase:
    """One AIR at its smallest size: dense columns [n_cols][M] of seeded felts with rows of EXTREMES, the periodic
    tables, alphas, 257 positions (the edges first) and the integer expectation at each."""

    def __init__(self, air):
        rng = random.Random("verify-points-" + air)
        spec = S.AIRS[air]
        self.air, self.n = air, AIR_N[air]
        self.M = M = 4 * self.n
        self.n_cols = spec["n_cols"]
        self.alphas = [rng.randrange(1, P) for _ in range(spec["n_constraints"])]
        self.cols = [[rng.randrange(P) for _ in range(M)] for _ in range(self.n_cols)]
        edges = edge_positions(air)
        fill = [rng.randrange(M) for _ in range(ITEM_COUNTS[-1] - len(edges))]
        self.positions = edges + fill
        # rows of extreme patterns, shifted per column, at some filler positions and their next rows
        for t, r in enumerate(fill[:2 * len(EXTREMES)]):
            for c in range(self.n_cols):
                self.cols[c][r] = EXTREMES[(c + t) % len(EXTREMES)]
                if t % 2:
                    self.cols[c][(r + 4) % M] = EXTREMES[(2 * c + t) % len(EXTREMES)]
        self.per = S.periodic_lde(self.n, SHIFT, air)
        w = S.root_of_unity(M.bit_length() - 1)
        self.zinv = [pow((pow(SHIFT, self.n, P) * pow(w, self.n * k, P) - 1) % P, -1, P) for k in range(4)]
        self.expected = [self.value_at(p) for p in self.positions]

    def rows(self, pos):
        return [c[pos] for c in self.cols], [c[(pos + 4) % self.M] for c in self.cols]

    def value(self, pos, cur, nxt):
        spec = S.AIRS[self.air]
        pv = [tab[pos % (4 * spec["period"])] for tab in self.per]
        cv = spec["constraints"](cur, nxt, pv)
        return sum(a * c for a, c in zip(self.alphas, cv)) % P * self.zinv[pos % 4] % P

    def value_at(self, pos):
        return self.value(pos, *self.rows(pos))

    def arrays(self, count):
        """(pos u64 [count], cur [count * n_cols, 4], nxt likewise, expected ints) of the first `count` positions."""
        pos = self.positions[:count]
        cur, nxt = [], []
        for p in pos:
            c, n = self.rows(p)
            cur += c
            nxt += n
        return np.array(pos, dtype=np.uint64), felts_np(cur), felts_np(nxt), self.expected[:count]

    def per_np(self):
        return felts_np([v for tab in self.per for v in tab])

    def bad_items(self):
        """Items that must come back OUT_OF_RANGE with a zero value beside good ones: (pos, cur, nxt, expected
        value or None).  Positions at and far above M - the periodic table must still be read inside - and a felt
        >= p in every column of cur and of nxt in turn."""
        items = []
        good = self.positions[12]
        for p in (good, self.M, self.M + 5, 2**32 + 1, 2**64 - 1):
            c, n = self.rows(p % self.M)
            items.append((p, c, n, self.value(p, c, n) if p < self.M else None))
        k = 0
        for which in (0, 1):
            for col in range(self.n_cols):
                c, n = self.rows(good)
                (c, n)[which][col] = NOT_FELTS[k % len(NOT_FELTS)]
                k += 1
                items.append((good, c, n, None))
        items.append((good,) + self.rows(good) + (self.value_at(good),))
        return items


@functools.lru_cache(maxsize=None)
def air_case(air):
    return AirCase(air)


# ---- fold chains ------------------------------------------------------------------------------------------------------
FRI_SHAPES = ((7, 1), (9, 3), (12, 6))  # (log_m, n_layers)


def fold_value(a, b, beta, x):
    return ((a + b) * pow(2, -1, P) + beta * (a - b) % P * pow(2 * x, -1, P)) % P


def fold_x(log_m, k, jk):
    return pow(SHIFT, 1 << k, P) * pow(S.root_of_unity(log_m - k), jk, P) % P


def fold_statuses(log_m, n_layers, betas, index, pairs, final):
    """The statuses of sp_fri_check_queries_dev in integers: verify_proof's fold loop per (q, k), with the range
    rules of the call in front."""
    out = []
    for j, layers in zip(index, pairs):
        row = []
        for k in range(n_layers):
            if j >= 1 << (log_m - 1):
                row.append(FOLD_OUT_OF_RANGE)
                continue
            mk = 1 << (log_m - k)
            jk = j % (mk // 2)
            a, b = layers[k]
            target = layers[k + 1][0 if jk < mk // 4 else 1] if k + 1 < n_layers else final[jk]
            if a >= P or b >= P or target >= P:
                row.append(FOLD_OUT_OF_RANGE)
            else:
                row.append(FOLD_OK if fold_value(a, b, betas[k], fold_x(log_m, k, jk)) == target else FOLD_MISMATCH)
        out.append(row)
    return out


class FriCase:
    """Layers folded by the oracle from a seeded layer 0, honest queries at the index edges, then mutated copies.
    `notes[q]` says what query q is; `single[q] = k` where exactly status (q, k) of the query must be MISMATCH."""

    def __init__(self, log_m, n_layers):
        rng = random.Random("verify-fri-%d-%d" % (log_m, n_layers))
        self.log_m, self.n_layers = log_m, n_layers
        m = 1 << log_m
        self.betas = [rng.randrange(1, P) for _ in range(n_layers)]
        self.layers = [[rng.randrange(P) for _ in range(m)]]
        s = SHIFT
        for k in range(n_layers):
            self.layers.append(S.fri_fold(self.layers[-1], self.betas[k], s))
            s = s * s % P
        self.final = list(self.layers[-1])
        n_final = len(self.final)
        self.index, self.pairs, self.notes, self.single = [], [], [], {}
        edges = [0, m // 2 - 1]
        for k in range(n_layers):  # both sides of a quarter of layer k
            mk = m >> k
            edges += [mk // 4 - 1, mk // 4]
            if mk // 4 + mk // 2 < m // 2:
                edges += [mk // 4 + mk // 2 - 1, mk // 4 + mk // 2]
        edges = [j for j in dict.fromkeys(edges) if 0 <= j < m // 2]
        # the final-layer slots 1 and 2 are kept for the two queries that change the shared final layer
        honest = [j for j in edges if j % n_final not in (1, 2)] + [j for j in (rng.randrange(m // 2) for _ in range(40))
                                                                   if j % n_final not in (1, 2)][:12]
        for j in honest:
            self.add(j, self.open(j), "honest")
        j0 = next(j for j in range(3, m // 2) if j % n_final not in (1, 2))
        # a == b, followed through: the value it folds to is a itself
        pr = self.open(j0)
        pr[0] = [pr[0][0], pr[0][0]]
        self.retarget(j0, pr, 0)
        self.add(j0, pr, "a == b at layer 0")
        # one bit of a layer-0 value: only (q, 0) sees it
        pr = self.open(j0)
        pr[0][1] ^= 1 << 200
        self.add(j0, pr, "bit of b at layer 0", single=0)
        # one bit of the final layer at slot 1: only (q, last)
        jf = n_final + 1 if n_final + 1 < m // 2 else 1
        self.final[1] ^= 1
        self.add(jf, self.open(jf), "bit of final[1]", single=n_layers - 1)
        if n_layers >= 3:
            # one bit of the target of a MIDDLE step (q, k): that value is also a or b of step k + 1, whose other
            # member is re-solved so that step k + 1 still folds to its own target
            k = n_layers // 2 - 1 if n_layers > 3 else 0
            pr = self.open(j0)
            jk = j0 % (m >> (k + 1))
            side = 0 if jk < (m >> (k + 2)) else 1
            pr[k + 1][side] ^= 1 << 17
            self.resolve_other(j0, pr, k + 1, side)
            self.add(j0, pr, "bit of the target of step %d" % k, single=k)
        # felts >= p: in a, in b, in the next pair's compared member, in the final layer (slot 2)
        for what, (k, side) in (("a", (0, 0)), ("b", (n_layers - 1, 1))):
            pr = self.open(j0)
            pr[k][side] = P if side == 0 else 2**256 - 1
            self.add(j0, pr, "%s >= p at layer %d" % (what, k))
        self.final[2] = P + 7
        jf = n_final + 2 if n_final + 2 < m // 2 else 2
        self.add(jf, self.open(jf), "final[2] >= p")
        for j in (m // 2, m - 1, 2**40 + 1, 2**64 - 1):
            self.add(j, self.open(j % (m // 2)), "index >= m / 2")
        self.expected = fold_statuses(log_m, n_layers, self.betas, self.index, self.pairs, self.final)

    def open(self, j):
        out, jk = [], j
        for k in range(self.n_layers):
            mk = 1 << (self.log_m - k)
            jk %= mk // 2
            out.append([self.layers[k][jk], self.layers[k][jk + mk // 2]])
        return out

    def retarget(self, j, pr, k):
        """Make step k of the query fold to what its pair says (changes the member of pair k + 1 it is compared with)."""
        mk = 1 << (self.log_m - k)
        jk = j % (mk // 2)
        v = fold_value(pr[k][0], pr[k][1], self.betas[k], fold_x(self.log_m, k, jk))
        assert k + 1 < self.n_layers or self.n_layers == 1
        if k + 1 < self.n_layers:
            pr[k + 1][0 if jk < mk // 4 else 1] = v

    def resolve_other(self, j, pr, k, kept_side):
        """Re-solve the member of pair k that is NOT kept_side so that step k folds to its unchanged target:
        folded = a (1/2 + beta/(2x)) + b (1/2 - beta/(2x))."""
        mk = 1 << (self.log_m - k)
        jk = j % (mk // 2)
        x = fold_x(self.log_m, k, jk)
        h, t = pow(2, -1, P), self.betas[k] * pow(2 * x, -1, P) % P
        ca, cb = (h + t) % P, (h - t) % P
        target = pr[k + 1][0 if jk < mk // 4 else 1] if k + 1 < self.n_layers else self.final[jk]
        if kept_side == 0:
            pr[k][1] = (target - pr[k][0] * ca) * pow(cb, -1, P) % P
        else:
            pr[k][0] = (target - pr[k][1] * cb) * pow(ca, -1, P) % P

    def add(self, j, pairs, note, single=None):
        if single is not None:
            self.single[len(self.index)] = single
        self.index.append(j)
        self.pairs.append(pairs)
        self.notes.append(note)

    def arrays(self):
        flat = [v for pr in self.pairs for pair in pr for v in pair]
        return np.array(self.index, dtype=np.uint64), felts_np(flat), felts_np(self.final), felts_np(self.betas)


@functools.lru_cache(maxsize=None)
def fri_case(log_m, n_layers):
    return FriCase(log_m, n_layers)
