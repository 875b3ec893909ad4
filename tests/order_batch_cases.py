"""Cases of sp_order_batch (include/starkperp.h, csrc/merkle.hip), shared by tests/test_order_batch_cases_cpu.py (no
GPU) and tests/test_gpu_order_batch.py.  Seeded.  Nothing of starkperp is imported: every expected value is Python
integers on oracle/ref_py.py and oracle/cref.py (the C comparator).

  message hashes   the left fold of the words, one cref.opt_pedersen_hash_many call per link across the batch
  order ids        (z >> id_shift) & (2**64 - 1)
  verdicts         cref.verify_codes for point keys, ref_py.verify on the integer key for x-only keys
  roots            sparse_root: the induced subtree of a {key: leaf} dict, one oracle call per level; a tree that
                   holds state has the root of the union of everything written, so a TreeCase keeps a running dict
  signatures       ref_py.sign, or sign_many: ref_py.sign's arithmetic from a chosen nonce k, R = k G from
                   cref.public_keys_many

The outcome of a call follows the rules of `expect` below, in the order the call applies them.

Oracle time, one family at a time on 8 cores: 2.5 s for a history (900 signatures, five roots), 1.5 s for a batch
of 32 x-only keys (ref_py.verify, pure Python), below 1 s for every other case."""
import functools
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import cref  # noqa: E402
from oracle import ref_py as R  # noqa: E402

P = R.FIELD_PRIME
EC_ORDER = R.EC_ORDER
BOUND = 2**251  # constants.cairo:57 SIGNED_MESSAGE_BOUND
MASK64 = 2**64 - 1
OK, BAD_ARGUMENT = 0, -3
HASH_OUT_OF_RANGE, NOT_COMMITTED = 1, 0x80
TABLE_SLOTS = 1 << 16  # a tree's first slot table (csrc/merkle.hip tree_initial_slots)


# ---- arrays ---------------------------------------------------------------------------------------------------------
def felts_np(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).astype(np.uint64)


def ints_of(arr):
    raw = np.ascontiguousarray(arr).astype("<u8").tobytes()
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(raw) // 32)]


# ---- the oracle side ------------------------------------------------------------------------------------------------
def hash_many(xs, ys):
    """(outputs, status bytes) of the C comparator; nothing is asked for an empty list."""
    if not xs:
        return [], []
    return cref.opt_pedersen_hash_many(list(xs), list(ys))


def fold_words(words):
    """words[k][i] = word k of order i -> (z, status): the left fold link by link across the batch, status[i] the OR
    of chain i's status bytes.  A chain of one word is the word itself: nothing is hashed, nothing is range-checked."""
    z, st = list(words[0]), [0] * len(words[0])
    for row in words[1:]:
        z, s = hash_many(z, row)
        st = [a | b for a, b in zip(st, s)]
    return z, st


@functools.lru_cache(maxsize=None)
def empty_roots(height, empty_leaf):
    out = [empty_leaf]
    for _ in range(height):
        out.append(hash_many([out[-1]], [out[-1]])[0][0])
    return out


def sparse_root(height, leaves, empty_leaf=0):
    """Root of the tree that holds {key: leaf} and `empty_leaf` everywhere else, level by level (merkle_tree.py:18-26:
    parents = set(index // 2)), one oracle call per level."""
    empties = empty_roots(height, empty_leaf)
    layer = dict(leaves)
    if not layer:
        return empties[height]
    for level in range(height):
        parents = sorted(set(i >> 1 for i in layer))
        e = empties[level]
        out, st = hash_many([layer.get(2 * i, e) for i in parents], [layer.get(2 * i + 1, e) for i in parents])
        assert not any(st)
        layer = dict(zip(parents, out))
    assert list(layer) == [0]
    return layer[0]


def node_count(height, keys):
    """How many nodes an update of `keys` hashes or writes, leaves and root included: one per distinct key >> l at
    every level l (what tree_level_counts of csrc/merkle.hip sums up; tree_reserve is asked for this many)."""
    return sum(len(set(k >> l for k in keys)) for l in range(height + 1)) if keys else 0


def sign_with_nonce(z, d, k, rx):
    """ref_py.sign (signature.py:137-173) from the point it has k and r = (k G).x; None where it would draw again."""
    r = rx
    if not (1 <= r < 2**R.N_ELEMENT_BITS_ECDSA):
        return None
    if (z + r * d) % EC_ORDER == 0:
        return None
    w = R.div_mod(k, z + r * d, EC_ORDER)
    if not (1 <= w < 2**R.N_ELEMENT_BITS_ECDSA):
        return None
    return r, R.inv_mod_curve_size(w)


def sign_many(zs, ds, rng):
    """Signatures of zs[i] < 2^251 under the private keys ds[i], nonces from `rng`, every k G in one oracle call."""
    out, todo = [None] * len(zs), list(range(len(zs)))
    while todo:
        ks = [rng.randrange(1, EC_ORDER) for _ in todo]
        pts = cref.public_keys_many(ks)
        for i, k, pt in zip(todo, ks, pts):
            assert 0 <= zs[i] < BOUND
            out[i] = sign_with_nonce(zs[i], ds[i], k, pt[0])
        todo = [i for i in todo if out[i] is None]
    return out


def xonly_code(z, r, s, x):
    """The verdict code of an x-only key: ref_py.verify on the integer key, its assertions as SP_VERIFY_ASSERT_*."""
    try:
        return 1 if R.verify(z, r, s, x) else 0
    except AssertionError as e:
        return {"s =": 2, "r =": 3, "w =": 4, "msg": 5}[str(e)[:3]]


def c_order_id(z, id_shift):
    """The extraction of sp_order_batch restated word for word: z as four 64-bit words, w = id_shift >> 6,
    sh = id_shift & 63, v = z[w] >> sh; if (sh && w + 1 < 4) v |= z[w + 1] << (64 - sh), in 64-bit arithmetic."""
    zw = [(z >> (64 * j)) & MASK64 for j in range(4)]
    w, sh = id_shift >> 6, id_shift & 63
    v = zw[w] >> sh
    if sh and w + 1 < 4:
        v |= (zw[w + 1] << (64 - sh)) & MASK64
    return v


# ---- one call and what it must do -----------------------------------------------------------------------------------
class Call:
    """One sp_order_batch call: words[k][i], signatures, keys (points; x-only sends the x alone), leaves, id_shift;
    after TreeCase.add also what the call must answer (`expect`)."""

    def __init__(self, words, sigs, keys, leaves, id_shift=187, xonly=False, note=""):
        self.words = [list(row) for row in words]
        self.depth, self.n = len(self.words), len(self.words[0])
        self.r, self.s = [a for a, _ in sigs], [b for _, b in sigs]
        self.keys, self.leaves, self.id_shift, self.xonly, self.note = list(keys), list(leaves), id_shift, xonly, note
        assert all(len(row) == self.n for row in self.words)
        assert len(self.r) == len(self.keys) == len(self.leaves) == self.n

    def arrays(self):
        """(words uint64[depth, n, 4], r, s, qx, qy or None, leaves) as batch_np.order_batch takes them."""
        words = np.stack([felts_np(row) for row in self.words])
        qy = None if self.xonly else felts_np([k[1] for k in self.keys])
        return words, felts_np(self.r), felts_np(self.s), felts_np([k[0] for k in self.keys]), qy, felts_np(self.leaves)

    def oracle_codes(self, z):
        if self.xonly:
            return [xonly_code(zz, r, s, k[0]) for zz, r, s, k in zip(z, self.r, self.s, self.keys)]
        return cref.verify_codes(z, self.r, self.s, self.keys) if self.n else []


def expect(call, height):
    """The outcome of a call on a tree of `height`, in the order sp_order_batch decides:
      rc         SP_OK or SP_ERR_BAD_ARGUMENT (then nothing else is specified and the tree is as it was)
      z          the message hashes, None where they are unspecified (a word out of range)
      verdicts   the oracle's codes; all 0 when a word was out of range
      status     *tree_status: 0, the SP_HASH_OUT_OF_RANGE byte or SP_TREE_NOT_COMMITTED
      committed  status == 0: the tree holds the leaves at the ids (an empty batch commits nothing and says 0)"""
    call.rc, call.status, call.committed, call.ids = OK, 0, False, None
    z, st = fold_words(call.words)
    chain_status = 0
    for b in st:
        chain_status |= b
    if chain_status:  # a word >= p at depth >= 2: nothing else runs
        call.z, call.verdicts, call.status = None, [0] * call.n, chain_status
        return
    call.z = z
    call.verdicts = call.oracle_codes(z)
    if any(v >= BOUND for v in z):  # no signed message, no 64-bit order id: verdicts only
        assert all(c == 5 for v, c in zip(z, call.verdicts) if v >= BOUND and c not in (2, 3, 4))
        call.status = NOT_COMMITTED
        return
    call.ids = [(v >> call.id_shift) & MASK64 for v in z]
    if len(set(call.ids)) < call.n or any(i >> height for i in call.ids):
        call.rc, call.verdicts = BAD_ARGUMENT, None
        return
    if any(v >= P for v in call.leaves):  # found by the level hashing, before the verifier is asked
        call.status = HASH_OUT_OF_RANGE
        return
    if any(c != 1 for c in call.verdicts):
        call.status = NOT_COMMITTED
        return
    call.committed = True


class TreeCase:
    """One tree (height, empty leaf, seed written with one plain update) and the calls made on it in sequence; every
    call carries the dict the tree holds before and after it and the roots of both."""

    def __init__(self, name, height=64, empty_leaf=0, seed=None):
        self.name, self.height, self.empty_leaf = name, height, empty_leaf
        self.seed = dict(seed or {})
        self.state = dict(self.seed)
        self.root = self.seed_root = sparse_root(height, self.state, empty_leaf)
        self.calls = []

    def add(self, call):
        call.before, call.old_root = dict(self.state), self.root
        expect(call, self.height)
        if call.committed and call.n:
            self.state.update(zip(call.ids, call.leaves))
            self.root = sparse_root(self.height, self.state, self.empty_leaf)
        call.after, call.new_root = dict(self.state), self.root
        self.calls.append(call)
        return call

    def __repr__(self):
        return self.name


# ---- signers of the cases -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signers(count, seed="order-batch-keys"):
    """(private keys, public points) - count distinct keys."""
    rng = random.Random(seed)
    ds = [rng.randrange(1, EC_ORDER) for _ in range(count)]
    return ds, cref.public_keys_many(ds)


def signed_call(rng, words, leaves, id_shift=187, n_keys=8, xonly=False, note="", key_seed="order-batch-keys"):
    """A call whose signatures are honest: order i signed by key i % n_keys over the oracle's message hash (words that
    do not hash, or hash to 2^251 and more, are signed as the hash reduced below 2^251 - they are refused anyway)."""
    ds, pts = signers(n_keys, key_seed)
    z, _ = fold_words(words)
    n = len(z)
    sigs = sign_many([v % BOUND for v in z], [ds[i % n_keys] for i in range(n)], rng)
    return Call(words, sigs, [pts[i % n_keys] for i in range(n)], leaves, id_shift, xonly, note)


def distinct_leaves(rng, n):
    out = set()
    while len(out) < n:
        out.add(rng.randrange(1, P))
    out = list(out)
    rng.shuffle(out)
    return out


def z_with_ids(rng, ids, id_shift=187):
    """Message hashes below 2^251 whose id window holds `ids`, random bits below it (and above it, where there are)."""
    out = []
    for i in ids:
        z = (rng.randrange(BOUND) & ~(MASK64 << id_shift)) | (i << id_shift)
        assert z < BOUND and (z >> id_shift) & MASK64 == i
        out.append(z)
    return out


# ---- family: id windows ---------------------------------------------------------------------------------------------
ID_SHIFTS = (0, 1, 59, 63, 64, 65, 128, 187, 188, 191, 192)


def window_bits(id_shift):
    """How many bits of the 64-bit window lie below bit 251."""
    return min(64, 251 - id_shift)


def window_patterns(id_shift, rng):
    """[(z, kind)] for one shift: the window all zeros, all ones, single bits at both ends, with the bits just
    outside it (id_shift - 1, id_shift + 64) and all bits outside it set or clear; then random ones.  kind: "sparse"
    (at most two window bits set), "dense" (at most one clear) or "random"."""
    a = window_bits(id_shift)
    m, top = (1 << a) - 1, id_shift + 64
    lo_all, lo_adj = (1 << id_shift) - 1, (1 << id_shift) >> 1
    hi_all = ((BOUND - 1) >> top) << top if top < 251 else 0
    hi_adj = 1 << top if top < 251 else 0
    rows = [
        (0, lo_adj | hi_adj, "sparse"),
        (m, 0, "dense"),
        (1, lo_all | hi_all, "sparse"),
        (1 << (a - 1), 0, "sparse"),
        ((1 << (a - 1)) | 1, lo_adj | hi_adj, "sparse"),
        (m - 1, lo_all, "dense"),
        (m >> 1, hi_all, "dense"),
        (2, lo_all | hi_all, "sparse"),
        (1 << (a - 2), lo_adj | hi_adj, "sparse"),
    ]
    seen = {w for w, _, _ in rows}
    while len(rows) < 12:
        w = rng.randrange(1 << a)
        if w not in seen:
            seen.add(w)
            rows.append((w, rng.randrange(BOUND) & (lo_all | hi_all), "random"))
    out = []
    for w, outside, kind in rows:
        assert outside & (MASK64 << id_shift) & (BOUND - 1) == 0
        z = (w << id_shift) | outside
        assert z < BOUND
        out.append((z, kind))
    return out


@functools.lru_cache(maxsize=None)
def id_window_case(id_shift):
    rng = random.Random("order-batch-window-%d" % id_shift)
    pats = window_patterns(id_shift, rng)
    rng.shuffle(pats)
    case = TreeCase("window-shift-%d" % id_shift, 64, 0, {3: 33, 2**63 + 5: 55})
    case.kinds = [k for _, k in pats]
    case.add(signed_call(rng, [[z for z, _ in pats]], distinct_leaves(rng, len(pats)), id_shift))
    return case


# ---- family: sort shapes --------------------------------------------------------------------------------------------
SORT_SIZES = (0, 1, 2, 16, 17, 33, 257)
SORT_PATTERNS = ("top16", "descending", "extremes", "adjacent", "random")
SORT_SHAPES = [(p, n) for n in SORT_SIZES for p in SORT_PATTERNS if n >= 2 or p == "random"]


def sort_ids(pattern, n, rng):
    """n distinct ids in an input order that is not the sorted one (n >= 2)."""
    ids = set()
    if pattern == "top16":  # one bucket of the counting pass at every size: the top 16 bits are shared
        top = rng.randrange(1 << 16) << 48
        while len(ids) < n:
            ids.add(top | rng.randrange(1 << 48))
    elif pattern == "adjacent":  # runs k .. k + 3: sibling pairs that are both new
        while len(ids) < n:
            k = rng.randrange(1 << 62) << 2
            ids.update(range(k, k + min(4, n - len(ids))))
    else:
        if pattern == "extremes":
            ids.update((0, MASK64))
        while len(ids) < n:
            ids.add(rng.randrange(1 << 64))
    ids = sorted(ids)
    if pattern == "descending":
        return ids[::-1]
    rng.shuffle(ids)
    if ids == sorted(ids) and n >= 2:
        ids[0], ids[1] = ids[1], ids[0]
    return ids


@functools.lru_cache(maxsize=None)
def sort_case(pattern, n):
    rng = random.Random("order-batch-sort-%s-%d" % (pattern, n))
    case = TreeCase("sort-%s-%d" % (pattern, n), 64, 0, {5: 7, 2**63 + 11: 9})
    z = z_with_ids(rng, sort_ids(pattern, n, rng))
    case.add(signed_call(rng, [z], distinct_leaves(rng, n)))
    return case


# ---- family: duplicates ---------------------------------------------------------------------------------------------
DUPLICATES = [(where, n) for n in (5, 40) for where in ("ends", "front", "middle")]


@functools.lru_cache(maxsize=None)
def duplicate_case(where, n):
    """Two orders with one id (different message hashes: the bits below the window differ), then the batch without
    the second of them.  "middle": every id shares its top 16 bits, the pair sits in the middle of the one bucket."""
    rng = random.Random("order-batch-dup-%s-%d" % (where, n))
    ids = sort_ids("top16" if where == "middle" else "random", n, rng)
    i, j = {"ends": (0, n - 1), "front": (0, 1), "middle": (n // 2 - 1, n // 2 + 1)}[where]
    case = TreeCase("dup-%s-%d" % (where, n), 64, 0, {9: 9})
    leaves = distinct_leaves(rng, n)
    case.add(signed_call(rng, [z_with_ids(rng, ids[:j] + [ids[i]] + ids[j + 1:])], leaves))
    case.add(signed_call(rng, [z_with_ids(rng, ids)], leaves))
    return case


# ---- family: depths -------------------------------------------------------------------------------------------------
DEPTH_KINDS = (1, 2, 3, 6, "limit")
DEPTH_TREES = ((187, 64), (192, 59), (192, 64))  # (id_shift, height): ids of shift 192 are below 2^59


def limit_order_args(rng):
    """Arguments of perpetual_messages.py:212-236 inside their bounds."""
    return (rng.randrange(2**128), rng.randrange(2**250), rng.randrange(2) == 1, rng.randrange(2**250),
            rng.randrange(2**64), rng.randrange(2**64), rng.randrange(2**64), rng.randrange(2**32), rng.randrange(2**64),
            rng.randrange(2**32))


@functools.lru_cache(maxsize=None)
def depth_words(kind, n=64):
    """(words[k][i], limit-order arguments or None)."""
    rng = random.Random("order-batch-depth-%s" % kind)
    if kind == "limit":
        args = [limit_order_args(rng) for _ in range(n)]
        return [list(col) for col in zip(*[R.limit_order_words(*a) for a in args])], args
    if kind == 1:  # the words are the hashes: below 2^251
        return [[rng.randrange(BOUND) for _ in range(n)]], None
    return [[rng.randrange(P) for _ in range(n)] for _ in range(kind)], None


@functools.lru_cache(maxsize=None)
def depth_signed(kind):
    rng = random.Random("order-batch-depth-sign-%s" % kind)
    words, _ = depth_words(kind)
    return signed_call(rng, words, distinct_leaves(rng, len(words[0])))


@functools.lru_cache(maxsize=None)
def depth_case(kind, id_shift, height):
    base = depth_signed(kind)
    case = TreeCase("depth-%s-shift-%d-height-%d" % (kind, id_shift, height), height, 0, {1: 2})
    case.add(Call(base.words, list(zip(base.r, base.s)), base.keys, base.leaves, id_shift))
    return case


# ---- family: low trees ----------------------------------------------------------------------------------------------
LOW_HEIGHTS = (1, 8, 63)


@functools.lru_cache(maxsize=None)
def low_tree_case(height):
    """Ids that fit (both ends of the key range among them); then one id that does not; then a good batch again."""
    rng = random.Random("order-batch-low-%d" % height)
    top = (1 << height) - 1
    n = min(1 << height, 20)
    ids = {0, top}
    while len(ids) < n:
        ids.add(rng.randrange(top + 1))
    ids = list(ids)
    rng.shuffle(ids)
    case = TreeCase("low-tree-%d" % height, height, 0)
    case.add(signed_call(rng, [z_with_ids(rng, ids)], distinct_leaves(rng, n)))
    over = ids[:n // 2] + [top + 1] + ids[n // 2 + 1:]
    case.add(signed_call(rng, [z_with_ids(rng, over)], distinct_leaves(rng, n)))
    case.add(signed_call(rng, [z_with_ids(rng, ids[::-1])], distinct_leaves(rng, n)))
    return case


# ---- family: verdict codes ------------------------------------------------------------------------------------------
def off_curve_point(rng):
    """(x, y) not on the curve whose x is on no curve point at all: the x-only run has no y for it."""
    while True:
        x = rng.randrange(P)
        if not R.is_valid_stark_key(x):
            return (x, rng.randrange(P))


def w_out_of_range_s(rng):
    """An s in [1, EC_ORDER) whose inverse is 2^251 or more (signature.py:226)."""
    w = rng.randrange(BOUND, EC_ORDER)
    return R.inv_mod_curve_size(w)


# label -> the code the label promises under point keys (None: whatever the oracle says)
CODE_LABELS = {"s flipped": 0, "r = 0": 3, "r = 2^251": 3, "s = 0": 2, "s = EC_ORDER": 2, "w >= 2^251": 4,
               "z >= 2^251": 5, "off curve": 6, "y negated": None}


@functools.lru_cache(maxsize=None)
def verdict_batch(which, xonly, n=32):
    """which: "codes" (one order per label of CODE_LABELS, the others valid), "codes-signed" (the same without the
    z >= 2^251 order, so that the batch takes the verifier-thread path), "first" / "last" (exactly one bad signature,
    at position 0 / n - 1), "repeated" (all valid, 4 keys), "distinct" (all valid, a key per order).
    Returns the TreeCase; `labels` on it maps position -> label."""
    rng = random.Random("order-batch-verdicts-%s" % which)  # the same batch for point keys and x-only keys
    n_keys = {"repeated": 4, "distinct": n}.get(which, 8)
    z = [rng.randrange(BOUND) for _ in range(n)]
    call = signed_call(rng, [z], distinct_leaves(rng, n), n_keys=n_keys, xonly=xonly)
    labels = {}
    if which in ("codes", "codes-signed"):
        spots = rng.sample(range(n), len(CODE_LABELS))
        labels = {pos: lab for pos, lab in zip(spots, CODE_LABELS) if not (which == "codes-signed" and lab == "z >= 2^251")}
    elif which in ("first", "last"):
        labels = {0 if which == "first" else n - 1: "s flipped"}
    for pos, lab in labels.items():
        if lab == "s flipped":
            call.s[pos] ^= 2
        elif lab == "r = 0":
            call.r[pos] = 0
        elif lab == "r = 2^251":
            call.r[pos] = BOUND
        elif lab == "s = 0":
            call.s[pos] = 0
        elif lab == "s = EC_ORDER":
            call.s[pos] = EC_ORDER
        elif lab == "w >= 2^251":
            call.s[pos] = w_out_of_range_s(rng)
        elif lab == "z >= 2^251":  # below p, the same low 251 bits as the message that was signed
            low = rng.randrange(2**192)
            call.words[0][pos] = BOUND + low
            call.r[pos], call.s[pos] = sign_many([low], [signers(n_keys)[0][pos % n_keys]], rng)[0]
        elif lab == "off curve":
            call.keys[pos] = off_curve_point(rng)
        elif lab == "y negated":
            call.keys[pos] = (call.keys[pos][0], P - call.keys[pos][1])
    case = TreeCase("verdicts-%s-%s" % (which, "xonly" if xonly else "points"), 64, 0, {7: 9})
    case.labels = labels
    case.add(call)
    return case


VERDICT_BATCHES = ("codes", "codes-signed", "first", "last", "repeated", "distinct")


# ---- family: leaves -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leaves_case():
    """A tree whose empty leaf is not zero.  Calls: leaves equal to the empty leaf, p - 1 and 0 among ordinary ones
    (commits); a leaf = p alone; a leaf = p with a bad signature elsewhere; a leaf = 2^256 - 1; a good batch."""
    rng = random.Random("order-batch-leaves")
    empty, n = 12345, 8
    case = TreeCase("leaves", 64, empty, {2**40: 77})
    ids = sort_ids("random", n, rng)
    first = distinct_leaves(rng, n)
    first[1], first[4], first[6] = empty, P - 1, 0
    case.add(signed_call(rng, [z_with_ids(rng, ids)], first, note="empty leaf, p - 1, 0"))
    for note, bad_leaf, bad_sig in (("leaf = p", P, None), ("leaf = p and a bad signature", P, 5),
                                    ("leaf = 2^256 - 1", 2**256 - 1, None)):
        leaves = distinct_leaves(rng, n)
        leaves[2] = bad_leaf
        call = signed_call(rng, [z_with_ids(rng, sort_ids("random", n, rng))], leaves, note=note)
        if bad_sig is not None:
            call.s[bad_sig] ^= 4
        case.add(call)
    # over the first call's keys: the empty-valued key gets a value, a valued key becomes empty again
    again = distinct_leaves(rng, n)
    again[0] = empty
    case.add(signed_call(rng, [z_with_ids(rng, ids)], again, note="overwrite, one key back to empty"))
    return case


# ---- family: words --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def words_case():
    """A word = p at depth 3, first and last; a depth-1 word in [p, 2^256) (it IS the message hash: no signed
    message), also beside equal ids and a leaf out of range; the same batches with the word put right."""
    rng = random.Random("order-batch-words")
    n = 8
    case = TreeCase("words", 64, 0, {11: 13})
    good = [[rng.randrange(P) for _ in range(n)] for _ in range(3)]
    for k, note in ((0, "first word = p"), (2, "last word = p")):
        words = [list(row) for row in good]
        words[k][3] = P
        case.add(signed_call(rng, words, distinct_leaves(rng, n), note=note))
    case.add(signed_call(rng, good, distinct_leaves(rng, n), note="depth 3, all words felts"))
    flat = [rng.randrange(BOUND) for _ in range(n)]
    for big, note in ((P, "depth-1 word = p"), (2**256 - 1, "depth-1 word = 2^256 - 1")):
        words = list(flat)
        words[6] = big
        case.add(signed_call(rng, [words], distinct_leaves(rng, n), note=note))
    # no signed message beside equal ids and a leaf = p: the batch ends after the verification, neither is reported
    words, leaves = list(flat), distinct_leaves(rng, n)
    words[6], words[1], leaves[2] = BOUND + 5, words[0] ^ 1, P
    case.add(signed_call(rng, [words], leaves, note="hash = 2^251 + 5 beside equal ids and a leaf = p"))
    case.add(signed_call(rng, [flat], distinct_leaves(rng, n), note="depth 1, all hashes signed messages"))
    return case


# ---- family: history ------------------------------------------------------------------------------------------------
GROWTH_ORDERS = 640


@functools.lru_cache(maxsize=None)
def history_case(seed=0):
    """One tree, in sequence: the seed (a plain update); 64 orders commit; the same ids with new leaves commit; one
    bad signature: refused; GROWTH_ORDERS orders - more nodes than half of the first slot table, so the table grows -
    with one bad signature: refused after the growth; 64 orders commit."""
    rng = random.Random("order-batch-history-%d" % seed)
    case = TreeCase("history-%d" % seed, 64, 0, {rng.randrange(2**64): rng.randrange(1, P) for _ in range(50)})
    z = z_with_ids(rng, sort_ids("random", 64, rng))
    first = case.add(signed_call(rng, [z], distinct_leaves(rng, 64), n_keys=16, note="commit"))
    case.add(Call(first.words, list(zip(first.r, first.s)), first.keys, distinct_leaves(rng, 64), note="overwrite"))
    bad = signed_call(rng, [z_with_ids(rng, sort_ids("random", 64, rng))], distinct_leaves(rng, 64), n_keys=16,
                      note="one bad signature")
    bad.s[40] ^= 1 << 100
    case.add(bad)
    big = signed_call(rng, [z_with_ids(rng, sort_ids("random", GROWTH_ORDERS, rng))], distinct_leaves(rng, GROWTH_ORDERS),
                      n_keys=16, note="grows the table, one bad signature")
    big.r[GROWTH_ORDERS - 1] ^= 1
    case.add(big)
    case.add(signed_call(rng, [z_with_ids(rng, sort_ids("random", 64, rng))], distinct_leaves(rng, 64), n_keys=16,
                         note="commit after the refused growth"))
    return case


# ---- argument edges -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_good_case(n=4):
    """A good batch of n orders for the calls that vary an argument, not the data."""
    rng = random.Random("order-batch-arguments")
    case = TreeCase("arguments", 64, 0, {21: 12})
    case.add(signed_call(rng, [z_with_ids(rng, sort_ids("random", n, rng))], distinct_leaves(rng, n)))
    return case
