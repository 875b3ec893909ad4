"""The shared case table of tests/test_verify_update_cpu.py and tests/test_gpu_verify_update.py: multi-updates, their
witnesses, and what a verifier of merkle_multi_update's statement (state/state.cairo:155-173) must say about each way of
spoiling them.  A case is (height, empty leaf, initial leaves, modifications); `build` runs it on a tree (the host twin
on the oracle hash, or the library's tree) and keeps what a verifier is given; a tamper changes ONE thing in a copy and
states the exact status bytes it must cause.  The expected bytes are derived here from the positions of the records
(witness_replay.layout) alone - never from the code under test.

Shapes, the smallest at which each piece can go wrong:
  A1, A2  height 1, one key / both keys: R = 1, the root's children are leaves; one side off every path, then none
  B       height 3, all 8 keys: no child off a path anywhere
  C       height 64, keys {0, 1, 2^63, 2^64 - 2, 2^64 - 1}: the shift at level 64, both ends of the key range
  D       height 64, 300 random keys on a tree that holds 300 others: R about 1.7 x 10^4, so the 2 R hashes are past the
          8192-item edge of the latency classes and the check kernel runs several 256-thread blocks
  E       height 12, 1100 keys out of 2048: paths merge from level 1 on, and more than 1024 keys take a second tile
          of the kernel that lists a level's nodes"""
import collections
import copy
import random

from oracle import ref_py as R
from witness_replay import layout

P = R.FIELD_PRIME
OUT_OF_RANGE, UNHASHABLE = 0x01, 0x02                                        # include/starkperp.h SP_HASH_*
HASH_MISMATCH, LINK_MISMATCH, SIBLING_CHANGED, ROOT_MISMATCH = 0x04, 0x08, 0x20, 0x40  # SP_WITNESS_*

Case = collections.namedtuple("Case", "name height empty_leaf initial modifications")


def _leaves(rng, keys):
    return {k: rng.randrange(1, P) for k in keys}


def _distinct(rng, height, n, avoid=()):
    out = set()
    while len(out) < n:
        k = rng.randrange(1 << height)
        if k not in avoid:
            out.add(k)
    return sorted(out)


def _cases():
    rng = random.Random(20260419)
    top = 2**64 - 1
    d_initial = _distinct(rng, 64, 300)
    d_keys = _distinct(rng, 64, 300, avoid=set(d_initial))
    e_keys = sorted(rng.sample(range(2048), 1100))
    return [
        Case("A1", 1, 0, {0: 5}, _leaves(rng, [1])),
        Case("A2", 1, 7, {}, _leaves(rng, [0, 1])),
        Case("B", 3, 0, _leaves(rng, [2, 5]), _leaves(rng, range(8))),
        Case("C", 64, 0, _leaves(rng, [1, 2**63 + 1, top - 1]), _leaves(rng, [0, 1, 2**63, top - 1, top])),
        Case("D", 64, 0, _leaves(rng, d_initial), _leaves(rng, d_keys)),
        Case("E", 12, 3, _leaves(rng, rng.sample(range(2048, 4096), 40) + e_keys[:50]), _leaves(rng, e_keys)),
    ]


CASES = {c.name: c for c in _cases()}
TAMPERED = ("A1", "A2", "D")  # the cases every tamper is applied to
FORGED = ("A1", "C", "D", "E")  # the cases with a key outside the modifications to forge a change at


class Instance:
    """What a verifier of one case is handed: sorted keys, the leaves and roots before and after, the two witnesses as
    lists of (level, index, node, left, right) tuples; and the positions of the records."""

    def __init__(self, case, keys, prev_leaves, new_leaves, prev_root, new_root, before, after):
        self.case, self.height, self.keys = case, case.height, keys
        self.prev_leaves, self.new_leaves = list(prev_leaves), list(new_leaves)
        self.prev_root, self.new_root = prev_root, new_root
        self.before, self.after = list(before), list(after)
        self.keys_set = set(keys)
        self.layout = layout(case.height, keys)
        self.place = {pos: u for u, pos in enumerate(self.layout)}
        self.records = len(self.layout)

    def clone(self):
        """A copy whose leaves, roots and records can be changed; the (read-only) positions are shared."""
        other = copy.copy(self)
        other.prev_leaves, other.new_leaves = list(self.prev_leaves), list(self.new_leaves)
        other.before, other.after = list(self.before), list(self.after)
        return other

    def half(self, h):
        return self.after if h else self.before

    def on_path(self, u, c):
        """Whether child c of record u lies on a key's path."""
        level, idx = self.layout[u]
        child = 2 * idx + c
        return child in self.keys_set if level == 1 else (level - 1, child) in self.place

    def parent(self, u):
        level, idx = self.layout[u]
        return self.place[(level + 1, idx >> 1)]

    def spots(self):
        """The four records every tamper is tried at: the first, the last of level 1, one in the middle, the root."""
        level1 = sum(1 for level, _ in self.layout if level == 1)
        return sorted({0, level1 - 1, self.records // 2, self.records - 1})

    def clean(self):
        return [[0] * self.records, [0] * self.records]


def build(case, make_tree):
    """Runs the case on make_tree(height, empty_leaf) - anything with update / get_many / witness / root."""
    tree = make_tree(case.height, case.empty_leaf)
    if case.initial:
        tree.update(dict(case.initial))
    keys = sorted(case.modifications)
    prev_leaves = tree.get_many(keys)
    before = tree.witness(keys)
    prev_root, new_root = tree.update(dict(case.modifications))
    after = tree.witness(keys)
    inst = Instance(case, keys, prev_leaves, [case.modifications[k] for k in keys], prev_root, new_root, before, after)
    return inst, tree


def _set(inst, h, u, **fields):
    rec = dict(zip(("level", "index", "node", "left", "right"), inst.half(h)[u]))
    rec.update(fields)
    inst.half(h)[u] = (rec["level"], rec["index"], rec["node"], rec["left"], rec["right"])


def _other(v):
    return (v + 1) % P


def _side(inst, u, on_path):
    """A side of record u that is (not) on a path, or None."""
    for c in (0, 1):
        if inst.on_path(u, c) == on_path:
            return c
    return None


def tampers(inst):
    """[(name, tampered copy, expected status [before bytes, after bytes])] - one tamper per status bit at each spot."""
    out = []

    def fresh():
        return inst.clone(), inst.clean()

    last = inst.records - 1
    for u in inst.spots():
        level, idx = inst.layout[u]
        for h in (0, 1):
            # a node changed in one half: its own hash no longer gives it, and its parent's child no longer is it
            t, want = fresh()
            _set(t, h, u, node=_other(inst.half(h)[u][2]))
            want[h][u] |= HASH_MISMATCH
            if u == last:
                want[h][u] |= ROOT_MISMATCH
            else:
                want[h][inst.parent(u)] |= LINK_MISMATCH
            out.append(("node changed, half %d, record %d" % (h, u), t, want))
            # a child on a path changed
            c = _side(inst, u, True)
            name = ("left", "right")[c]
            t, want = fresh()
            _set(t, h, u, **{name: _other(inst.half(h)[u][3 + c])})
            want[h][u] |= HASH_MISMATCH | LINK_MISMATCH
            out.append(("on-path child changed, half %d, record %d" % (h, u), t, want))
            # a child set to p: the hash reports the range, and no mismatch is claimed for a hash that was not taken
            t, want = fresh()
            _set(t, h, u, **{name: P})
            want[h][u] |= OUT_OF_RANGE | LINK_MISMATCH
            out.append(("on-path child = p, half %d, record %d" % (h, u), t, want))
            # left and right swapped
            left, right = inst.half(h)[u][3:5]
            if left != right:
                t, want = fresh()
                _set(t, h, u, left=right, right=left)
                want[h][u] |= HASH_MISMATCH | LINK_MISMATCH
                if _side(inst, u, False) is not None:  # the side off every path now shows the other child's value
                    want[0][u] |= SIBLING_CHANGED
                    want[1][u] |= SIBLING_CHANGED
                out.append(("children swapped, half %d, record %d" % (h, u), t, want))
        # a child off every path changed in the after half only
        c = _side(inst, u, False)
        if c is not None:
            t, want = fresh()
            _set(t, 1, u, **{("left", "right")[c]: _other(inst.after[u][3 + c])})
            want[0][u] |= SIBLING_CHANGED
            want[1][u] |= SIBLING_CHANGED | HASH_MISMATCH
            out.append(("off-path child changed after, record %d" % u, t, want))
            t, want = fresh()
            _set(t, 1, u, **{("left", "right")[c]: P})
            want[0][u] |= SIBLING_CHANGED
            want[1][u] |= SIBLING_CHANGED | OUT_OF_RANGE
            out.append(("off-path child = p after, record %d" % u, t, want))
    t, want = fresh()
    t.prev_root = _other(inst.prev_root)
    want[0][last] |= ROOT_MISMATCH
    out.append(("wrong prev_root", t, want))
    t, want = fresh()
    t.new_root = _other(inst.new_root)
    want[1][last] |= ROOT_MISMATCH
    out.append(("wrong new_root", t, want))
    for j in sorted({0, len(inst.keys) // 2, len(inst.keys) - 1}):
        at = inst.place[(1, inst.keys[j] >> 1)]
        t, want = fresh()
        t.prev_leaves[j] = _other(inst.prev_leaves[j])
        want[0][at] |= LINK_MISMATCH
        out.append(("wrong previous leaf %d" % j, t, want))
        t, want = fresh()
        t.new_leaves[j] = _other(inst.new_leaves[j])
        want[1][at] |= LINK_MISMATCH
        out.append(("wrong new leaf %d" % j, t, want))
    return out


def forgery_key(inst):
    """A key OUTSIDE the modifications, and the one position whose off-path child covers it: walking down from the root
    towards the key, the first node that is on no modified key's path is a child of exactly one record."""
    rng = random.Random(inst.records)
    while True:
        x = rng.randrange(1 << inst.height)
        if x not in inst.keys_set:
            break
    for level in range(inst.height, 0, -1):
        child = x >> (level - 1)
        below = child in inst.keys_set if level == 1 else (level - 1, child) in inst.place
        if not below:
            return x, inst.place[(level, child >> 1)]
    raise AssertionError("unreachable: x is not a modified key")


def forge(case, inst, make_tree):
    """The consistent forgery: the after witness and the new root come from a twin tree in which forgery_key's leaf was
    ALSO changed.  Every record hashes, every link holds, both roots are right - only the untouched side differs.
    Returns (forged copy, expected status)."""
    x, at = forgery_key(inst)
    tree = make_tree(case.height, case.empty_leaf)
    if case.initial:
        tree.update(dict(case.initial))
    mods = dict(case.modifications)
    mods[x] = _other(tree.get_many([x])[0])
    _, root = tree.update(mods)
    t = inst.clone()
    t.after, t.new_root = list(tree.witness(inst.keys)), root
    want = inst.clean()
    want[0][at] = want[1][at] = SIBLING_CHANGED
    return t, want
