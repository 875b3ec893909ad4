"""Leaf / tree conventions of the perpetual state (the callers either side of the hash kernels).

  * position_hash: services/perpetual/cairo/position/hash.cairo:22-74 (bounds
    definitions/constants.cairo:11-38);
  * orders-tree leaf = fulfilled amount felt, order id = top 64 bits of the 251-bit message hash
    (services/perpetual/cairo/order/order.cairo:23-59,122-124);
  * tree updates: merkle_multi_update call sites state/state.cairo:155-173.
All hashing goes through starkperp.batch (GPU)."""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

from . import batch

BALANCE_LOWER_BOUND = -(2**63)
BALANCE_UPPER_BOUND = 2**63
FUNDING_INDEX_LOWER_BOUND = -(2**63)
FUNDING_INDEX_UPPER_BOUND = 2**63
N_ASSETS_UPPER_BOUND = 2**16

Position = Tuple[int, int, Sequence[Tuple[int, int, int]]]  # (public_key, collateral, assets)


def pack_asset(asset_id: int, cached_funding_index: int, balance: int) -> int:
    """hash.cairo:30-36."""
    packed = asset_id
    packed = packed * (FUNDING_INDEX_UPPER_BOUND - FUNDING_INDEX_LOWER_BOUND) + (
        cached_funding_index - FUNDING_INDEX_LOWER_BOUND)
    return packed * (BALANCE_UPPER_BOUND - BALANCE_LOWER_BOUND) + (balance - BALANCE_LOWER_BOUND)


def position_words(position: Position) -> List[int]:
    """The chain  H(...H(H(0, a_1), a_2)..., public_key), tail)  as its input words."""
    public_key, collateral, assets = position
    tail = (collateral - BALANCE_LOWER_BOUND) * N_ASSETS_UPPER_BOUND + len(assets)
    return [0] + [pack_asset(*a) for a in assets] + [public_key, tail]


def position_hash(position: Position) -> int:
    """hash.cairo:58-74."""
    return batch.pedersen_chain(position_words(position))


def position_hashes_many(positions: Iterable[Position]) -> List[int]:
    """Many position leaves (chains of n_assets + 3 words).  Positions of one asset count run as equal-depth
    chains (batch.pedersen_chains_many); a batch whose asset counts differ goes out as ONE ragged call
    (batch.pedersen_chains_ragged) that lasts as long as its longest chain, not one call per depth."""
    words = [position_words(p) for p in positions]
    if len({len(w) for w in words}) <= 1:
        return batch.pedersen_chains_many(words)
    return batch.pedersen_chains_ragged(words)


def order_id_of(message_hash: int) -> int:
    """order/order.cairo:23-59: the 64 most significant bits of the 251-bit hash."""
    return message_hash >> 187


def orders_tree_root(fulfilled: Dict[int, int], height: int = 64) -> int:
    """Root of the orders tree (leaf = fulfilled amount, empty leaf 0) after writing `fulfilled`."""
    return batch.merkle_sparse_root(height, fulfilled, 0)


# ---- persistent sparse tree with a preimage ("facts") store -------------------------------------
class SparseMerkleTree:
    """Height-h Pedersen Merkle tree over 2^h leaves, stored sparsely as the reference stores it:
    a map node_hash -> (left, right) (`merkle_facts`, services/perpetual/cairo/main.cairo:39-40,
    61-64) plus the current root.  `update` is the equivalent of one
    merkle_multi_update{hash_ptr=pedersen_ptr} call (state/state.cairo:155-173): it walks the
    subtree induced by the modified leaves (starkware/python/merkle_tree.py:4-26), takes untouched
    siblings from the store and recomputes the touched nodes level by level - one batched GPU
    launch pair per level through `hash_many` (default: starkperp.batch.pedersen_hash_many).

    Only bookkeeping (dicts of ints) happens on the host; every hash goes through `hash_many`.
    """

    def __init__(self, height: int, empty_leaf: int = 0, hash_many=None):
        self.height = height
        self.hash_many = hash_many or batch.pedersen_hash_many
        self.facts: Dict[int, Tuple[int, int]] = {}
        self.empties = [empty_leaf]
        for _ in range(height):
            prev = self.empties[-1]
            node = self.hash_many([prev], [prev])[0]
            self.facts[node] = (prev, prev)
            self.empties.append(node)
        self.root = self.empties[height]

    def _children(self, node: int, level: int) -> Tuple[int, int]:
        """Children of `node`, which sits `level` levels above the leaves."""
        if node == self.empties[level]:
            e = self.empties[level - 1]
            return e, e
        return self.facts[node]

    def get(self, key: int) -> int:
        node = self.root
        for level in range(self.height, 0, -1):
            left, right = self._children(node, level)
            node = right if (key >> (level - 1)) & 1 else left
        return node

    def get_many(self, keys: Sequence[int]) -> List[int]:
        return [self.get(k) for k in keys]

    def update(self, modifications: Dict[int, int]) -> Tuple[int, int]:
        """Writes {leaf_index: value}; returns (old_root, new_root)."""
        old_root = self.root
        if not modifications:
            return old_root, old_root
        for k in modifications:
            assert 0 <= k < (1 << self.height)
        # top-down: current hashes of every node on a modified path, per level (level = height
        # above the leaves), keyed by node index within its level
        paths: List[Dict[int, int]] = [dict() for _ in range(self.height + 1)]
        paths[self.height][0] = self.root
        for level in range(self.height, 0, -1):
            wanted = sorted(set(k >> (level - 1) for k in modifications))
            for idx in wanted:
                parent = paths[level][idx >> 1]
                left, right = self._children(parent, level)
                paths[level - 1][idx] = right if idx & 1 else left
                sib = idx ^ 1
                if sib not in paths[level - 1]:
                    paths[level - 1][sib] = left if idx & 1 else right
        # bottom-up: new values
        layer = dict(modifications)
        for level in range(1, self.height + 1):
            parents = sorted(set(i >> 1 for i in layer))
            lefts = [layer.get(2 * i, paths[level - 1][2 * i]) for i in parents]
            rights = [layer.get(2 * i + 1, paths[level - 1][2 * i + 1]) for i in parents]
            hashes = self.hash_many(lefts, rights)
            for node, l, r in zip(hashes, lefts, rights):
                self.facts[node] = (l, r)
            layer = dict(zip(parents, hashes))
        self.root = layer[0]
        return old_root, self.root

    def witness(self, keys: Iterable[int]) -> List[Tuple[int, int, int, int, int]]:
        """The merkle_facts of the subtree induced by `keys` (sorted and made distinct first) in the tree as it stands:
        one (level, index, node, left, right) per inner node, level 1 (parents of leaves) up to the root, ascending
        index inside a level - what merkle_multi_update walks from this root (merkle_tree.py:4-26).  Read from the
        facts store by walking down from the root."""
        keys = sorted(set(keys))
        for k in keys:
            assert 0 <= k < (1 << self.height), "key out of range for height"
        if not keys:
            return []
        levels: List[List[Tuple[int, int, int, int, int]]] = [[] for _ in range(self.height + 1)]
        values = {0: self.root}
        for level in range(self.height, 0, -1):
            below = {}
            for idx in sorted(set(k >> level for k in keys)):
                left, right = self._children(values[idx], level)
                levels[level].append((level, idx, values[idx], left, right))
                below[2 * idx], below[2 * idx + 1] = left, right
            values = below
        return [rec for level in levels for rec in level]

    def prove(self, keys: Sequence[int]) -> List[Tuple[int, List[int]]]:
        """Inclusion proofs: per key (any order, repeats allowed) the leaf and its sibling path, siblings[l] at level l
        (0 = the leaf's own sibling ... height - 1 = the other child of the root)."""
        out = []
        for key in keys:
            assert 0 <= key < (1 << self.height), "key out of range for height"
            node, siblings = self.root, [0] * self.height
            for level in range(self.height, 0, -1):
                left, right = self._children(node, level)
                bit = (key >> (level - 1)) & 1
                node, siblings[level - 1] = (right, left) if bit else (left, right)
            out.append((node, siblings))
        return out

    def verify(self, keys: Sequence[int], proofs: Sequence[Tuple[int, Sequence[int]]]) -> List[bool]:
        """Checks inclusion proofs (the shape `prove` returns) against the tree's CURRENT root: True where the proof
        has this tree's height, its key and values are in range and it folds to the root.  One `hash_many` call per
        level over all proofs."""
        assert len(keys) == len(proofs)
        good = [i for i, (k, p) in enumerate(zip(keys, proofs)) if _proof_well_formed(self.height, k, p)]
        nodes = [proofs[i][0] for i in good]
        for level in range(self.height):
            sibs = [proofs[i][1][level] for i in good]
            bits = [(keys[i] >> level) & 1 for i in good]
            lefts = [s if b else n for n, s, b in zip(nodes, sibs, bits)]
            rights = [n if b else s for n, s, b in zip(nodes, sibs, bits)]
            nodes = list(self.hash_many(lefts, rights)) if good else []
        out = [False] * len(keys)
        for i, node in zip(good, nodes):
            out[i] = node == self.root
        return out

    def scan(self, lo: int = 0, hi: Optional[int] = None, capacity: Optional[int] = None):
        """Ordered range scan, the host twin of sp_tree_scan: the first `capacity` (None: all) keys k, lo <= k <= hi
        inclusive (hi None: the last key of the tree), whose leaf differs from the empty leaf, as [(key, leaf)] in
        ascending order, and `more`: whether further such keys exist in the range.  The same descent as the device's,
        through the facts store: the frontier of a level holds the nodes whose key interval meets [lo, hi] and whose
        VALUE differs from the level's empty-subtree root (a leaf set back to the empty leaf leaves nodes that exist
        but hold empty roots: they are pruned by value), cut after every step to its first capacity + 2 nodes above
        level 0 and to `capacity` keys at level 0.  The margin of two: a kept node has a live leaf below it, which is
        in range unless the node's interval sticks out of [lo, hi] - only the first node of a frontier (it holds lo)
        and the last (it holds hi) can - so a frontier that was cut, and thereby lost its last node, keeps at least
        capacity + 1 nodes with a leaf in range: the page is complete and a cut at any level means `more`.  No hash."""
        top = (1 << self.height) - 1
        hi = top if hi is None else hi
        assert 0 <= lo <= hi <= top, "scan range out of order or out of range for height"
        assert capacity is None or capacity >= 1, "capacity must be at least 1"
        more = False
        frontier = [(0, self.root)] if self.root != self.empties[self.height] else []
        for level in range(self.height, 0, -1):
            below = []
            for idx, node in frontier:
                for child, value in zip((2 * idx, 2 * idx + 1), self._children(node, level)):
                    first = child << (level - 1)
                    if value != self.empties[level - 1] and first <= hi and first | ((1 << (level - 1)) - 1) >= lo:
                        below.append((child, value))
            limit = None if capacity is None else capacity + 2 if level > 1 else capacity
            if limit is not None and len(below) > limit:
                more, below = True, below[:limit]
            frontier = below
        return frontier, more

    def items(self, lo: int = 0, hi: Optional[int] = None, page: int = 65536):
        """Generator over every (key, leaf) of `scan`'s range, one scan of `page` keys at a time."""
        return _scan_pages(self, lo, hi, page)

    def snapshot(self) -> dict:
        """Everything that defines the tree: {"height", "empty_leaf", "root", "keys", "leaves"} (lists of ints, the keys
        ascending).  `restore` rebuilds an equal tree from it."""
        pairs = list(self.items())
        return {"height": self.height, "empty_leaf": self.empties[0], "root": self.root,
                "keys": [k for k, _ in pairs], "leaves": [v for _, v in pairs]}

    @classmethod
    def restore(cls, snapshot: dict, hash_many=None, chunk: int = 1 << 18) -> "SparseMerkleTree":
        """A fresh tree holding the snapshot's leaves, written in ascending chunks; ValueError when the root that
        results is not the snapshot's."""
        tree = cls(int(snapshot["height"]), int(snapshot["empty_leaf"]), hash_many)
        keys, leaves = _snapshot_ints(snapshot)
        for at in range(0, len(keys), chunk):
            tree.update(dict(zip(keys[at:at + chunk], leaves[at:at + chunk])))
        if tree.root != int(snapshot["root"]):
            raise ValueError("the restored tree's root is not the snapshot's")
        return tree

    def clone(self) -> "SparseMerkleTree":
        """A second tree holding the same state, the host twin of sp_tree_clone: the facts store is copied, nothing is
        hashed, and updating either tree afterwards leaves the other untouched."""
        out = object.__new__(type(self))
        out.height, out.hash_many = self.height, self.hash_many
        out.facts, out.empties, out.root = dict(self.facts), list(self.empties), self.root
        return out

    def diff(self, other: "SparseMerkleTree", lo: int = 0, hi: Optional[int] = None, capacity: Optional[int] = None):
        """Ordered diff, the host twin of sp_tree_diff: the first `capacity` (None: all) keys k, lo <= k <= hi inclusive,
        whose leaf here differs from the leaf in `other` (same height and empty leaf), as [(key, leaf_self, leaf_other)]
        ascending, and `more`.  `scan`'s descent from the two roots through the two facts stores: the frontier of a level
        holds the nodes whose key interval meets [lo, hi] and whose VALUES differ - equal nodes are equal subtrees, a
        node that differs has a differing leaf below it - with the same cut (capacity + 2 above level 0, capacity at
        level 0, a cut at any level means `more`).  No hash."""
        assert self.height == other.height and self.empties[0] == other.empties[0], \
            "diff needs two trees of one height and one empty leaf"
        top = (1 << self.height) - 1
        hi = top if hi is None else hi
        assert 0 <= lo <= hi <= top, "diff range out of order or out of range for height"
        assert capacity is None or capacity >= 1, "capacity must be at least 1"
        more = False
        frontier = [(0, self.root, other.root)] if self.root != other.root else []
        for level in range(self.height, 0, -1):
            below = []
            for idx, mine, theirs in frontier:
                for child, a, b in zip((2 * idx, 2 * idx + 1), self._children(mine, level), other._children(theirs, level)):
                    first = child << (level - 1)
                    if a != b and first <= hi and first | ((1 << (level - 1)) - 1) >= lo:
                        below.append((child, a, b))
            limit = None if capacity is None else capacity + 2 if level > 1 else capacity
            if limit is not None and len(below) > limit:
                more, below = True, below[:limit]
            frontier = below
        return frontier, more

    def diff_items(self, other, lo: int = 0, hi: Optional[int] = None, page: int = 65536):
        """Generator over every (key, leaf_self, leaf_other) of `diff`'s range, one diff of `page` keys at a time."""
        return _diff_pages(self, other, lo, hi, page)

    def delta(self, base: "SparseMerkleTree", page: int = 1 << 18) -> dict:
        """What turns `base` into this tree: {"height", "empty_leaf", "base_root", "root", "keys", "leaves"} - the keys
        (ascending) where this tree differs from `base`, with THIS tree's leaves.  `base.apply_delta` of it reaches this
        tree's root: an incremental snapshot."""
        triples = list(self.diff_items(base, page=page))
        return {"height": self.height, "empty_leaf": self.empties[0], "base_root": base.root, "root": self.root,
                "keys": [k for k, _, _ in triples], "leaves": [v for _, v, _ in triples]}

    def apply_delta(self, delta: dict, chunk: int = 1 << 18):
        """Writes the leaves of a `delta` (of either tree class) in ascending chunks.  ValueError, with nothing written,
        when this tree's root is not the delta's base_root or its height or empty leaf differ; ValueError when the root
        that results is not delta["root"] - the tree then HOLDS the delta's leaves.  Returns (old_root, new_root)."""
        _check_delta(self, self.empties[0], delta)
        old_root = self.root
        keys, leaves = _snapshot_ints(delta)
        for at in range(0, len(keys), chunk):
            self.update(dict(zip(keys[at:at + chunk], leaves[at:at + chunk])))
        if self.root != int(delta["root"]):
            raise ValueError("the tree's root after the delta is not the delta's")
        return old_root, self.root


def _diff_pages(tree, other, lo, hi, page):
    """The pages of tree.diff(other, lo, hi, page) one after the other, as _scan_pages pages a scan."""
    while True:
        triples, more = tree.diff(other, lo, hi, page)
        yield from triples
        if not more:
            return
        lo = triples[-1][0] + 1


def _check_delta(tree, empty_leaf, delta):
    """What apply_delta checks BEFORE it writes: the delta was taken for a tree of this shape standing at this root."""
    if int(delta["height"]) != tree.height or int(delta["empty_leaf"]) != empty_leaf:
        raise ValueError("the delta was taken from a tree of another height or empty leaf")
    if tree.root != int(delta["base_root"]):
        raise ValueError("the tree's root is not the delta's base root")


def _scan_pages(tree, lo, hi, page):
    """The pages of tree.scan(lo, hi, page) one after the other: `more` says whether to go on, the next page starts
    behind the last key (which is below hi whenever more is set)."""
    while True:
        pairs, more = tree.scan(lo, hi, page)
        yield from pairs
        if not more:
            return
        lo = pairs[-1][0] + 1


def _snapshot_ints(snapshot):
    """(keys, leaves) of a snapshot as lists of ints, whichever class took it (arrays or lists)."""
    keys, leaves = snapshot["keys"], snapshot["leaves"]
    if hasattr(keys, "tolist"):
        keys = keys.tolist()
    if hasattr(leaves, "shape"):
        from . import batch_np
        leaves = batch_np.ints_from_felts(leaves) if len(keys) else []
    return [int(k) for k in keys], [int(v) for v in leaves]


def facts_of(witness) -> Dict[int, Tuple[int, int]]:
    """Witness records -> {node: (left, right)}: the shape of program_input['merkle_facts'] (main.cairo:39-40)."""
    return {node: (left, right) for _, _, node, left, right in witness}


def records_from_facts(facts, root: int, height: int, keys: Iterable[int]) -> List[Tuple[int, int, int, int, int]]:
    """The reference's dictionary {node: (left, right)} -> witness records of `keys` under `root`, in witness order
    (level 1 .. height, ascending index inside a level): the walk down from the root along the subtree induced by the
    keys (merkle_tree.py:4-26), nothing hashed.  KeyError: a preimage is missing."""
    keys = sorted(set(keys))
    for k in keys:
        assert 0 <= k < (1 << height), "key out of range for height"
    if not keys:
        return []
    levels: List[List[Tuple[int, int, int, int, int]]] = [[] for _ in range(height + 1)]
    values = {0: root}
    for level in range(height, 0, -1):
        below = {}
        for idx in sorted(set(k >> level for k in keys)):
            left, right = facts[values[idx]]
            levels[level].append((level, idx, values[idx], left, right))
            below[2 * idx], below[2 * idx + 1] = left, right
        values = below
    return [rec for level in levels for rec in level]


def _hash_records(records, hash_many):
    """(hashes, status) of H(left, right) per record, the status as the library reports it: HASH_OUT_OF_RANGE for a
    child outside [0, p) (nothing is hashed then), HASH_UNHASHABLE where the hash itself raises."""
    status = [batch.HASH_OK if 0 <= rec[3] < batch.FIELD_PRIME and 0 <= rec[4] < batch.FIELD_PRIME
              else batch.HASH_OUT_OF_RANGE for rec in records]
    todo = [u for u, st in enumerate(status) if st == batch.HASH_OK]
    hashes = [None] * len(records)
    try:
        done = hash_many([records[u][3] for u in todo], [records[u][4] for u in todo]) if todo else []
        for u, hv in zip(todo, done):
            hashes[u] = hv
    except AssertionError:  # "Unhashable input." somewhere in the batch: one by one, to know where
        for u in todo:
            try:
                hashes[u] = hash_many([records[u][3]], [records[u][4]])[0]
            except AssertionError:
                status[u] = batch.HASH_UNHASHABLE
    return hashes, status


def verify_update_records(height: int, keys: Sequence[int], prev_leaves: Sequence[int], new_leaves: Sequence[int],
                          prev_root: int, new_root: int, before, after, hash_many):
    """Host twin of sp_merkle_verify_update (include/starkperp.h), the same status bits computed in plain Python with
    every hash through `hash_many`: the statement of merkle_multi_update(prev_leaves, new_leaves, height, prev_root,
    new_root) (state/state.cairo:155-173) against the witness records `before` and `after` ((level, index, node, left,
    right) in witness order; level and index are NOT read - the positions follow from the strictly increasing `keys`
    alone, as in the library).  Returns (verdict, [status of the before records, status of the after records]): per
    record the OR of HASH_OUT_OF_RANGE / HASH_UNHASHABLE (from hashing left, right), WITNESS_HASH_MISMATCH (the hash has
    status 0 and is not the node), WITNESS_LINK_MISMATCH (a child on a key's path is not the node of the record below
    it in the same half - at level 1 not that key's leaf), WITNESS_SIBLING_CHANGED (a child on no key's path differs
    between the two records of the position; on both) and WITNESS_ROOT_MISMATCH (last record: the node is not the
    half's root).  The verdict is True iff every status is 0; without keys it is prev_root == new_root."""
    keys = list(keys)
    assert 1 <= height <= 64, "height must be in 1..64"
    assert all(0 <= k < (1 << height) for k in keys), "key out of range for height"
    assert all(a < b for a, b in zip(keys, keys[1:])), "keys must be strictly increasing"
    assert len(prev_leaves) == len(keys) and len(new_leaves) == len(keys)
    layout = [(level, idx) for level in range(1, height + 1) for idx in sorted({k >> level for k in keys})]
    records = len(layout)
    assert len(before) == records and len(after) == records, "n_records is not the witness size of the keys"
    if not keys:
        return prev_root == new_root, [[], []]
    place = {pos: u for u, pos in enumerate(layout)}
    leaf_at = {k: j for j, k in enumerate(keys)}
    halves, leaves, roots = (before, after), (prev_leaves, new_leaves), (prev_root, new_root)
    status = []
    for h in (0, 1):
        hashes, st = _hash_records(halves[h], hash_many)
        for u, (level, idx) in enumerate(layout):
            _, _, node, left, right = halves[h][u]
            if st[u] == batch.HASH_OK and hashes[u] != node:
                st[u] |= batch.WITNESS_HASH_MISMATCH
            for c, child in enumerate((left, right)):
                pos = (level - 1, 2 * idx + c)
                if level == 1 and pos[1] in leaf_at:
                    linked = child == leaves[h][leaf_at[pos[1]]]
                elif level > 1 and pos in place:
                    linked = child == halves[h][place[pos]][2]
                else:  # on no key's path: the same value before and after
                    linked = True
                    if before[u][3 + c] != after[u][3 + c]:
                        st[u] |= batch.WITNESS_SIBLING_CHANGED
                if not linked:
                    st[u] |= batch.WITNESS_LINK_MISMATCH
        if halves[h][-1][2] != roots[h]:
            st[-1] |= batch.WITNESS_ROOT_MISMATCH
        status.append(st)
    return not any(status[0]) and not any(status[1]), status


def _record_arrays(records):
    """Witness records (tuples of ints) -> the arrays batch_np.tree_witness returns."""
    import numpy as np
    from .batch_np import felts_from_ints
    felts = lambda i: felts_from_ints([rec[i] for rec in records]) if records else np.zeros((0, 4), dtype=np.uint64)
    return (np.array([rec[0] for rec in records], dtype=np.uint8), np.array([rec[1] for rec in records], dtype=np.uint64),
            felts(2), felts(3), felts(4))


def _verify_records(height, keys, prev_leaves, new_leaves, prev_root, new_root, before, after, hash_many) -> bool:
    """One verdict for records given as tuples: the host twin with an injected hash, else ONE library call."""
    if hash_many is not None:
        return verify_update_records(height, keys, prev_leaves, new_leaves, prev_root, new_root, before, after,
                                     hash_many)[0]
    import numpy as np
    from . import batch_np
    felts = lambda values: batch_np.felts_from_ints(values) if values else np.zeros((0, 4), dtype=np.uint64)
    return batch_np.merkle_verify_update(height, np.array(keys, dtype=np.uint64), felts(list(prev_leaves)),
                                         felts(list(new_leaves)), prev_root, new_root, _record_arrays(before),
                                         _record_arrays(after))[0]


def verify_multi_update(facts, height: int, prev_root: int, new_root: int, modifications, hash_many=None) -> bool:
    """The statement of merkle_multi_update (state/state.cairo:155-173) for modifications = {key: (prev_leaf,
    new_leaf)}: whether `facts` ({node: (left, right)}, program_input['merkle_facts']) carries a tree of root
    prev_root holding the previous leaves, a tree of root new_root holding the new ones, and nothing else differs
    between the two.  The records are read out of `facts` from both roots (records_from_facts: KeyError for a missing
    preimage) and checked in ONE library call (sp_merkle_verify_update: every record hashed once, no dependent chain);
    with an injected `hash_many` the host twin verify_update_records does the same."""
    keys = sorted(modifications)
    before = records_from_facts(facts, prev_root, height, keys)
    after = records_from_facts(facts, new_root, height, keys)
    return _verify_records(height, keys, [modifications[k][0] for k in keys], [modifications[k][1] for k in keys],
                           prev_root, new_root, before, after, hash_many)


def proof_root(key: int, leaf: int, siblings: Sequence[int], hash_many) -> int:
    """Folds an inclusion proof (SparseMerkleTree.prove / LibrarySparseTree.prove) to the root it commits to."""
    node = leaf
    for level, sib in enumerate(siblings):
        left, right = (sib, node) if (key >> level) & 1 else (node, sib)
        node = hash_many([left], [right])[0]
    return node


def proof_roots_many(keys: Sequence[int], proofs: Sequence[Tuple[int, Sequence[int]]]) -> List[int]:
    """[proof_root(key, leaf, siblings, ...)] for proofs of any lengths in ONE library call (sp_merkle_fold_paths):
    every path is folded on the device, the call lasting as long as its longest path."""
    return batch.merkle_fold_paths(list(keys), list(proofs))


def _proof_well_formed(height: int, key, proof) -> bool:
    """A proof that can belong to a tree of `height` at all: `height` siblings, the key inside the tree, every value
    a field element."""
    leaf, siblings = proof
    if len(siblings) != height or not 0 <= key < (1 << height):
        return False
    return all(0 <= v < batch.FIELD_PRIME for v in [leaf, *siblings])


class LibrarySparseTree:
    """The same tree with its state kept by the library (sp_tree_*, csrc/merkle.hip): one call per
    update instead of one host round trip per level - 4096 leaves at height 64 in about 15 ms
    instead of 270.  Same interface as SparseMerkleTree (`update`, `get`, `root`, `witness`, `prove`): the library
    stores nodes by position, not by hash, and `witness` reads the preimages of an induced subtree back by position
    (sp_tree_witness)."""

    def __init__(self, height: int, empty_leaf: int = 0, context: int = 0):
        """context: which device of sp_init_devices keeps the tree (0 = the primary; one process per GPU has only that)."""
        import ctypes
        from . import _lib
        self._lib, self._ct = _lib, ctypes
        self.height = height
        self.empty_leaf = empty_leaf
        self.context = context
        handle = ctypes.c_int()
        _lib.check(_lib.ensure_init().sp_tree_create_on(context, height, _lib.pack_felts([empty_leaf]),
                                                        ctypes.byref(handle)), "sp_tree_create_on")
        self._handle = handle.value

    @property
    def root(self) -> int:
        out = self._lib.new_felts(1)
        self._lib.check(self._lib.ensure_init().sp_tree_root(self._handle, out), "sp_tree_root")
        return self._lib.unpack_felts(out, 1)[0]

    def get(self, key: int) -> int:
        out = self._lib.new_felts(1)
        keys = (self._ct.c_uint64 * 1)(key)
        self._lib.check(self._lib.ensure_init().sp_tree_get(self._handle, keys, 1, out), "sp_tree_get")
        return self._lib.unpack_felts(out, 1)[0]

    def get_many(self, keys: Sequence[int]) -> List[int]:
        n = len(keys)
        if n == 0:
            return []
        out = self._lib.new_felts(n)
        arr = (self._ct.c_uint64 * n)(*keys)
        self._lib.check(self._lib.ensure_init().sp_tree_get(self._handle, arr, n, out), "sp_tree_get")
        return self._lib.unpack_felts(out, n)

    def update(self, modifications: Dict[int, int]) -> Tuple[int, int]:
        """Writes {leaf_index: value}; returns (old_root, new_root)."""
        items = sorted(dict(modifications).items())
        n = len(items)
        for k, v in items:
            assert 0 <= k < (1 << self.height) and 0 <= v < batch.FIELD_PRIME
        keys = (self._ct.c_uint64 * max(n, 1))(*[k for k, _ in items])
        old, new, st = self._lib.new_felts(1), self._lib.new_felts(1), self._lib.new_bytes(1)
        self._lib.check(self._lib.ensure_init().sp_tree_update(
            self._handle, keys, self._lib.pack_felts([v for _, v in items]), n, old, new, st), "sp_tree_update")
        if st[0]:
            raise AssertionError("Unhashable input." if st[0] & 2 else "leaf out of range")
        return self._lib.unpack_felts(old, 1)[0], self._lib.unpack_felts(new, 1)[0]

    def update_arrays(self, keys, leaves) -> Tuple[int, int]:
        """The same update from NumPy arrays: keys uint64[n] (any order, distinct), leaves uint64[n, 4]."""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        leaves = np.ascontiguousarray(leaves, dtype=np.uint64)
        assert keys.ndim == 1 and leaves.shape == (keys.shape[0], 4)
        order = np.argsort(keys, kind="stable")
        keys, leaves = np.ascontiguousarray(keys[order]), np.ascontiguousarray(leaves[order])
        old, new, st = self._lib.new_felts(1), self._lib.new_felts(1), self._lib.new_bytes(1)
        self._lib.check(self._lib.ensure_init().sp_tree_update(
            self._handle, keys.ctypes.data_as(self._ct.c_void_p), leaves.ctypes.data_as(self._ct.c_void_p),
            keys.shape[0], old, new, st), "sp_tree_update")
        if st[0]:
            raise AssertionError("Unhashable input." if st[0] & 2 else "leaf out of range")
        return self._lib.unpack_felts(old, 1)[0], self._lib.unpack_felts(new, 1)[0]

    def update_checked(self, modifications: Dict[int, int]) -> Tuple[int, int]:
        """`update` with its own audit: the witness of the keys before, the update, the witness after, and ONE
        sp_merkle_verify_update call on the two (previous leaves from sp_tree_get) - the statement of
        merkle_multi_update for exactly this batch.  Returns (old_root, new_root); AssertionError when the verdict is
        false (the update has been written by then)."""
        import numpy as np
        from . import batch_np
        items = sorted(dict(modifications).items())
        if not items:
            return self.update({})
        keys = np.array([k for k, _ in items], dtype=np.uint64)
        prev = batch_np.felts_from_ints(self.get_many([k for k, _ in items]))
        before = batch_np.tree_witness(self, keys)
        old_root, new_root = self.update(dict(items))
        after = batch_np.tree_witness(self, keys)
        ok, status = batch_np.merkle_verify_update(self.height, keys, prev, batch_np.felts_from_ints([v for _, v in items]),
                                                   old_root, new_root, before, after)
        assert ok, "the witnesses do not verify the update (status bits 0x%02x)" % int(np.bitwise_or.reduce(status, axis=None))
        return old_root, new_root

    def witness(self, keys: Iterable[int]) -> List[Tuple[int, int, int, int, int]]:
        """As SparseMerkleTree.witness, read from the library's node table in one call (sp_tree_witness)."""
        import numpy as np
        from . import batch_np
        keys = sorted(set(keys))
        for k in keys:
            assert 0 <= k < (1 << self.height), "key out of range for height"
        if not keys:
            return []
        level, index, node, left, right = batch_np.tree_witness(self, np.array(keys, dtype=np.uint64))
        return list(zip(level.tolist(), index.tolist(), batch_np.ints_from_felts(node), batch_np.ints_from_felts(left),
                        batch_np.ints_from_felts(right)))

    def prove(self, keys: Sequence[int]) -> List[Tuple[int, List[int]]]:
        """As SparseMerkleTree.prove, in one call (sp_tree_prove)."""
        import numpy as np
        from . import batch_np
        keys = list(keys)
        for k in keys:
            assert 0 <= k < (1 << self.height), "key out of range for height"
        if not keys:
            return []
        leaves, siblings = batch_np.tree_prove(self, np.array(keys, dtype=np.uint64))
        leaves, flat, h = batch_np.ints_from_felts(leaves), batch_np.ints_from_felts(siblings), self.height
        return [(leaf, flat[i * h:(i + 1) * h]) for i, leaf in enumerate(leaves)]

    def verify(self, keys: Sequence[int], proofs: Sequence[Tuple[int, Sequence[int]]]) -> List[bool]:
        """As SparseMerkleTree.verify, against the tree's current root (sp_tree_root), every well-formed proof folded
        and compared on the device in one call (sp_merkle_verify_paths): only the verdict bytes come back."""
        import numpy as np
        from . import batch_np
        assert len(keys) == len(proofs)
        good = [i for i, (k, p) in enumerate(zip(keys, proofs)) if _proof_well_formed(self.height, k, p)]
        out = [False] * len(keys)
        if not good:
            return out
        leaves = batch_np.felts_from_ints([proofs[i][0] for i in good])
        siblings = batch_np.felts_from_ints([v for i in good for v in proofs[i][1]])
        verdict, _ = batch_np.merkle_verify_paths(leaves, siblings, np.array([keys[i] for i in good], dtype=np.uint64),
                                                  batch_np.felts_from_ints([self.root]), height=self.height)
        for i, ok in zip(good, verdict.tolist()):
            out[i] = ok
        return out

    def scan(self, lo: int = 0, hi: Optional[int] = None, capacity: Optional[int] = None):
        """As SparseMerkleTree.scan, one page in one call (sp_tree_scan): ([(key, leaf)] ascending, more).  capacity
        None: the largest page of a call (batch_np.TREE_SCAN_MAX keys); `items` pages through any number."""
        from . import batch_np
        top = (1 << self.height) - 1
        hi = top if hi is None else hi
        assert 0 <= lo <= hi <= top, "scan range out of order or out of range for height"
        assert capacity is None or capacity >= 1, "capacity must be at least 1"
        keys, leaves, more = batch_np.tree_scan(self, lo, hi, batch_np.TREE_SCAN_MAX if capacity is None else capacity)
        return list(zip(keys.tolist(), batch_np.ints_from_felts(leaves))), more

    def items(self, lo: int = 0, hi: Optional[int] = None, page: int = 65536):
        """Generator over every (key, leaf) of `scan`'s range, one sp_tree_scan call of `page` keys at a time.  Each
        page describes a batch boundary (the tree's mutex); an update between two pages shows in the later ones."""
        return _scan_pages(self, lo, hi, page)

    def snapshot(self, page: int = 1 << 18) -> dict:
        """Everything that defines the tree: {"height", "empty_leaf", "root", "keys" uint64[n] ascending, "leaves"
        uint64[n, 4]}, read in pages of `page` keys.  The caller keeps updates away while it is taken; the root is read
        first and `restore` compares it, so a snapshot torn by an update does not restore."""
        import numpy as np
        from . import batch_np
        root, lo, top = self.root, 0, (1 << self.height) - 1
        keys, leaves = [np.zeros(0, dtype=np.uint64)], [np.zeros((0, 4), dtype=np.uint64)]
        while True:
            k, v, more = batch_np.tree_scan(self, lo, top, page)
            keys.append(k)
            leaves.append(v)
            if not more:
                break
            lo = int(k[-1]) + 1
        return {"height": self.height, "empty_leaf": self.empty_leaf, "root": root,
                "keys": np.concatenate(keys), "leaves": np.concatenate(leaves)}

    @classmethod
    def restore(cls, snapshot: dict, context: int = 0, chunk: int = 1 << 18) -> "LibrarySparseTree":
        """A fresh tree on `context` that holds the snapshot's leaves (of either tree class): the keys go to
        `update_arrays` in ascending chunks of `chunk`; ValueError, with the new tree closed, when the root that
        results is not the snapshot's.  Saving, moving to another context and compacting are all this."""
        import numpy as np
        from . import batch_np
        keys, leaves = snapshot["keys"], snapshot["leaves"]
        if not hasattr(leaves, "shape"):
            leaves = batch_np.felts_from_ints(leaves) if len(leaves) else np.zeros((0, 4), dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        tree = cls(int(snapshot["height"]), int(snapshot["empty_leaf"]), context)
        try:
            assert keys.ndim == 1 and leaves.shape == (keys.shape[0], 4) and (keys[1:] > keys[:-1]).all(), \
                "snapshot keys must be strictly increasing, one leaf each"
            for at in range(0, keys.shape[0], chunk):
                tree.update_arrays(keys[at:at + chunk], leaves[at:at + chunk])
            if tree.root != int(snapshot["root"]):
                raise ValueError("the restored tree's root is not the snapshot's")
        except BaseException:
            tree.close()
            raise
        return tree

    def compacted(self) -> "LibrarySparseTree":
        """A new tree with the same leaves and a table that holds only what they need (the table of a live tree only
        grows, and keeps the paths of leaves that were set back to the empty leaf)."""
        return self.restore(self.snapshot(), context=self.context)

    def clone(self) -> "LibrarySparseTree":
        """A second tree holding the same state on the same context (sp_tree_clone): one device copy of the node table,
        nothing hashed; updating or closing either tree afterwards leaves the other untouched.  A checkpoint to roll
        back to, a fork to try a batch on, a base to `diff` against."""
        from . import batch_np
        out = object.__new__(type(self))
        out._lib, out._ct = self._lib, self._ct
        out.height, out.empty_leaf, out.context = self.height, self.empty_leaf, self.context
        out._handle = None
        out._handle = batch_np.tree_clone(self)
        return out

    def diff(self, other: "LibrarySparseTree", lo: int = 0, hi: Optional[int] = None, capacity: Optional[int] = None):
        """As SparseMerkleTree.diff, one page in one call (sp_tree_diff): ([(key, leaf_self, leaf_other)] ascending,
        more).  capacity None: the largest page of a call (batch_np.TREE_DIFF_MAX keys); `diff_items` pages through any
        number.  The page is taken under both trees' mutexes: it describes a batch boundary of both."""
        from . import batch_np
        assert isinstance(other, LibrarySparseTree), "diff compares two trees the library keeps"
        top = (1 << self.height) - 1
        hi = top if hi is None else hi
        assert 0 <= lo <= hi <= top, "diff range out of order or out of range for height"
        assert capacity is None or capacity >= 1, "capacity must be at least 1"
        keys, mine, theirs, more = batch_np.tree_diff(self, other, lo, hi,
                                                      batch_np.TREE_DIFF_MAX if capacity is None else capacity)
        if not len(keys):
            return [], more
        return list(zip(keys.tolist(), batch_np.ints_from_felts(mine), batch_np.ints_from_felts(theirs))), more

    def diff_items(self, other, lo: int = 0, hi: Optional[int] = None, page: int = 65536):
        """Generator over every (key, leaf_self, leaf_other) of `diff`'s range, one sp_tree_diff call of `page` keys at
        a time; an update of either tree between two pages shows in the later ones."""
        return _diff_pages(self, other, lo, hi, page)

    def delta(self, base: "LibrarySparseTree", page: int = 1 << 18) -> dict:
        """What turns `base` into this tree: {"height", "empty_leaf", "base_root", "root", "keys" uint64[n] ascending,
        "leaves" uint64[n, 4]} - the keys where this tree differs from `base`, with THIS tree's leaves, read in pages of
        `page` keys.  An incremental snapshot: `base.apply_delta` of it reaches this tree's root.  The caller keeps
        updates away from both trees while it is taken; both roots are read first and `apply_delta` compares them."""
        import numpy as np
        from . import batch_np
        root, base_root, lo, top = self.root, base.root, 0, (1 << self.height) - 1
        keys, leaves = [np.zeros(0, dtype=np.uint64)], [np.zeros((0, 4), dtype=np.uint64)]
        while True:
            k, mine, _, more = batch_np.tree_diff(self, base, lo, top, page)
            keys.append(k)
            leaves.append(mine)
            if not more:
                break
            lo = int(k[-1]) + 1
        return {"height": self.height, "empty_leaf": self.empty_leaf, "base_root": base_root, "root": root,
                "keys": np.concatenate(keys), "leaves": np.concatenate(leaves)}

    def apply_delta(self, delta: dict, chunk: int = 1 << 18):
        """Writes the leaves of a `delta` (of either tree class) through `update_arrays` in ascending chunks of `chunk`.
        ValueError, with nothing written, when this tree's root is not the delta's base_root or its height or empty leaf
        differ; ValueError when the root that results is not delta["root"] - the tree then HOLDS the delta's leaves (a
        `clone` taken before is the way back).  Returns (old_root, new_root)."""
        import numpy as np
        from . import batch_np
        _check_delta(self, self.empty_leaf, delta)
        old_root = self.root
        keys, leaves = delta["keys"], delta["leaves"]
        if not hasattr(leaves, "shape"):
            leaves = batch_np.felts_from_ints(leaves) if len(leaves) else np.zeros((0, 4), dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert keys.ndim == 1 and leaves.shape == (keys.shape[0], 4) and (keys[1:] > keys[:-1]).all(), \
            "delta keys must be strictly increasing, one leaf each"
        for at in range(0, keys.shape[0], chunk):
            self.update_arrays(keys[at:at + chunk], leaves[at:at + chunk])
        new_root = self.root
        if new_root != int(delta["root"]):
            raise ValueError("the tree's root after the delta is not the delta's")
        return old_root, new_root

    @property
    def entries(self) -> int:
        """Slots of the node table in use (sp_tree_table_size): it never shrinks."""
        from . import batch_np
        return batch_np.tree_table_size(self)[0]

    def close(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            lib = self._lib.load()
            if lib.sp_is_initialised():  # after sp_shutdown the library has already dropped every tree
                self._lib.check(lib.sp_tree_destroy(handle), "sp_tree_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter teardown / library already gone
            pass


def hash_position_updates(updates: Sequence[Tuple[int, Position, Position]]):
    """position/hash.cairo:76-131: (key, prev_position, new_position) -> (key, prev_hash, new_hash);
    an unchanged position is hashed once."""
    changed = [i for i, u in enumerate(updates) if u[1] != u[2]]
    # previous and new leaves of all updates as one batch: one call, ragged when the asset counts differ
    both = position_hashes_many([u[1] for u in updates] + [updates[i][2] for i in changed])
    prev, new_h = both[: len(updates)], both[len(updates):]
    out = [(u[0], p, p) for u, p in zip(updates, prev)]
    for i, hnew in zip(changed, new_h):
        out[i] = (updates[i][0], prev[i], hnew)
    return out


def pack_state_batch(pos_updates: Sequence[Tuple[int, Position, Position]],
                     order_updates: Sequence[Tuple[int, int, int]]):
    """Squashed updates -> the arrays of batch_np.state_batch / sp_state_batch (pure host code, no GPU):
    pos_updates (key, previous Position, new Position) and order_updates (key, previous leaf, new leaf), both sorted
    by key (squash_updates).  Returns (pos_keys uint64[n_pos], prev_words uint64[*, 4], prev_off uint32[n_pos + 1],
    new_words uint64[*, 4], new_off uint32[n_pos + 1], ord_keys uint64[n_ord], ord_prev uint64[n_ord, 4], ord_new
    uint64[n_ord, 4]): the words of position_words chain after chain; an unchanged position (hash.cairo:76-131: it is
    hashed once) gives a new chain of length zero, new_off[i + 1] == new_off[i]."""
    import numpy as np
    from .batch_np import felts_from_ints
    n_pos = len(pos_updates)
    prev_flat, new_flat = [], []
    prev_off, new_off = np.zeros(n_pos + 1, dtype=np.uint32), np.zeros(n_pos + 1, dtype=np.uint32)
    for i, (_, prev, new) in enumerate(pos_updates):
        prev_flat.extend(position_words(prev))
        prev_off[i + 1] = len(prev_flat)
        if prev != new:
            new_flat.extend(position_words(new))
        new_off[i + 1] = len(new_flat)
    felts = lambda values: felts_from_ints(values) if values else np.zeros((0, 4), dtype=np.uint64)
    return (np.array([k for k, _, _ in pos_updates], dtype=np.uint64), felts(prev_flat), prev_off, felts(new_flat),
            new_off, np.array([k for k, _, _ in order_updates], dtype=np.uint64),
            felts([p for _, p, _ in order_updates]), felts([q for _, _, q in order_updates]))


# ---- the per-batch state-root update ------------------------------------------------------------
def squash_updates(accesses: Sequence[Tuple[int, object, object]]):
    """squash_dict semantics (state/state.cairo:67-96): a chronological list of
    (key, prev_value, new_value) accesses -> one (key, first_prev, last_new) per key, sorted by key;
    every access must continue from the previous value of its key."""
    first, last = {}, {}
    for key, prev, new in accesses:
        if key in last:
            assert last[key] == prev, "inconsistent dict access for key %d" % key
        else:
            first[key] = prev
        last[key] = new
    return [(k, first[k], last[k]) for k in sorted(first)]


class SharedState:
    """The two roots of services/perpetual/cairo/state/state.cairo:99-107 with their sparse trees
    (leaf of the positions tree = position_hash, empty leaf = hash of the empty position; leaf of
    the orders tree = fulfilled amount, empty leaf 0)."""

    EMPTY_POSITION: Position = (0, 0, ())

    def __init__(self, positions_tree_height: int = 64, orders_tree_height: int = 64, hash_many=None,
                 position_hashes=None):
        self._position_hashes = position_hashes or position_hashes_many
        self._hash_many = hash_many  # None: the library checks collected facts (check_facts), else the host twin does
        empty_leaf = self._position_hashes([self.EMPTY_POSITION])[0]
        if hash_many is None:  # the library keeps the trees: one call per update
            self.positions = LibrarySparseTree(positions_tree_height, empty_leaf)
            self.orders = LibrarySparseTree(orders_tree_height, 0)
        else:  # an injected hash (the oracle's, in CPU tests): host bookkeeping, hashes through it
            self.positions = SparseMerkleTree(positions_tree_height, empty_leaf, hash_many)
            self.orders = SparseMerkleTree(orders_tree_height, 0, hash_many)

    @property
    def positions_root(self) -> int:
        return self.positions.root

    @property
    def orders_root(self) -> int:
        return self.orders.root

    def apply_state_updates(self, position_accesses, order_accesses, facts=None, check_facts=False):
        """shared_state_apply_state_updates (state/state.cairo:135-186): squash, hash the previous
        and new positions (hash_position_updates), check the previous leaves against the tree,
        merkle-multi-update both trees.  Returns ((old_pos_root, new_pos_root), (old_ord, new_ord)).
        When the library keeps both trees and hashes the positions, all of it is ONE library call (sp_state_batch,
        _apply_in_one_call); with an injected hash the steps are separate calls (_apply_in_separate_calls).
        facts: a dict that receives the batch's merkle_facts (main.cairo:39-40, 61-64) for both trees - the witness
        of the squashed keys before the update and again after it, {node: (left, right)} - merged in only when the
        batch commits: a batch that raises leaves the dict as it was.  None: nothing is read back.
        check_facts (with facts): both trees' collected witnesses are verified against the batch's roots and the trees'
        leaves at the squashed keys before and after (the statement of merkle_multi_update, one
        sp_merkle_verify_update call per tree, or verify_update_records with an injected hash) BEFORE they are merged
        into the dict; AssertionError, with the dict as it was, when one does not verify."""
        if (isinstance(self.positions, LibrarySparseTree) and isinstance(self.orders, LibrarySparseTree)
                and self._position_hashes is position_hashes_many):
            apply = self._apply_in_one_call
        else:
            apply = self._apply_in_separate_calls
        if facts is None:
            assert not check_facts, "check_facts needs a facts dict"
            return apply(position_accesses, order_accesses)
        touched = [(self.positions, [key for key, _, _ in squash_updates(position_accesses)]),
                   (self.orders, [key for key, _, _ in squash_updates(order_accesses)])]
        collected: Dict[int, Tuple[int, int]] = {}
        prev_leaves = [tree.get_many(keys) if check_facts else None for tree, keys in touched]
        before = [tree.witness(keys) for tree, keys in touched]
        roots = apply(position_accesses, order_accesses)
        after = [tree.witness(keys) for tree, keys in touched]
        for (tree, keys), prev, wit_b, wit_a, (old_root, new_root) in zip(touched, prev_leaves, before, after, roots):
            if check_facts:
                assert _verify_records(tree.height, keys, prev, tree.get_many(keys), old_root, new_root, wit_b, wit_a,
                                       self._hash_many), "the collected merkle_facts do not verify the batch"
            collected.update(facts_of(wit_b))
            collected.update(facts_of(wit_a))
        facts.update(collected)
        return roots

    def _apply_in_one_call(self, position_accesses, order_accesses):
        """Through sp_state_batch: the previous-leaf checks, both trees' hashing and the all-or-nothing decision
        happen on the device; the status bytes are turned into the assertions of the separate-call route."""
        from . import batch_np
        pos = squash_updates(position_accesses)
        orders = squash_updates(order_accesses)
        for key, _, _ in pos:
            assert 0 <= key < (1 << self.positions.height)
        for key, _, new in orders:
            assert 0 <= key < (1 << self.orders.height) and 0 <= new < batch.FIELD_PRIME, \
                "order leaf out of range"
        # (a previous value that is no field element cannot be what a tree holds, nor be packed into a felt)
        assert all(0 <= prev < batch.FIELD_PRIME for _, prev, _ in orders), \
            "previous order state does not match the tree"
        pos_roots, ord_roots, pos_st, ord_st, batch_st = batch_np.state_batch(
            self.positions, self.orders, *pack_state_batch(pos, orders))
        if batch_st == 0:
            return pos_roots, ord_roots
        hashing = batch.HASH_OUT_OF_RANGE | batch.HASH_UNHASHABLE
        for code in pos_st:  # a position word out of range / an unhashable step: what the chain call raises
            if code & hashing:
                batch._raise_hash_status(batch.HASH_UNHASHABLE if code & batch.HASH_UNHASHABLE
                                         else batch.HASH_OUT_OF_RANGE)
        assert not any(code & batch_np.STATE_PREV_MISMATCH for code in pos_st), \
            "previous position does not match the tree"
        assert not any(code & batch_np.STATE_PREV_MISMATCH for code in ord_st), \
            "previous order state does not match the tree"
        assert not any(code & batch.HASH_OUT_OF_RANGE for code in ord_st), "order leaf out of range"
        # what is left was raised by the level hashing of one of the trees
        raise AssertionError("Unhashable input." if batch_st & batch.HASH_UNHASHABLE else "leaf out of range")

    def _apply_in_separate_calls(self, position_accesses, order_accesses):
        """The same step as separate calls: two position-hash calls, two previous-leaf reads, the two tree updates
        one after the other and a third update to roll the first back when the second fails."""
        # Every precondition first - the Cairo twin fails the whole batch, so nothing may be written
        # before both access lists have been squashed and checked against both trees.
        pos = squash_updates(position_accesses)
        orders = squash_updates(order_accesses)
        prev_h = self._position_hashes([p for _, p, _ in pos])
        changed = [i for i, (_, p, q) in enumerate(pos) if p != q]
        new_h = list(prev_h)
        for i, hv in zip(changed, self._position_hashes([pos[i][2] for i in changed])):
            new_h[i] = hv
        assert self.positions.get_many([key for key, _, _ in pos]) == list(prev_h), \
            "previous position does not match the tree"
        assert self.orders.get_many([key for key, _, _ in orders]) == [prev for _, prev, _ in orders], \
            "previous order state does not match the tree"
        for key, _, new in orders:
            assert 0 <= key < (1 << self.orders.height) and 0 <= new < batch.FIELD_PRIME, \
                "order leaf out of range"
        pos_roots = self.positions.update({k: hv for (k, _, _), hv in zip(pos, new_h)})
        try:
            ord_roots = self.orders.update({k: new for k, _, new in orders})
        except BaseException:
            # data-dependent failure inside the second update (an unhashable node): put the previous
            # position leaves back so that the two roots still describe one batch boundary
            self.positions.update({k: hv for (k, _, _), hv in zip(pos, prev_h)})
            raise
        return pos_roots, ord_roots

    def snapshot(self) -> dict:
        """{"positions": ..., "orders": ...}: the `snapshot` of both trees, taken between two batches."""
        return {"positions": self.positions.snapshot(), "orders": self.orders.snapshot()}

    @classmethod
    def restore(cls, snap: dict, hash_many=None, position_hashes=None, context: int = 0) -> "SharedState":
        """A state whose two trees are restored from `snap` (SharedState.snapshot of either route): library trees on
        `context` when hash_many is None, host twins on the injected hash otherwise.  ValueError when a tree does not
        come back to its snapshot's root; nothing is left open then."""
        out = cls(int(snap["positions"]["height"]), int(snap["orders"]["height"]), hash_many, position_hashes)
        out.close()  # the empty trees of __init__ give way to the restored ones
        trees = []
        try:
            for part in ("positions", "orders"):
                if hash_many is None:
                    trees.append(LibrarySparseTree.restore(snap[part], context=context))
                else:
                    trees.append(SparseMerkleTree.restore(snap[part], hash_many))
        except BaseException:
            for tree in trees:
                if hasattr(tree, "close"):
                    tree.close()
            raise
        out.positions, out.orders = trees
        return out

    def fork(self) -> "SharedState":
        """A second state standing where this one stands: both trees cloned (sp_tree_clone, or the host twins' stores
        copied), nothing mutable shared.  A batch tried on the fork leaves this state untouched."""
        out = object.__new__(type(self))
        out._position_hashes, out._hash_many = self._position_hashes, self._hash_many
        out.positions = self.positions.clone()
        try:
            out.orders = self.orders.clone()
        except BaseException:
            if hasattr(out.positions, "close"):
                out.positions.close()
            raise
        return out

    def delta(self, base: "SharedState") -> dict:
        """{"positions": ..., "orders": ...}: the `delta` of both trees against `base`'s, taken between two batches -
        what the batches since `base` changed, not what the trees hold."""
        return {"positions": self.positions.delta(base.positions), "orders": self.orders.delta(base.orders)}

    def apply_delta(self, d: dict):
        """Applies a `delta` (of either route) to both trees.  ValueError with NEITHER tree written when one of them does
        not stand at its delta's base root; then as the trees' apply_delta.  Returns ((old_pos_root, new_pos_root),
        (old_ord_root, new_ord_root))."""
        for tree, part in ((self.positions, "positions"), (self.orders, "orders")):
            _check_delta(tree, tree.empty_leaf if hasattr(tree, "empty_leaf") else tree.empties[0], d[part])
        return self.positions.apply_delta(d["positions"]), self.orders.apply_delta(d["orders"])

    def close(self):
        """Releases the library-side trees (no-op for the host-bookkeeping variant)."""
        for tree in (self.positions, self.orders):
            if hasattr(tree, "close"):
                tree.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
