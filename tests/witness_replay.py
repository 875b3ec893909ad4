"""Helpers shared by tests/test_tree_witness_cpu.py and tests/test_gpu_tree_witness.py: the consumer's side of a
witness.  Nothing here comes from the code under test or from the reference: replay_multi_update is the walk that
merkle_multi_update performs (state/state.cairo:155-173 over the induced subtree of merkle_tree.py:4-26), restated with
a dictionary of preimages as its only source of nodes."""
from oracle import cref

_memo = {}


def oracle_hash_many(xs, ys):
    """The C oracle's Pedersen hash over two lists; pairs seen before are served from a memo."""
    xs, ys = list(xs), list(ys)
    todo = sorted({p for p in zip(xs, ys) if p not in _memo})
    if todo:
        _memo.update(zip(todo, cref.opt_pedersen_hash_many([a for a, _ in todo], [b for _, b in todo])[0]))
    return [_memo[p] for p in zip(xs, ys)]


def oracle_hash(x, y):
    return oracle_hash_many([x], [y])[0]


def witness_size(height, keys):
    """The ten-line count: one record per distinct key >> level, levels 1 .. height."""
    return sum(len({k >> level for k in keys}) for level in range(1, height + 1))


def layout(height, keys):
    """Positions of the records, in order: level 1 .. height, ascending index inside a level."""
    return [(level, idx) for level in range(1, height + 1) for idx in sorted({k >> level for k in keys})]


def empties(height, empty_leaf):
    out = [empty_leaf]
    for _ in range(height):
        out.append(oracle_hash(out[-1], out[-1]))
    return out


def node_values(height, leaves, empty_leaf, positions):
    """{(level, index): value} for `positions` in the tree that holds `leaves` ({key: value}) and the empty leaf
    elsewhere, from scratch: a subtree without a written key is its level's empty root, anything else the hash of its
    two children."""
    emp = empties(height, empty_leaf)
    occupied = [set(k >> level for k in leaves) for level in range(height + 1)]
    memo = {}

    def value(level, idx):
        if idx not in occupied[level]:
            return emp[level]
        if level == 0:
            return leaves[idx]
        if (level, idx) not in memo:
            memo[(level, idx)] = oracle_hash(value(level - 1, 2 * idx), value(level - 1, 2 * idx + 1))
        return memo[(level, idx)]

    return {(level, idx): value(level, idx) for level, idx in positions}


def check_witness(height, leaves, empty_leaf, keys, witness):
    """A witness against the from-scratch tree: the layout order, every value, every record hashes."""
    keys = sorted(set(keys))
    assert [(rec[0], rec[1]) for rec in witness] == layout(height, keys)
    assert len(witness) == witness_size(height, keys)
    wanted = set()
    for level, idx in layout(height, keys):
        wanted |= {(level, idx), (level - 1, 2 * idx), (level - 1, 2 * idx + 1)}
    values = node_values(height, leaves, empty_leaf, wanted)
    for level, idx, node, left, right in witness:
        assert node == values[(level, idx)], (level, idx)
        assert left == values[(level - 1, 2 * idx)] and right == values[(level - 1, 2 * idx + 1)], (level, idx)
    hashed = oracle_hash_many([rec[3] for rec in witness], [rec[4] for rec in witness])
    assert hashed == [rec[2] for rec in witness]


def replay_multi_update(height, prev_root, new_root, modifications, preimage):
    """modifications {key: (previous leaf, new leaf)}.  Walks down from both roots through `preimage`
    ({node: (left, right)}) alone, along the subtree induced by the modified keys: a side without a modified key must
    be the same node in the old and in the new tree; the leaves reached must be the expected ones.  KeyError: a
    preimage is missing."""
    assert modifications

    def visit(level, idx, old, new, keys):
        if level == 0:
            assert keys == [idx]
            assert (old, new) == tuple(modifications[idx]), "leaf %d" % idx
            return
        old_left, old_right = preimage[old]
        new_left, new_right = preimage[new]
        left_keys = [k for k in keys if not (k >> (level - 1)) & 1]
        right_keys = [k for k in keys if (k >> (level - 1)) & 1]
        if left_keys:
            visit(level - 1, 2 * idx, old_left, new_left, left_keys)
        else:
            assert old_left == new_left, "untouched left side of (%d, %d) changed" % (level, idx)
        if right_keys:
            visit(level - 1, 2 * idx + 1, old_right, new_right, right_keys)
        else:
            assert old_right == new_right, "untouched right side of (%d, %d) changed" % (level, idx)

    for k in modifications:
        assert 0 <= k < (1 << height)
    visit(height, 0, prev_root, new_root, sorted(modifications))
