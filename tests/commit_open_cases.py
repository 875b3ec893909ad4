"""Cases of the opening call (sp_commit_open[_dev], csrc/commit_open.hpp) shared by tests/test_commit_open_cpu.py (the
shared header under g++, over host arrays) and tests/test_gpu_commit_open.py (the library, over device arrays).

Table contents are TAGS, nothing is hashed: every felt says where it sits, so a wrong index shows as a wrong tag.
    a value     (VALUE_TAG + t, column, row, 0)                    rows n_rows .. col_stride - 1 of a padded column carry
                                                                   PAD_TAG: nothing may ever read them
    a level     (LEVEL_TAG + t, flat index, level, index in level)
The expected arrays come from NumPy indexing with _path_indices of starkperp/stark.py restated here."""
import numpy as np

VALUE_TAG, LEVEL_TAG, PAD_TAG = 0x1000, 0x2000, 0x3000
SENTINEL = 0xA5A5A5A5A5A5A5A5
SLICE_MAX = 1 << 16  # csrc/commit_open.hpp OPEN_SLICE_MAX; both test files check it against the header's value
SP_OK, SP_ERR_BAD_ARGUMENT = 0, -3


def path_indices(n_leaves, idx):
    """starkperp/stark.py _path_indices: flat indices (leaves-first levels buffer) of the siblings of leaf idx."""
    out, off, width, i = [], 0, n_leaves, idx
    while width > 1:
        out.append(off + (i ^ 1))
        off += width
        width >>= 1
        i >>= 1
    return out


def table_arrays(t, n_rows, n_cols, col_stride):
    """(cols [n_cols * col_stride, 4], levels [2 n_rows - 1, 4]) of table t as uint64 tags."""
    cols = np.zeros((n_cols, col_stride, 4), dtype=np.uint64)
    cols[:, :, 0] = PAD_TAG + t
    cols[:, :n_rows, 0] = VALUE_TAG + t
    cols[:, :, 1] = np.arange(n_cols, dtype=np.uint64)[:, None]
    cols[:, :, 2] = np.arange(col_stride, dtype=np.uint64)[None, :]
    levels = np.zeros((2 * n_rows - 1, 4), dtype=np.uint64)
    levels[:, 0] = LEVEL_TAG + t
    levels[:, 1] = np.arange(2 * n_rows - 1, dtype=np.uint64)
    at, width, level = 0, n_rows, 0
    while width >= 1:
        levels[at : at + width, 2] = level
        levels[at : at + width, 3] = np.arange(width, dtype=np.uint64)
        at, width, level = at + width, width >> 1, level + 1
    return cols.reshape(n_cols * col_stride, 4), levels


class Case:
    """tables = [(n_rows, n_cols, col_stride)], picks = [(table, row)]; the arrays and the expected outputs."""

    def __init__(self, name, tables, picks):
        self.name, self.tables = name, tables
        self.n_open = len(picks)
        self.table_of = np.array([t for t, _ in picks], dtype=np.uint32)
        self.rows = np.array([r for _, r in picks], dtype=np.uint64)
        self.arrays = [table_arrays(t, *shape) for t, shape in enumerate(tables)]

    def expected(self):
        """(values, val_off, leaves, siblings, off): per table and per column / level one vectorised NumPy gather."""
        n = self.n_open
        heights = np.array([r.bit_length() - 1 for r, _, _ in self.tables] + [0], dtype=np.int64)
        widths = np.array([c for _, c, _ in self.tables] + [0], dtype=np.int64)
        val_off, off = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        val_off[1:] = np.cumsum(widths[self.table_of])
        off[1:] = np.cumsum(heights[self.table_of])
        values = np.zeros((int(val_off[-1]), 4), dtype=np.uint64)
        siblings = np.zeros((int(off[-1]), 4), dtype=np.uint64)
        leaves = np.zeros((n, 4), dtype=np.uint64)
        for t, (n_rows, n_cols, stride) in enumerate(self.tables):
            mine = np.nonzero(self.table_of == t)[0]
            if len(mine) == 0:
                continue
            rows = self.rows[mine].astype(np.int64)
            cols, levels = self.arrays[t]
            paths = np.array([path_indices(n_rows, r) for r in range(n_rows)], dtype=np.int64).reshape(n_rows, -1)
            for c in range(n_cols):
                values[val_off[mine].astype(np.int64) + c] = cols[c * stride + rows]
            leaves[mine] = levels[rows]
            for level in range(paths.shape[1]):
                siblings[off[mine].astype(np.int64) + level] = levels[paths[rows, level]]
        return values, val_off, leaves, siblings, off


def _spread(n_rows):
    """first, last and middle rows"""
    return sorted({0, n_rows - 1, n_rows // 2, n_rows // 3})


def cases():
    out = []
    # every table shape, alone: all its interesting rows, both strides
    for n_rows in (1, 2, 4, 64, 128):
        for n_cols in (1, 2, 5, 18):
            for pad in (0, 3):
                out.append(Case("one table %dx%d pad %d" % (n_rows, n_cols, pad), [(n_rows, n_cols, n_rows + pad)],
                                [(0, r) for r in _spread(n_rows)]))
    # more slots than a wave has lanes (70 values + the leaf + 2 siblings): a lane takes slot j and slot j + 64
    out.append(Case("one table 4x70: 73 slots", [(4, 70, 5)], [(0, r) for r in (3, 0, 2, 1)]))
    out.append(Case("one table 128x56: exactly 64 slots", [(128, 56, 128)], [(0, 127), (0, 77)]))
    three = [(64, 5, 67), (1, 2, 1), (128, 18, 128)]
    rows_of = lambda t, k: (k * 37 + t) % three[t][0]
    out.append(Case("two tables interleaved", three[:2], [(k % 2, rows_of(k % 2, k)) for k in range(9)]))
    out.append(Case("three tables interleaved", three, [(k % 3, rows_of(k % 3, k)) for k in range(17)]))
    out.append(Case("three tables, all picks from the last", three, [(2, rows_of(2, k)) for k in range(11)]))
    out.append(Case("three tables, all picks from the one-row table", three, [(1, 0)] * 5))
    out.append(Case("duplicates", three, [(0, 5), (0, 5), (2, 127), (0, 5), (2, 127), (1, 0), (1, 0)]))
    out.append(Case("reversed order", three, [(2, r) for r in range(127, -1, -1)] + [(0, r) for r in range(63, -1, -1)]))
    # n_open at the wave / block edges, and nothing at all
    for n in (0, 1, 63, 64, 65):
        out.append(Case("n_open %d" % n, three, [(k % 3, rows_of(k % 3, k)) for k in range(n)]))
    out.append(Case("no tables, no openings", [], []))
    # the slice class and its neighbours: the third is two launches
    small = [(128, 1, 131), (2, 2, 2)]
    for n in (SLICE_MAX - 1, SLICE_MAX, SLICE_MAX + 1):
        out.append(Case("n_open %d (slice class %+d)" % (n, n - SLICE_MAX), small,
                        [(int(k % 5 == 4), (k * 7 + 1) % small[int(k % 5 == 4)][0]) for k in range(n)]))
    return out


def slices_of(n_open):
    return -(-n_open // SLICE_MAX)


# ---- bad arguments ------------------------------------------------------------------------------------------------
# Each entry: (name, patch, word): `patch` edits the argument dict of a good base call, `word` is what the error text
# must name.  The argument dict (see base_args): n_tables, cols, col_stride, n_rows, n_cols, levels (lists, one entry per
# table; cols / levels hold pointers), n_open, table_of, rows (arrays), and null = the set of output names passed as NULL.
BASE_TABLES = [(64, 5, 67), (4, 1, 4)]
BASE_PICKS = [(0, 63), (1, 2), (0, 0)]


def _set(key, index, value):
    def patch(a):
        a[key] = list(a[key])
        a[key][index] = value
    return patch


def _null(name):
    return lambda a: a["null"].add(name)


def _no_tables(a):
    a["n_tables"] = 0


def _too_many_values(a):
    # two openings of a table of 2^31 columns: 2^32 value felts.  Nothing is dereferenced: the shapes fail first.
    a["n_cols"] = [1 << 31, 1]
    a["col_stride"] = [64, 4]
    a["table_of"] = np.array([0, 0], dtype=np.uint32)
    a["rows"] = np.array([0, 1], dtype=np.uint64)
    a["n_open"] = 2


def _too_many_siblings(a):
    # 2^27 openings of a table of 2^32 rows: 2^32 sibling felts.  The two arrays are zero pages that are only read.
    a["n_rows"] = [1 << 32, 4]
    a["col_stride"] = [1 << 32, 4]
    a["n_open"] = 1 << 27
    a["table_of"] = np.zeros(1 << 27, dtype=np.uint32)
    a["rows"] = np.zeros(1 << 27, dtype=np.uint64)


BAD = [
    ("n_tables == 0 with openings", _no_tables, "n_tables"),
    ("NULL cols pointer", _set("cols", 1, 0), "cols"),
    ("NULL levels pointer", _set("levels", 0, 0), "levels"),
    ("n_rows 0", _set("n_rows", 1, 0), "n_rows"),
    ("n_rows not a power of two", _set("n_rows", 1, 3), "n_rows"),
    ("n_rows above 2^32", _set("n_rows", 0, 1 << 33), "n_rows"),
    ("n_cols 0", _set("n_cols", 0, 0), "n_cols"),
    ("col_stride below n_rows", _set("col_stride", 0, 63), "col_stride"),
    ("table_of out of range", lambda a: a["table_of"].__setitem__(1, 2), "table_of"),
    ("row out of range", lambda a: a["rows"].__setitem__(0, 64), "rows"),
    ("row out of range in the small table", lambda a: a["rows"].__setitem__(1, 4), "rows"),
    ("more than 2^32 - 1 value felts", _too_many_values, "value felts"),
    ("more than 2^32 - 1 sibling felts", _too_many_siblings, "sibling felts"),
    ("NULL values", _null("values"), "values"),
    ("NULL val_off", _null("val_off"), "val_off"),
    ("NULL siblings", _null("siblings"), "siblings"),
    ("NULL off", _null("off"), "off"),
]


def base_args(col_ptrs, level_ptrs):
    """The good call the BAD patches start from; the caller supplies the table pointers (host or device)."""
    return {"n_tables": len(BASE_TABLES), "cols": list(col_ptrs), "levels": list(level_ptrs),
            "col_stride": [s for _, _, s in BASE_TABLES], "n_rows": [r for r, _, _ in BASE_TABLES],
            "n_cols": [c for _, c, _ in BASE_TABLES], "n_open": len(BASE_PICKS),
            "table_of": np.array([t for t, _ in BASE_PICKS], dtype=np.uint32),
            "rows": np.array([r for _, r in BASE_PICKS], dtype=np.uint64), "null": set()}


def all_sentinel(a):
    """whether every entry of `a` still holds the fill pattern of Outputs"""
    return bool((a == a.dtype.type(SENTINEL & ((1 << (8 * a.itemsize)) - 1))).all())


class Outputs:
    """Sentinel-filled outputs of a call with room for `n_values`, `n_open`, `n_siblings`; untouched() after a
    refused call."""

    def __init__(self, n_open, n_values, n_siblings):
        fill = lambda shape, dt: np.full(shape, dt(SENTINEL & ((1 << (8 * np.dtype(dt).itemsize)) - 1)), dtype=dt)
        self.values = fill((max(n_values, 1), 4), np.uint64)
        self.leaves = fill((max(n_open, 1), 4), np.uint64)
        self.siblings = fill((max(n_siblings, 1), 4), np.uint64)
        self.val_off = fill(n_open + 1, np.uint32)
        self.off = fill(n_open + 1, np.uint32)

    def untouched(self):
        return all(all_sentinel(a) for a in (self.values, self.leaves, self.siblings, self.val_off, self.off))
