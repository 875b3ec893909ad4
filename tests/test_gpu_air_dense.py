"""Dense parity of the other half of the prover - the witness generators, the composition kernels, the rc16 product column,
sp_felt_add_dev and the row-shard entry points of csrc/stark.hip and csrc/builtins.hip - with oracle/stark_ref.py at
every item count, size, shift, plan edge and argument edge of tests/air_cases.py (itself checked by
tests/test_air_cases_cpu.py).  Every comparison is equality of integers on whole arrays: no sampling, no tolerance."""
import functools
import random

import numpy as np
import pytest

import air_cases as cases
import transform_cases as tc
from oracle import ref_py as R
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
P = S.P
SP_OK, SP_ERR_BAD_ARGUMENT = 0, -3
MARKER = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def stark():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from starkperp import stark as st
    return st


def to_dev(ints):
    """Python ints -> int64[len, 4] on the device."""
    import torch
    return torch.from_numpy(tc.felts_from_ints(ints).view(np.int64)).cuda()


def cols_to_dev(cols):
    import torch
    return torch.stack([to_dev(c) for c in cols])


def to_host(t):
    return t.cpu().contiguous().numpy().view(np.uint64)


def marked(*shape):
    import torch
    return torch.full(shape, MARKER, dtype=torch.int64, device="cuda")


def assert_column(got, want_ints, what):
    """got: uint64[k, 4]; the message names where the first differing felt sits."""
    want = tc.felts_from_ints(want_ints)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d of %d felts differ, first at index %d: got %#x, want %#x" % (
        what, bad.size, len(want_ints), bad[0], tc.ints_from_felts(got[bad[0]:bad[0] + 1])[0], want_ints[bad[0]])


# ---- witness generators -----------------------------------------------------------------------------------------------------
def run_generator(stark, gen, items):
    if gen == "pedersen":
        return stark.pedersen_trace(to_dev([x for x, _ in items]), to_dev([y for _, y in items]))
    if gen == "ec_ladder":
        return stark.ec_ladder_trace(to_dev([m for m, _ in items]), to_dev([q[0] for _, q in items]),
                                     to_dev([q[1] for _, q in items]))
    return stark.ecdsa_trace(*(to_dev(v) for v in ([i[0] for i in items], [i[1] for i in items], [i[2] for i in items],
                                                   [i[3][0] for i in items], [i[3][1] for i in items])))


def assert_trace(gen, got, items):
    """Every cell of every column against the oracle; a failure names the column, the item, its row and its lane."""
    want = cases.oracle_trace(gen, items)
    rows = cases.ROWS[gen]
    got = to_host(got)
    assert got.shape == (len(want), rows * len(items), 4)
    for c, name in enumerate(cases.COLUMN_NAMES[gen]):
        want_c = tc.felts_from_ints(want[c])
        bad = np.flatnonzero((got[c] != want_c).any(axis=1))
        if bad.size:
            item, row = divmod(int(bad[0]), rows)
            pytest.fail("%s witness of %d items: column %s differs in %d cells, first at item %d (block %d, lane %d) row %d: "
                        "got %#x, want %#x" % (gen, len(items), name, bad.size, item, item // 64, item % 64, row,
                                               tc.ints_from_felts(got[c, bad[0]:bad[0] + 1])[0], want[c][bad[0]]))


@pytest.mark.parametrize("gen", sorted(cases.BATCHES))
def test_witness_calls_of_different_counts_back_to_back(stark, gen):
    """65, then 1, then 64 items on one stream with nothing between the calls: the scratch planes are [row][limb][item]
    with the item count as the stride, and the buffer of the first call is reused by the other two."""
    batch = cases.BATCHES[gen]()
    got = [run_generator(stark, gen, batch[:count]) for count in cases.REUSE_ORDER]
    for count, g in zip(cases.REUSE_ORDER, got):
        assert_trace(gen, g, batch[:count])


@pytest.mark.parametrize("count", cases.ITEM_COUNTS)
@pytest.mark.parametrize("gen", sorted(cases.BATCHES))
def test_witness_matches_oracle_cell_by_cell(stark, gen, count):
    """One lane, a full block, a block and one lane: the first `count` items of the edge batch, whose lanes 0, 63 and 64
    hold edge operands.  Of the Pedersen witness, row 511 of px is also the reference's hash of every pair."""
    items = cases.BATCHES[gen]()[:count]
    got = run_generator(stark, gen, items)
    assert_trace(gen, got, items)
    if gen == "pedersen" and count == cases.BATCH:
        px = tc.ints_from_felts(to_host(got[1, 511::512]))
        assert px == [R.pedersen_hash(x, y) for x, y in items]


def test_range_check_and_rc16_witness_edges(stark):
    """Both kernels run one row per lane: 11 values are five blocks and a half, 35 values one block and 24 rows.  The
    range-check kernel shifts across all four words, so 2^128, 2^192 + 5 and p - 1 have a trace as well (not a valid one)."""
    values = list(cases.range_check_batch())
    got = to_host(stark.range_check_trace(to_dev(values)))
    assert_column(got[0], S.range_check_trace(values)[0], "range_check witness")
    values = list(cases.rc16_batch())
    cols = stark.rc16_columns(to_dev(values))
    want = S.rc16_trace(values)
    for c, name in enumerate(("a", "acc", "s")):
        assert_column(to_host(cols[c]), want[c], "rc16 witness, column " + name)


# ---- compositions ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def periodic_tables(air, log_n, shift):
    """The library's periodic tables on the coset (device tensor) and the oracle's, compared once per (AIR, n, shift)."""
    from starkperp import stark as st
    n = 1 << log_n
    got = st.periodic_lde(n, shift, "cuda", air)
    want = cases.rc16_periodic_lde(log_n, shift) if air == "rc16" else S.periodic_lde(n, shift, air=air)
    for k, (g, w) in enumerate(zip(to_host(got), want)):
        assert_column(g, w, "periodic table %d of %s at log_n %d" % (k, air, log_n))
    return got, want


def composition_params(airs):
    return [pytest.param(air, log_n, shift, kind, id="%s-%d-%s-%s" % (air, log_n, name, kind))
            for air in airs for log_n in cases.COMPOSITION_LOG_N[air]
            for shift, name in zip(cases.SHIFTS, cases.SHIFT_IDS) for kind in cases.KINDS]


@pytest.mark.parametrize("air,log_n,shift,kind", composition_params(("pedersen", "ec_ladder", "ecdsa", "range_check")))
def test_composition_matches_oracle(stark, air, log_n, shift, kind):
    """The whole column at the smallest legal size (M = the periodic table's length), one size up, and where the table
    index wraps several times and the row index does not; the shift enters zinv[k] and the periodic tables."""
    n = 1 << log_n
    cols, alphas = cases.composition_inputs(air, log_n, kind)
    per, want_per = periodic_tables(air, log_n, shift)
    got = to_host(stark.air_eval(cols_to_dev(cols), per, n, alphas, shift, air))
    assert_column(got, S.composition_on_coset(cols, want_per, n, alphas, shift=shift, air=air),
                  "%s composition, log_n %d, shift %#x, %s columns" % (air, log_n, shift, kind))


@pytest.mark.parametrize("air,log_n,shift,kind", composition_params(("rc16",)))
def test_rc16_composition_matches_oracle(stark, air, log_n, shift, kind):
    """The kernel with the most uncarried subtractions feeding a multiply, on full-width columns (a, acc, s and p random or
    extreme felts, not 16-bit limbs) and on every corner of the limb range."""
    n = 1 << log_n
    cols, alphas, p, z = cases.composition_inputs(air, log_n, kind)
    per, _ = periodic_tables(air, log_n, shift)
    dev_cols, dev_p = cols_to_dev(cols), to_dev(p)
    for rc_min, rc_max in cases.RC16_LIMB_RANGES:
        got = to_host(stark.air_eval_rc16(dev_cols, dev_p, per, n, alphas, z, rc_min, rc_max, shift))
        assert_column(got, S.rc16_composition_on_coset(cols, p, n, alphas, z, rc_min, rc_max, shift=shift),
                      "rc16 composition, log_n %d, shift %#x, %s columns, limbs %d .. %d" % (log_n, shift, kind, rc_min, rc_max))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("n", cases.PRODUCT_LENGTHS)
def test_rc16_product_at_every_plan_edge(stark, n, kind):
    """One thread / one level of chunks / two levels, with and without a partial group of 16 and a partial chunk of 64
    (air_cases.product_plan), on full-width operands."""
    a, s, z = cases.product_inputs(n, kind)
    got = to_host(stark.rc16_product(to_dev(a), to_dev(s), z))
    assert_column(got, S.rc16_product_column(a, s, z), "rc16 product of %d cells, plan %s" % (n, cases.product_plan(n)))


@pytest.mark.parametrize("n", cases.FELT_ADD_LENGTHS)
def test_felt_add(stark, n):
    pairs = cases.felt_add_operands(n)
    got = to_host(stark.felt_add(to_dev([a for a, _ in pairs]), to_dev([b for _, b in pairs])))
    assert_column(got, [(a + b) % P for a, b in pairs], "felt_add of %d pairs" % n)


# ---- row shards -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sharded(stark):
    """The Pedersen composition of a real trace at log_n = 10: LDE, periodic tables, alphas, the whole column."""
    pairs = cases.pedersen_batch()[3:5]
    trace = stark.pedersen_trace(to_dev([x for x, _ in pairs]), to_dev([y for _, y in pairs]))
    n = trace.shape[1]
    assert n == 1 << cases.SHARD_LOG_N
    t_lde = stark.lde(trace)
    per, want_per = periodic_tables("pedersen", cases.SHARD_LOG_N, 3)
    alphas = cases.felts("random", 11, 77)
    whole = stark.air_eval(t_lde, per, n, alphas)
    lde_ints = [tc.ints_from_felts(c) for c in to_host(t_lde)]
    assert_column(to_host(whole), S.composition_on_coset(lde_ints, want_per, n, alphas), "composition of a real trace")
    return t_lde, per, alphas, whole


def eval_shard(stark, shard, col_stride, n_points, row0, per, alphas, out, log_n=cases.SHARD_LOG_N, shift=3):
    from starkperp import _lib
    lib = _lib.ensure_init()
    return lib.sp_air_eval_shard_dev(shard.data_ptr(), col_stride, n_points, row0, per.data_ptr(), log_n,
                                     _lib.pack_felts(alphas), _lib.pack_felts([shift]), out.data_ptr(), stark._stream())


def shard_of(t_lde, row0, n_points, extra=0):
    """Rows row0 .. row0 + n_points of every column and the four rows behind them (the last shard's halo is rows 0 .. 3),
    `extra` marker rows after that: [4, n_points + 4 + extra, 4]."""
    import torch
    big = t_lde.shape[1]
    idx = (torch.arange(n_points + 4, device="cuda") + row0) % big
    shard = marked(4, n_points + 4 + extra, 4)
    shard[:, : n_points + 4] = t_lde[:, idx]
    return shard


@pytest.mark.parametrize("world", cases.SHARD_WORLDS)
def test_composition_row_shards_reassemble(stark, sharded, world):
    import torch
    t_lde, per, alphas, whole = sharded
    big = t_lde.shape[1]
    size = big // world
    got = marked(big, 4)
    for rank in range(world):
        shard = shard_of(t_lde, rank * size, size)
        rc = eval_shard(stark, shard, size + 4, size, rank * size, per, alphas, got[rank * size:])
        assert rc == SP_OK, (world, rank)
    differ = [rank for rank in range(world) if not torch.equal(got[rank * size:(rank + 1) * size], whole[rank * size:(rank + 1) * size])]
    assert not differ, "world %d: shards %s differ from the whole column" % (world, differ)


def test_composition_row_shard_with_a_wider_column_stride(stark, sharded):
    import torch
    t_lde, per, alphas, whole = sharded
    size = t_lde.shape[1] // 2
    shard = shard_of(t_lde, size, size, extra=7)
    out = marked(size + 1, 4)
    assert eval_shard(stark, shard, size + 11, size, size, per, alphas, out) == SP_OK
    assert torch.equal(out[:size], whole[size:]) and (out[size] == MARKER).all().item()


def test_composition_row_shard_arguments(stark, sharded):
    from starkperp import _lib
    t_lde, per, alphas, _ = sharded
    big = t_lde.shape[1]
    size = big // 2
    shard = shard_of(t_lde, 0, size)
    out = marked(size, 4)
    refused = {"row0 = 2": (size + 4, size, 2), "col_stride = n_points + 3": (size + 3, size, 0),
               "row0 + n_points = 4n + 4": (size + 4, size, big + 4 - size)}
    for what, (col_stride, n_points, row0) in refused.items():
        assert eval_shard(stark, shard, col_stride, n_points, row0, per, alphas, out) == SP_ERR_BAD_ARGUMENT, what
        assert "shard" in _lib.last_error(), what
    for log_n in cases.REFUSED_LOG_N["pedersen"]:
        assert eval_shard(stark, shard, size + 4, size, 0, per, alphas, out, log_n=log_n) == SP_ERR_BAD_ARGUMENT, log_n
        assert "sp_air_eval_shard_dev" in _lib.last_error() and "log_n" in _lib.last_error()
    for shift in cases.REFUSED_SHIFTS:
        assert eval_shard(stark, shard, size + 4, size, 0, per, alphas, out, shift=shift) == SP_ERR_BAD_ARGUMENT, shift
        assert "sp_air_eval_shard_dev" in _lib.last_error() and "shift" in _lib.last_error()
    # an empty shard is no launch at all
    assert eval_shard(stark, shard, size + 4, 0, 0, per, alphas, out) == SP_OK
    assert (out == MARKER).all().item()


def fold_shards(stark, t, log_m, shards, beta, shift):
    """sp_fri_fold_shard_dev on `shards` contiguous shards of the lower half -> (the reassembled fold, return codes)."""
    from starkperp import _lib
    lib = _lib.ensure_init()
    half = 1 << (log_m - 1)
    count = half // shards
    out = marked(half, 4)
    codes = []
    for k in range(shards):
        i0 = k * count
        codes.append(lib.sp_fri_fold_shard_dev(t[i0:].data_ptr(), t[half + i0:].data_ptr(), out[i0:].data_ptr(), log_m, i0, count,
                                               _lib.pack_felts([beta]), _lib.pack_felts([shift]), stark._stream()))
    return out, codes


@pytest.mark.parametrize("kind", cases.KINDS)
def test_fold_row_shards_reassemble(stark, kind):
    """Every shard but the first has i0 > 0: the twiddle index is (i0 + i) << (log_tw - log_m).  Once with whatever inverse
    twiddle table the process holds, once after a fold of 2^14 points has made it at least four times the layer's."""
    from starkperp import _lib
    log_m = cases.FOLD_SHARD_LOG_M
    half = 1 << (log_m - 1)
    layer = cases.felts(kind, 1 << log_m, 1212)
    beta, shift = cases.felts(kind, 1, 1213)[0], cases.RANDOM_SHIFT
    want = S.fri_fold(layer, beta, shift)
    t = to_dev(layer)

    def check(when):
        for shards in cases.FOLD_SHARDS:
            out, codes = fold_shards(stark, t, log_m, shards, beta, shift)
            assert codes == [SP_OK] * shards
            got, count = to_host(out), half // shards
            want_arr = tc.felts_from_ints(want)
            differ = [k for k in range(shards) if not np.array_equal(got[k * count:(k + 1) * count], want_arr[k * count:(k + 1) * count])]
            assert not differ, "%s, %d shards of %d: shards %s differ from the oracle's fold" % (when, shards, count, differ)

    check("before the larger table")
    big = cases.felts(kind, 1 << cases.FOLD_TABLE_LOG, 1414)
    assert_column(to_host(stark.fri_fold(to_dev(big), beta, 3)), S.fri_fold(big, beta, 3), "fold of 2^14 points")
    check("after a fold of 2^14 points")
    # one past the half is refused, as is a shift of 0
    lib = _lib.ensure_init()
    out = marked(half, 4)
    count = half // 4
    args = (t.data_ptr(), t[half:].data_ptr(), out.data_ptr(), log_m)
    assert lib.sp_fri_fold_shard_dev(*args, half - count + 1, count, _lib.pack_felts([beta]), _lib.pack_felts([shift]),
                                     stark._stream()) == SP_ERR_BAD_ARGUMENT
    assert lib.sp_fri_fold_shard_dev(*args, 0, count, _lib.pack_felts([beta]), _lib.pack_felts([0]),
                                     stark._stream()) == SP_ERR_BAD_ARGUMENT
    assert "shift" in _lib.last_error()
    assert lib.sp_fri_fold_dev(t.data_ptr(), out.data_ptr(), log_m, _lib.pack_felts([beta]), _lib.pack_felts([0]),
                               stark._stream()) == SP_ERR_BAD_ARGUMENT
    assert (out == MARKER).all().item()


# ---- argument edges -----------------------------------------------------------------------------------------------------------
# Every call below is refused on the host before anything is launched (csrc/stark.hip air_log_n_ok and air_zinv, the range
# checks at the head of sp_air_eval_rc16_dev): a log_n of 31 that reached a launch would read far outside these buffers.
def composition_call(stark, air, log_n, shift, buf, out):
    """The composition entry point of `air` on marked buffers that a refused call never touches -> return code."""
    from starkperp import _lib
    lib = _lib.ensure_init()
    alphas, sh = _lib.pack_felts(cases.felts("random", cases.N_ALPHAS[air], 5)), _lib.pack_felts([shift])
    if air == "rc16":
        return lib.sp_air_eval_rc16_dev(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), log_n, alphas, sh, _lib.pack_felts([7]),
                                        0, 0xFFFF, out.data_ptr(), stark._stream())
    return getattr(lib, stark.AIRS[air]["eval"])(buf.data_ptr(), buf.data_ptr(), log_n, alphas, sh, out.data_ptr(),
                                                 stark._stream())


@pytest.mark.parametrize("air", sorted(cases.COMPOSITION_LOG_N))
def test_composition_calls_refuse_bad_sizes_and_shifts(stark, air):
    from starkperp import _lib
    # as large as the largest legal call below would read (ecdsa at log_n 10: ten columns of 2^12 felts, twelve tables of 2^12)
    buf, out = marked(1 << 16, 4), marked(1 << 12, 4)
    name = "sp_air_eval_rc16_dev" if air == "rc16" else stark.AIRS[air]["eval"]
    for log_n in cases.REFUSED_LOG_N[air]:       # one below the AIR's period, and 31
        assert composition_call(stark, air, log_n, 3, buf, out) == SP_ERR_BAD_ARGUMENT, log_n
        assert name in _lib.last_error() and "log_n" in _lib.last_error(), _lib.last_error()
    smallest = cases.COMPOSITION_LOG_N[air][0]
    for log_n in (smallest, max(smallest, 9)):
        refused = cases.REFUSED_SHIFTS + (S.root_of_unity(log_n + 2),)     # 0, 1, p - 1 and w_4n itself
        for shift in refused:
            assert 0 in cases.denominators(shift, log_n) or shift == 0
            assert composition_call(stark, air, log_n, shift, buf, out) == SP_ERR_BAD_ARGUMENT, (log_n, hex(shift))
            assert name in _lib.last_error() and "shift" in _lib.last_error(), _lib.last_error()
    assert (out == MARKER).all().item() and (buf == MARKER).all().item()


def test_blocks_call_refuses_bad_sizes(stark):
    from starkperp import _lib
    lib = _lib.ensure_init()
    buf = marked(16, 4)
    alphas, sh = _lib.pack_felts(cases.felts("random", 11, 5)), _lib.pack_felts([3])
    for log_n in cases.REFUSED_LOG_N["pedersen"]:
        rc = lib.sp_air_eval_blocks_dev(buf.data_ptr(), 8, 1, 2, 1, 0, buf.data_ptr(), log_n, alphas, sh, buf.data_ptr(),
                                        stark._stream())
        assert rc == SP_ERR_BAD_ARGUMENT and "log_n" in _lib.last_error()
    assert (buf == MARKER).all().item()


def test_empty_witness_calls_are_no_launch(stark):
    import torch
    from starkperp import _lib
    lib = _lib.ensure_init()
    buf, out = marked(4, 4), marked(16, 4)
    p, st = buf.data_ptr(), stark._stream()
    assert lib.sp_pedersen_trace_dev(p, p, 0, out.data_ptr(), st) == SP_OK
    assert lib.sp_ec_ladder_trace_dev(p, p, p, 0, out.data_ptr(), st) == SP_OK
    assert lib.sp_ecdsa_trace_dev(p, p, p, p, p, 0, out.data_ptr(), st) == SP_OK
    assert lib.sp_range_check_trace_dev(p, 0, out.data_ptr(), st) == SP_OK
    assert lib.sp_rc16_trace_dev(p, 0, out.data_ptr(), st) == SP_OK
    torch.cuda.synchronize()
    assert (out == MARKER).all().item() and (buf == MARKER).all().item()
    # and the library is still usable: a launch error would have stayed with the stream
    x, y = cases.pedersen_batch()[0]
    assert_trace("pedersen", stark.pedersen_trace(to_dev([x]), to_dev([y])), [(x, y)])
