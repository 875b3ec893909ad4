"""Prover-side pipeline on device-resident columns: trace -> coset LDE -> commit -> AIR composition
-> commit -> FRI folds with per-layer commits.  Build-defined (the reference has no prover); every
commitment hash is the reference's pedersen_hash.  Columns live in HBM as torch int64 [n, 4]
tensors (four little-endian 64-bit limbs per felt); torch is only the allocator / stream owner."""
from typing import List, Tuple

from . import _lib
from ._lib import pack_felts

FIELD_PRIME = 2**251 + 17 * 2**192 + 1
FIELD_GEN = 3
BLOWUP_LOG = 2
N_CONSTRAINTS = 11
SHIFT_POINT = (
    0x49EE3EBA8C1600700EE1B87EB599F16716B0B1022947733551FDE4050CA6804,
    0x3CA0CFE4B3BC6DDF346D49D06EA0ED34E621062C0E056C1D0405D266E10268A,
)
EC_GEN = (
    0x1EF15C18599971B7BECED415A40F0C7DEACFD9B0D1819E03D723D8BC943CFCA,
    0x5668060AA49730B7BE4801DF46EC62DE53ECD11ABE43A32873000C36E8DC1F,
)


def _torch():
    import torch
    return torch


def felts_to_tensor(values, device="cuda"):
    torch = _torch()
    import numpy as np
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    arr = np.frombuffer(raw, dtype="<i8").reshape(len(values), 4).copy()
    return torch.from_numpy(arr).to(device)


def tensor_to_felts(t):
    raw = t.detach().cpu().contiguous().numpy().astype("<i8").tobytes()
    return [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(len(raw) // 32)]


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def ntt(col, inverse=False):
    """Natural-order NTT of a [n, 4] column (n a power of two)."""
    torch = _torch()
    lib = _lib.ensure_init()
    n = col.shape[0]
    out = torch.empty_like(col)
    _lib.check(lib.sp_ntt_dev(col.data_ptr(), out.data_ptr(), n.bit_length() - 1, 1 if inverse else 0,
                              _stream()), "sp_ntt_dev")
    return out


def lde(cols, blowup_log=BLOWUP_LOG, shift=FIELD_GEN):
    """cols: [ncols, n, 4] -> [ncols, n << blowup_log, 4] on the coset shift * <w>."""
    torch = _torch()
    lib = _lib.ensure_init()
    ncols, n = cols.shape[0], cols.shape[1]
    out = torch.empty((ncols, n << blowup_log, 4), dtype=torch.int64, device=cols.device)
    _lib.check(lib.sp_lde_dev(cols.data_ptr(), out.data_ptr(), ncols, n.bit_length() - 1, blowup_log,
                              pack_felts([shift]), _stream()), "sp_lde_dev")
    return out


def pedersen_trace(xs, ys):
    """xs, ys: [m, 4] device tensors of hash inputs -> [4, 512 m, 4] trace (s, px, py, lambda)."""
    torch = _torch()
    lib = _lib.ensure_init()
    m = xs.shape[0]
    cols = torch.empty((4, 512 * m, 4), dtype=torch.int64, device=xs.device)
    _lib.check(lib.sp_pedersen_trace_dev(xs.data_ptr(), ys.data_ptr(), m, cols.data_ptr(), _stream()),
               "sp_pedersen_trace_dev")
    return cols


def periodic_columns():
    """The six period-512 columns of the AIR (constant points and selectors) as Python ints; the
    per-bit constant points come from starkperp.signature.CONSTANT_POINTS."""
    from .signature import CONSTANT_POINTS
    cx, cy, step, mid, end, z252 = [], [], [], [], [], []
    for r in range(512):
        block, j = divmod(r, 256)
        c = CONSTANT_POINTS[2 + 252 * block + j] if j < 252 else EC_GEN
        cx.append(c[0])
        cy.append(c[1])
        step.append(0 if j == 255 else 1)
        mid.append(1 if r == 255 else 0)
        end.append(1 if r == 511 else 0)
        z252.append(1 if j == 252 else 0)
    return [cx, cy, step, mid, end, z252]


def ec_ladder_periodic_columns():
    """Period-256 selectors of the EC-ladder AIR: step (rows 0..254), first (row 0), z251."""
    return [[0 if j == 255 else 1 for j in range(256)], [1 if j == 0 else 0 for j in range(256)],
            [1 if j == 251 else 0 for j in range(256)]]


def ecdsa_periodic_columns():
    """Period-1024 tables of the ECDSA-verification AIR (oracle/stark_ref.py ecdsa_periodic_columns is the
    definition): step, first, start_y, z251, gbase, oncurve, carry_load, carry_hold, addb, rload, rhold, fin."""
    def rows(fn):
        return [1 if fn(i) else 0 for i in range(1024)]
    ladder = lambda i: i < 768
    start_y = [0] * 1024
    start_y[0], start_y[256], start_y[512] = FIELD_PRIME - SHIFT_POINT[1], SHIFT_POINT[1], SHIFT_POINT[1]
    return [rows(lambda i: ladder(i) and i % 256 != 255), rows(lambda i: ladder(i) and i % 256 == 0), start_y,
            rows(lambda i: ladder(i) and i % 256 == 251), rows(lambda i: i == 0), rows(lambda i: i == 256),
            rows(lambda i: i == 255), rows(lambda i: 256 <= i < 511), rows(lambda i: i == 511),
            rows(lambda i: i == 256), rows(lambda i: 256 <= i < 767), rows(lambda i: i == 767)]


def range_check_periodic_columns():
    """step (rows 0..126 of every 128), last (row 127): oracle/stark_ref.py range_check_periodic_columns."""
    return [[1] * 127 + [0], [0] * 127 + [1]]


N_RANGE_CHECK_CONSTRAINTS = 2
RANGE_CHECK_BITS = 128
N_EC_LADDER_CONSTRAINTS = 12
N_ECDSA_CONSTRAINTS = 26
EC_ORDER = 0x800000000000010FFFFFFFFFFFFFFFFB781126DCAE7B2321E66A241ADC64D2F
AIRS = {
    "ecdsa": {"n_cols": 10, "period": 1024, "n_constraints": N_ECDSA_CONSTRAINTS, "periodic": ecdsa_periodic_columns,
              "eval": "sp_air_eval_ecdsa_dev"},
    "pedersen": {"n_cols": 4, "period": 512, "n_constraints": N_CONSTRAINTS, "periodic": periodic_columns,
                 "eval": "sp_air_eval_dev"},
    "ec_ladder": {"n_cols": 7, "period": 256, "n_constraints": N_EC_LADDER_CONSTRAINTS,
                  "periodic": ec_ladder_periodic_columns, "eval": "sp_air_eval_ec_ladder_dev"},
    "range_check": {"n_cols": 1, "period": 128, "n_constraints": N_RANGE_CHECK_CONSTRAINTS,
                    "periodic": range_check_periodic_columns, "eval": "sp_air_eval_range_check_dev"},
}


def rc16_periodic_columns():
    """first8 (limb 0 of a value), step8 (the next row belongs to the same value): oracle/stark_ref.py rc16."""
    return [[1, 0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0]]


N_RC16_CONSTRAINTS = 8
RC16_LIMBS = 8
AIRS["rc16"] = {"n_cols": 3, "period": 8, "n_constraints": N_RC16_CONSTRAINTS, "periodic": rc16_periodic_columns,
                "eval": None}  # evaluated by air_eval_rc16 (it needs the second-phase column and the challenge z)
BUILTIN_SEGMENTS = ["pedersen", "ecdsa", "rc16"]  # column order of a combined builtin trace


def periodic_lde(n, shift=FIELD_GEN, device="cuda", air="pedersen"):
    """[k, 4 * period, 4]: the periodic columns on the LDE coset (they repeat with period 4 * period)."""
    torch = _torch()
    spec = AIRS[air]
    cols = torch.stack([felts_to_tensor(c, device) for c in spec["periodic"]()])
    return lde(cols, BLOWUP_LOG, pow(shift, n // spec["period"], FIELD_PRIME))


def air_eval(trace_lde, per_lde, n, alphas, shift=FIELD_GEN, air="pedersen"):
    torch = _torch()
    lib = _lib.ensure_init()
    spec = AIRS[air]
    assert len(alphas) == spec["n_constraints"] and trace_lde.shape[0] == spec["n_cols"]
    assert trace_lde.shape[1] == 4 * n
    out = torch.empty((4 * n, 4), dtype=torch.int64, device=trace_lde.device)
    _lib.check(getattr(lib, spec["eval"])(trace_lde.data_ptr(), per_lde.data_ptr(), n.bit_length() - 1,
                                          pack_felts(alphas), pack_felts([shift]), out.data_ptr(), _stream()),
               spec["eval"])
    return out


def ec_ladder_trace(ms, qxs, qys):
    """ms, qxs, qys: [k, 4] device tensors (scalars 0 < m < 2^251, affine base points) ->
    [7, 256 k, 4] witness of k mimic_ec_mult_air ladders (m, px, py, qx, qy, la, ld)."""
    torch = _torch()
    lib = _lib.ensure_init()
    k = ms.shape[0]
    cols = torch.empty((7, 256 * k, 4), dtype=torch.int64, device=ms.device)
    _lib.check(lib.sp_ec_ladder_trace_dev(ms.data_ptr(), qxs.data_ptr(), qys.data_ptr(), k, cols.data_ptr(),
                                          _stream()), "sp_ec_ladder_trace_dev")
    return cols


def ecdsa_trace(zs, rs, ws, qxs, qys):
    """zs, rs, ws, qxs, qys: [k, 4] device tensors (message hashes, r, w = s^-1 mod N, public key points) of
    signatures verify() accepts -> [10, 1024 k, 4] witness of the ECDSA-verification AIR."""
    torch = _torch()
    lib = _lib.ensure_init()
    k = zs.shape[0]
    cols = torch.empty((10, 1024 * k, 4), dtype=torch.int64, device=zs.device)
    _lib.check(lib.sp_ecdsa_trace_dev(zs.data_ptr(), rs.data_ptr(), ws.data_ptr(), qxs.data_ptr(), qys.data_ptr(), k,
                                      cols.data_ptr(), _stream()), "sp_ecdsa_trace_dev")
    return cols


def range_check_trace(values):
    """values: [k, 4] device tensor -> [1, 128 k, 4] witness of the range-check AIR (v_i = value >> i)."""
    torch = _torch()
    lib = _lib.ensure_init()
    k = values.shape[0]
    col = torch.empty((1, RANGE_CHECK_BITS * k, 4), dtype=torch.int64, device=values.device)
    _lib.check(lib.sp_range_check_trace_dev(values.data_ptr(), k, col.data_ptr(), _stream()),
               "sp_range_check_trace_dev")
    return col


def fri_fold(layer, beta, shift):
    torch = _torch()
    lib = _lib.ensure_init()
    m = layer.shape[0]
    out = torch.empty((m // 2, 4), dtype=torch.int64, device=layer.device)
    _lib.check(lib.sp_fri_fold_dev(layer.data_ptr(), out.data_ptr(), m.bit_length() - 1,
                                   pack_felts([beta]), pack_felts([shift]), _stream()),
               "sp_fri_fold_dev")
    return out


def commit_rows(cols):
    """Pedersen-Merkle root over rows of `cols` [ncols, n, 4]: leaf = left-fold hash of the row
    (a single column commits the felts themselves).  Returns (root_int, levels tensor)."""
    torch = _torch()
    lib = _lib.ensure_init()
    ncols, n = cols.shape[0], cols.shape[1]
    levels = torch.empty((2 * n - 1, 4), dtype=torch.int64, device=cols.device)
    _lib.check(lib.sp_commit_rows_dev(cols.contiguous().data_ptr(), n, ncols, levels.data_ptr(), None, _stream()),
               "sp_commit_rows_dev")
    return levels


def root_of(levels):
    return tensor_to_felts(levels[-1:])[0]


def prove_commitments(xs, ys, alphas, betas, final_log=6, shift=FIELD_GEN):
    """The AIR+FRI commit job of BASELINE.json configs[3]: returns the list of commitment roots
    [trace, composition, fri_1, ..., fri_k] and the final FRI layer (Python ints)."""
    n = 512 * xs.shape[0]
    trace = pedersen_trace(xs, ys)
    trace_lde = lde(trace)
    roots = [commit_rows(trace_lde)]
    per = periodic_lde(n, shift, xs.device)
    comp = air_eval(trace_lde, per, n, alphas, shift)
    roots.append(commit_rows(comp.unsqueeze(0)))
    layer, s, k = comp, shift, 0
    while layer.shape[0] > (1 << final_log):
        layer = fri_fold(layer, betas[k], s)
        s = s * s % FIELD_PRIME
        k += 1
        if layer.shape[0] > (1 << final_log):
            roots.append(commit_rows(layer.unsqueeze(0)))
    return [root_of(r) for r in roots], tensor_to_felts(layer)


# ---- a checkable proof: Fiat-Shamir transcript, query openings -----------------------------------
# Build-defined like the rest of this module (the reference has no prover).  The transcript hash
# is SHA-256 (host); every commitment / opening hash is the reference's pedersen_hash on the GPU.
import hashlib as _hashlib


class Transcript:
    """Running SHA-256 Fiat-Shamir transcript: every challenge depends on the statement and on EVERY
    commitment absorbed before it (state <- SHA256(state || label || values))."""

    def __init__(self, air: str, n: int, shift: int, seed: int, public_inputs=()):
        self.state = _hashlib.sha256(b"starkperp/airfri/v2").digest()
        self.absorb("statement:" + air, n, shift, seed, len(public_inputs), *public_inputs)

    def absorb(self, label: str, *values: int):
        h = _hashlib.sha256(self.state + label.encode())
        for v in values:
            h.update(int(v).to_bytes(32, "big"))
        self.state = h.digest()

    def challenge(self, label: str, index: int = 0, modulus: int = FIELD_PRIME) -> int:
        d = _hashlib.sha256(self.state + label.encode() + int(index).to_bytes(8, "big")).digest()
        return int.from_bytes(d + _hashlib.sha256(d).digest(), "big") % modulus


def _path_indices(n_leaves: int, idx: int):
    """Flat indices (into a leaves-first levels buffer) of the siblings along the path of leaf idx."""
    out, off, width, i = [], 0, n_leaves, idx
    while width > 1:
        out.append(off + (i ^ 1))
        off += width
        width >>= 1
        i >>= 1
    return out


def _gather_felts(t, indices):
    torch = _torch()
    idx = torch.tensor(indices, dtype=torch.int64, device=t.device)
    return tensor_to_felts(t.index_select(0, idx))


def _table_shape(cols):
    """(n_rows, n_cols, col_stride in felts) of a committed table: [n_cols, n_rows, 4] or one column [n_rows, 4]."""
    if cols.dim() == 2:
        cols = cols.unsqueeze(0)
    assert cols.dim() == 3 and cols.shape[2] == 4 and cols.stride(2) == 1 and cols.stride(1) == 4
    stride = cols.stride(0) // 4 if cols.shape[0] > 1 else cols.shape[1]
    assert cols.stride(0) % 4 == 0 and stride >= cols.shape[1]
    return cols.shape[1], cols.shape[0], stride


def open_rows(tables, picks, host_call: bool = False):
    """The query phase's reads, all of them in one go: tables = [(cols, levels)] as committed by commit_rows (cols
    [n_cols, n_rows, 4] or a single column [n_rows, 4]; levels the tensor commit_rows returned), picks = [(table,
    row)].  Returns per pick (values, leaf, path) as Python ints: the row's value in every column, its leaf in the
    tree and the siblings from the leaves' level up - what _open_by_slices reads with one round trip per value and
    per path.  ONE sp_commit_open_dev call on the current stream and one download; host_call=True takes the
    library's host-pointer call instead (its own lane, one staged copy back; the current stream is drained first)."""
    import ctypes
    import numpy as np
    torch = _torch()
    lib = _lib.ensure_init()
    n_t, n = len(tables), len(picks)
    if n == 0:
        return []
    shapes = [_table_shape(c) for c, _ in tables]
    for (rows_t, _, _), (_, lv) in zip(shapes, tables):
        assert lv.shape[0] == 2 * rows_t - 1 and lv.is_contiguous()
    ptrs = lambda vals: (ctypes.c_void_p * max(n_t, 1))(*vals)
    sizes = lambda vals: (ctypes.c_size_t * max(n_t, 1))(*vals)
    cols_p, lv_p = ptrs([c.data_ptr() for c, _ in tables]), ptrs([lv.data_ptr() for _, lv in tables])
    n_rows, n_cols, strides = (sizes([sh[k] for sh in shapes]) for k in range(3))
    table_of = np.array([t for t, _ in picks], dtype=np.uint32)
    rows = np.array([r for _, r in picks], dtype=np.uint64)
    nv, ns = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.sp_commit_open_size(n_t, n_rows, n_cols, n, table_of.ctypes.data, ctypes.byref(nv), ctypes.byref(ns)),
               "sp_commit_open_size")
    nv, ns = nv.value, ns.value
    val_off, off = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    # one buffer: values | leaves | siblings
    if host_call:
        out = np.zeros((nv + n + ns, 4), dtype=np.uint64)
        base = out.ctypes.data
    else:
        out = torch.empty((nv + n + ns, 4), dtype=torch.int64, device=tables[0][0].device)
        base = out.data_ptr()
    args = (n_t, cols_p, strides, n_rows, n_cols, lv_p, n, table_of.ctypes.data, rows.ctypes.data, base,
            val_off.ctypes.data, base + 32 * nv, base + 32 * (nv + n), off.ctypes.data)
    if host_call:
        torch.cuda.current_stream().synchronize()  # the lane's stream does not wait for the one that committed
        _lib.check(lib.sp_commit_open(*args), "sp_commit_open")
        raw = out.tobytes()
    else:
        _lib.check(lib.sp_commit_open_dev(*args, _stream()), "sp_commit_open_dev")
        raw = out.cpu().numpy().tobytes()  # the one download; it waits for the stream
    felts = [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(nv + n + ns)]
    val_off, off, sib = val_off.tolist(), off.tolist(), nv + n
    return [(felts[val_off[i] : val_off[i + 1]], felts[nv + i], felts[sib + off[i] : sib + off[i + 1]])
            for i in range(n)]


def _open_by_slices(tables, picks):
    """What open_rows returns, read the way the query phase read it before sp_commit_open: every value with its own
    slice and synchronous download, every path with its own index upload, gather and download.  Kept as the
    in-process reference of open_rows (tests/test_gpu_commit_open.py)."""
    out = []
    for t, row in picks:
        cols, lv = tables[t]
        if cols.dim() == 2:
            cols = cols.unsqueeze(0)
        values = [tensor_to_felts(cols[c][row : row + 1])[0] for c in range(cols.shape[0])]
        out.append((values, tensor_to_felts(lv[row : row + 1])[0], _gather_felts(lv, _path_indices(cols.shape[1], row))))
    return out


def prove(xs, ys, n_queries: int = 8, seed: int = 0, final_log: int = 6, shift: int = FIELD_GEN):
    """Benchmark-grade argument (NOT a sound proof system) that the trace of the hashes (xs[i], ys[i])
    satisfies the Pedersen-step AIR: see prove_trace for what is and is not bound."""
    return prove_trace(pedersen_trace(xs, ys), "pedersen", n_queries, seed, final_log, shift)


def prove_ec_ladders(ms, qxs, qys, n_queries: int = 8, seed: int = 0, final_log: int = 6,
                     shift: int = FIELD_GEN):
    """Benchmark-grade argument (NOT a sound proof system) that k scalar multiplications
    m * Q + SHIFT_POINT were carried out step by step as mimic_ec_mult_air does (the EC-ladder AIR)."""
    return prove_trace(ec_ladder_trace(ms, qxs, qys), "ec_ladder", n_queries, seed, final_log, shift)


def prove_ecdsa(msg_hashes, rs, ss, public_keys, n_queries: int = 8, seed: int = 0, final_log: int = 6,
                shift: int = FIELD_GEN):
    """Benchmark-grade argument (NOT a sound proof system) that every (z, r, s, Q) passes the reference's
    verify (signature.py:217-260: the three ladders, the two additions, x == r).  Python ints in; the
    count must be a power of two.  w = s^-1 mod N is computed here as verify() does (:220) and the public
    inputs (z, r, s, Qx, Qy per signature) are absorbed into the transcript; the verifier (verify, and its oracle
    oracle/stark_ref.verify_proof) re-derives w from s."""
    dev = "cuda"
    ws = [pow(s, -1, EC_ORDER) for s in ss]
    for z, r, w in zip(msg_hashes, rs, ws):
        assert 0 < z < 2**251 and 1 <= r < 2**251 and 1 <= w < 2**251
    trace = ecdsa_trace(*(felts_to_tensor(v, dev) for v in (msg_hashes, rs, ws, [q[0] for q in public_keys],
                                                          [q[1] for q in public_keys])))
    public = [v for z, r, s, q in zip(msg_hashes, rs, ss, public_keys) for v in (z, r, s, q[0], q[1])]
    return prove_trace(trace, "ecdsa", n_queries, seed, final_log, shift, public)


def prove_range_checks(values, n_queries: int = 8, seed: int = 0, final_log: int = 6, shift: int = FIELD_GEN):
    """Benchmark-grade argument (NOT a sound proof system) that every value lies in [0, 2^128) - the bound
    the Cairo range-check builtin gives the amounts, ids, nonces and timestamps of the exchange messages.
    Python ints in; the count must be a power of two.  The values are absorbed as public inputs."""
    values = list(values)
    assert values and len(values) & (len(values) - 1) == 0
    for v in values:
        assert 0 <= v < FIELD_PRIME
    return prove_trace(range_check_trace(felts_to_tensor(values, "cuda")), "range_check", n_queries, seed, final_log,
                       shift, values)


def prove_trace(trace, air: str, n_queries: int = 8, seed: int = 0, final_log: int = 6,
                shift: int = FIELD_GEN, public_inputs=()):
    """Commitments to the trace LDE, the composition column and every FRI layer, the final layer in
    the clear, and for each query the openings a verifier needs (verify; oracle/stark_ref.verify_proof is its oracle).

    What this is: the prover-side workload of BASELINE.json configs[3] made checkable end to end.  The
    Fiat-Shamir transcript is chained (statement, then every commitment in order; alpha, every beta and
    the query positions are drawn from it).  What it is not: a sound, complete STARK - no boundary
    constraint binds the hash inputs / outputs (or `public_inputs`, which are only absorbed; for the
    Pedersen AIR prove_hashes adds those constraints, for the ECDSA and range-check AIRs prove_signatures and
    prove_ranges), there is no zero knowledge, and the default 8 queries at blowup 4 give about 16 bits.  The reference has no
    prover; this path is build-defined and benchmark-grade."""
    return _query_trace(_commit_trace(trace, air, seed, final_log, shift, public_inputs), n_queries)


def _commit_trace(trace, air, seed, final_log, shift, public_inputs, statement=None):
    """The commit phase of prove_trace: every commitment, the transcript up to the final layer.  Returns what the
    query phase needs.  `statement` (prove_hashes) = (name, extra, add): the AIR name the transcript and the proof
    carry instead of `air`, how many challenges are drawn after the AIR's own in the same way, and the function
    add(trace_lde, comp, extra_alphas) -> comp of what they bring to the composition."""
    P = FIELD_PRIME
    spec = AIRS[air]
    name, n_extra, add = statement or (air, 0, None)
    n = trace.shape[1]
    M = n << BLOWUP_LOG
    tr = Transcript(name, n, shift, seed, public_inputs)
    trace_lde = lde(trace)
    lv_trace = commit_rows(trace_lde)
    root_t = root_of(lv_trace)
    tr.absorb("trace_root", root_t)
    alphas = [tr.challenge("alpha", k) for k in range(spec["n_constraints"] + n_extra)]
    per = periodic_lde(n, shift, trace.device, air)
    comp = air_eval(trace_lde, per, n, alphas[:spec["n_constraints"]], shift, air)
    if add is not None:
        comp = add(trace_lde, comp, alphas[spec["n_constraints"]:])
    layers, level_bufs, roots = [comp], [], []
    s = shift
    while True:
        cur = layers[-1]
        lv = commit_rows(cur.unsqueeze(0))
        level_bufs.append(lv)
        roots.append(root_of(lv))
        tr.absorb("layer_root", roots[-1])
        beta = tr.challenge("beta", len(roots))
        nxt = fri_fold(cur, beta, s)
        s = s * s % P
        layers.append(nxt)
        if nxt.shape[0] <= (1 << final_log):
            break
    final = tensor_to_felts(layers[-1])
    tr.absorb("final_layer", *final)
    return {"tr": tr, "M": M, "trace_lde": trace_lde, "lv_trace": lv_trace, "layers": layers, "level_bufs": level_bufs,
            "head": {"n": n, "air": name, "seed": seed, "shift": shift, "public_inputs": list(public_inputs),
                     "trace_root": root_t, "layer_roots": roots, "final_layer": final}}


def _layer_positions(j, layers):
    """The pair of positions a query at index j opens in every committed FRI layer."""
    out, jk = [], j
    for layer in layers:
        mk = layer.shape[0]
        jk %= mk // 2
        out.append((jk, jk + mk // 2))
    return out


def _query_trace(c, n_queries, opener=None):
    """The query phase of prove_trace on the state _commit_trace returned: the positions are drawn first (host-only
    transcript work), every pick of the proof - four trace rows and one pair per layer for each query - goes to ONE
    opener call (open_rows; _open_by_slices is the reference), then the dict is assembled."""
    opener = opener or open_rows
    M, layers = c["M"], c["layers"][:-1]
    tables = [(c["trace_lde"], c["lv_trace"])] + list(zip(layers, c["level_bufs"]))
    indices = [c["tr"].challenge("query", q, modulus=M // 2) for q in range(n_queries)]
    picks = []
    for j in indices:
        for pos in (j, j + M // 2):
            for row in (pos, (pos + (1 << BLOWUP_LOG)) % M):
                picks.append((0, row))
        for k, pair in enumerate(_layer_positions(j, layers)):
            picks += [(1 + k, pos) for pos in pair]
    opened = iter(zip(picks, opener(tables, picks)))
    queries = []
    for j in indices:
        entry = {"index": j, "trace": [], "layers": []}
        for _ in range(4):
            (_, row), (values, _, path) = next(opened)
            entry["trace"].append({"row": row, "values": values, "path": path})
        for _ in layers:
            pair = []
            for _ in range(2):
                (_, pos), (values, _, path) = next(opened)
                pair.append({"pos": pos, "value": values[0], "path": path})
            entry["layers"].append(pair)
        queries.append(entry)
    return dict(c["head"], queries=queries)


def check_merkle_openings(proof) -> List[Tuple[str, bool]]:
    """The Merkle part of a verifier, on the GPU: does every opening of `proof` (from prove_trace or one of its
    wrappers: prove, prove_ec_ladders, prove_ecdsa, prove_range_checks) fold to the commitment it claims?

    Returns one (label, ok) per opening in proof order, labelled "q3/trace/row 517" (a trace row against
    trace_root) or "q3/layer 2/pos 40" (a FRI layer value against layer_roots[2]).  Two library calls in all: the
    leaves of the opened trace rows - the left fold of the row's values, as commit_rows - are hashed by one
    pedersen_chains_ragged call, and every path of the proof, the trace openings of height log2(M) and the layer
    openings of falling heights, goes to ONE sp_merkle_verify_paths call with offsets and per-item expected roots.
    A value outside [0, p) makes its opening False.

    This checks the Merkle part ONLY.  The AIR relation between the opened rows and the composition column, the FRI
    fold consistency, the final layer's degree, the query positions and the transcript are verify()'s, which calls
    this for its Merkle part: a proof whose openings are all True here can still be rejected there."""
    import numpy as np
    from . import batch_np
    P = FIELD_PRIME
    felt = lambda v: v if 0 <= v < 2**256 else P  # unrepresentable: p itself, which the device flags as out of range
    labels, keys, expected, paths = [], [], [], []
    rows, leaf_slot = [], []  # the chains of the trace rows; leaf_slot[i] = index into rows or None (leaf given)
    leaves = []
    for qi, q in enumerate(proof["queries"]):
        for t in q["trace"]:
            labels.append("q%d/trace/row %d" % (qi, t["row"]))
            keys.append(t["row"])
            expected.append(proof["trace_root"])
            paths.append([felt(v) for v in t["path"]])
            leaf_slot.append(len(rows))
            rows.append([felt(v) for v in t["values"]])
            leaves.append(0)
        for k, pair in enumerate(q["layers"]):
            for o in pair:
                labels.append("q%d/layer %d/pos %d" % (qi, k, o["pos"]))
                keys.append(o["pos"])
                expected.append(proof["layer_roots"][k])
                paths.append([felt(v) for v in o["path"]])
                leaf_slot.append(None)
                leaves.append(felt(o["value"]))
    n = len(labels)
    if n == 0:
        return []
    leaf_arr = batch_np.felts_from_ints(leaves)
    leaf_bad = np.zeros(n, dtype=bool)
    if rows:
        row_off = np.zeros(len(rows) + 1, dtype=np.uint32)
        row_off[1:] = np.cumsum([len(r) for r in rows])
        hashed, row_st = batch_np.pedersen_chains_ragged(batch_np.felts_from_ints([v for r in rows for v in r]), row_off)
        slots = np.array([i for i, s in enumerate(leaf_slot) if s is not None])
        leaf_arr[slots] = hashed
        leaf_bad[slots] = row_st != 0
        leaf_arr[slots[row_st != 0]] = 0  # what a failed chain leaves is unspecified; the opening is False anyway
    # a position that does not fit its path's height cannot be opened by it
    fits = np.array([len(p) <= 64 and 0 <= k < (1 << len(p)) for k, p in zip(keys, paths)])
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) if f else 0 for p, f in zip(paths, fits)])
    flat = [v for p, f in zip(paths, fits) if f for v in p]
    sib = batch_np.felts_from_ints(flat) if flat else np.zeros((0, 4), dtype=np.uint64)
    key_arr = np.array([k if f else 0 for k, f in zip(keys, fits)], dtype=np.uint64)
    verdict, _ = batch_np.merkle_verify_paths(leaf_arr, sib, key_arr, batch_np.felts_from_ints([felt(v) for v in expected]),
                                              offsets=off)
    ok = verdict & fits & ~leaf_bad
    return list(zip(labels, [bool(v) for v in ok]))


# ---- the verifier ---------------------------------------------------------------------------------------------
# Product twin of oracle/stark_ref.verify_proof: the same checks in the same order with the same reasons.  The
# transcript (SHA-256) and the comparisons of positions run on the host; every hash goes through the chain and path
# calls of check_merkle_openings, the composition values and the fold chains through the two calls of csrc/verify.hip,
# the final layer's interpolation through ntt.
AIR_IDS = {"pedersen": 0, "ec_ladder": 1, "ecdsa": 2, "range_check": 3}  # SP_AIR_* of include/starkperp.h
POINT_OK, POINT_OUT_OF_RANGE = 0, 1
FOLD_OK, FOLD_MISMATCH, FOLD_OUT_OF_RANGE = 0, 1, 2


def air_eval_points(air, n, per_lde, alphas, shift, pos, cur, nxt):
    """The composition value at arbitrary LDE positions from opened rows (sp_air_eval_points_dev): pos [k] int64
    tensor of LDE indices, cur / nxt [k, n_cols, 4] the rows at pos and at (pos + 4) mod 4n.  Returns (out [k, 4],
    status [k] uint8): what air_eval writes at those indices, and POINT_OK / POINT_OUT_OF_RANGE per point."""
    torch = _torch()
    lib = _lib.ensure_init()
    spec = AIRS[air]
    k = pos.shape[0]
    assert len(alphas) == spec["n_constraints"] and tuple(cur.shape) == tuple(nxt.shape) == (k, spec["n_cols"], 4)
    assert pos.dtype == torch.int64 and pos.is_contiguous() and cur.is_contiguous() and nxt.is_contiguous()
    out = torch.empty((k, 4), dtype=torch.int64, device=cur.device)
    status = torch.empty((k,), dtype=torch.uint8, device=cur.device)
    _lib.check(lib.sp_air_eval_points_dev(AIR_IDS[air], n.bit_length() - 1, per_lde.data_ptr(), pack_felts(alphas),
                                          pack_felts([shift]), k, pos.data_ptr(), cur.data_ptr(), nxt.data_ptr(),
                                          out.data_ptr(), status.data_ptr(), _stream()), "sp_air_eval_points_dev")
    return out, status


def fri_check_queries(log_m, betas, shift, index, pairs, final_layer):
    """The fold chain of every query (sp_fri_check_queries_dev): index [q] int64 tensor, pairs [q, n_layers, 2, 4]
    the opened values of every layer, final_layer [2^(log_m - n_layers), 4].  Returns status [q, n_layers] uint8:
    FOLD_OK / FOLD_MISMATCH / FOLD_OUT_OF_RANGE for the step from layer k to layer k + 1 (the final layer last)."""
    torch = _torch()
    lib = _lib.ensure_init()
    q, n_layers = index.shape[0], len(betas)
    assert tuple(pairs.shape) == (q, n_layers, 2, 4) and tuple(final_layer.shape) == (1 << (log_m - n_layers), 4)
    assert index.dtype == torch.int64 and index.is_contiguous() and pairs.is_contiguous() and final_layer.is_contiguous()
    status = torch.empty((q, n_layers), dtype=torch.uint8, device=pairs.device)
    _lib.check(lib.sp_fri_check_queries_dev(log_m, n_layers, pack_felts([shift]), pack_felts(betas), q, index.data_ptr(),
                                            pairs.data_ptr(), final_layer.data_ptr(), status.data_ptr(), _stream()),
               "sp_fri_check_queries_dev")
    return status


def _is_int(v):
    return type(v) is int


def _is_felt(v):
    return type(v) is int and 0 <= v < FIELD_PRIME


def _felt_list(v, length=None):
    return isinstance(v, (list, tuple)) and (length is None or len(v) == length) and all(_is_felt(x) for x in v)


def _wellformed(proof):
    """Whether `proof` has the keys and types of a prove_trace proof, every felt in [0, p), every integer an int: what
    must hold before a value is hashed into the transcript or sent to the device.  Lengths that the oracle reports
    as "shape" (layer_roots, final_layer) are left to verify."""
    if not isinstance(proof, dict):
        return False
    air, n, shift = proof.get("air", "pedersen"), proof.get("n"), proof.get("shift")
    if not isinstance(air, str) or air not in AIR_IDS:
        return False
    spec = AIRS[air]
    if not (_is_int(n) and spec["period"] <= n <= 1 << 30 and n & (n - 1) == 0):
        return False
    # a shift with shift^(4n) = 1 puts the coset onto the trace domain: no composition column exists on it
    if not (_is_felt(shift) and shift != 0 and pow(shift, 4 * n, FIELD_PRIME) != 1):
        return False
    if not (_is_int(proof.get("seed")) and 0 <= proof["seed"] < 1 << 256 and _is_felt(proof.get("trace_root"))):
        return False
    pub = proof.get("public_inputs", ())
    if not (isinstance(pub, (list, tuple)) and all(_is_int(v) and 0 <= v < 1 << 256 for v in pub)):
        return False
    if not (_felt_list(proof.get("layer_roots")) and _felt_list(proof.get("final_layer"))):
        return False
    queries = proof.get("queries")
    if not isinstance(queries, (list, tuple)):
        return False
    log_m = n.bit_length() + 1
    for q in queries:
        if not (isinstance(q, dict) and _is_int(q.get("index")) and isinstance(q.get("trace"), (list, tuple))
                and isinstance(q.get("layers"), (list, tuple)) and len(q["trace"]) == 4):
            return False
        for t in q["trace"]:
            if not (isinstance(t, dict) and _is_int(t.get("row")) and _felt_list(t.get("values"), spec["n_cols"])
                    and _felt_list(t.get("path"), log_m)):
                return False
        for k, pair in enumerate(q["layers"]):
            if not (isinstance(pair, (list, tuple)) and len(pair) == 2):
                return False
            for o in pair:
                if not (isinstance(o, dict) and _is_int(o.get("pos")) and _is_felt(o.get("value"))
                        and _felt_list(o.get("path"), max(log_m - k, 0))):
                    return False
    return True


def _public_inputs_ok(air, n, pub):
    """The statement rules of oracle/stark_ref.verify_proof for the AIRs that have public inputs."""
    if air == "ecdsa":
        from .signature import is_point_on_curve
        if len(pub) != 5 * (n // 1024):
            return False
        for k in range(n // 1024):
            z, r, sig_s, qx, qy = pub[5 * k : 5 * k + 5]
            if not (1 <= sig_s < EC_ORDER and 1 <= r < 2**251 and 0 < z < 2**251 and is_point_on_curve(qx, qy)):
                return False
            if not 1 <= pow(sig_s, -1, EC_ORDER) < 2**251:
                return False
    if air == "range_check":
        if len(pub) != n // RANGE_CHECK_BITS or not all(0 <= v < 2**RANGE_CHECK_BITS for v in pub):
            return False
    return True


# What every verifier here shares, _verify_trace_proof and verify_builtins alike.  Each helper that can fail returns
# the reason, or None.
def _fri_shape_reason(proof, n_layers, final_log, n_queries):
    """The lengths of layer_roots and final_layer, at least one layer, and a given n_queries."""
    if len(proof["layer_roots"]) != n_layers or len(proof["final_layer"]) != 1 << final_log or n_layers < 1:
        return "shape"
    if n_queries is not None and n_queries != len(proof["queries"]):
        return "shape"
    if any(len(q["layers"]) != n_layers for q in proof["queries"]):
        return "malformed"
    return None


def _replay_fri_challenges(tr, proof, m):
    """The transcript after the alphas: (betas, query indices)."""
    betas = []
    for k, root in enumerate(proof["layer_roots"]):
        tr.absorb("layer_root", root)
        betas.append(tr.challenge("beta", k + 1))
    tr.absorb("final_layer", *proof["final_layer"])
    return betas, [tr.challenge("query", qi, modulus=m // 2) for qi in range(len(proof["queries"]))]


def _final_layer_reason(final_t, n, n_layers):
    """The final layer's interpolant on shift^(2^n_layers) * <w> has the coefficients c_k shift'^k of the inverse
    transform over <w>, so the zero pattern is the same."""
    coeffs = tensor_to_felts(ntt(final_t, inverse=True))
    return "final layer degree" if any(c != 0 for c in coeffs[3 * n >> n_layers:]) else None


def _fold_statuses(queries, indices, betas, shift, log_m, final_t, dev):
    """[q][n_layers] FOLD_* of every fold step of every query, one sp_fri_check_queries_dev launch."""
    torch = _torch()
    pairs = felts_to_tensor([o["value"] for q in queries for pair in q["layers"] for o in pair], dev)
    fold_st = fri_check_queries(log_m, betas, shift, torch.tensor(indices, dtype=torch.int64, device=dev),
                                pairs.reshape(len(queries), len(betas), 2, 4), final_t)
    return fold_st.cpu().tolist()


def _composition_reason(q, qi, comp, comp_st):
    """Layer 0 of query qi opens the composition column at the two opened points."""
    for side in (0, 1):
        if comp_st[2 * qi + side] != POINT_OK or q["layers"][0][side]["value"] != comp[2 * qi + side]:
            return "composition value"
    return None


def _layers_reason(q, j, m, layer_ok, fold_st):
    """The layers of one query in the oracle's order: layer_ok[k] the verdicts of layer k's two Merkle openings,
    fold_st[k] the FOLD_* of the step out of layer k."""
    jk, mk = j, m
    for k, (a, b) in enumerate(q["layers"]):
        jk %= mk // 2
        if (a["pos"], b["pos"]) != (jk, jk + mk // 2):
            return "layer positions"
        if not all(layer_ok[k]):
            return "layer path"
        if fold_st[k] != FOLD_OK:
            return "fold consistency at layer %d" % k
        mk //= 2
    return None


def _verify_trace_proof(proof, final_log, n_queries, name, air, public_ok, boundary=None):
    """The one verifier of prove_trace-shaped proofs; verify, verify_hashes, verify_signatures and verify_ranges are
    its wrappers and document it.  `name` is the AIR name the proof and the transcript carry, `air` the base AIR whose
    shape rules, constraints and Merkle part apply; public_ok(air, n, pub) is the statement rule.  `boundary`, when
    given, is (n_extra, f): the transcript yields n_extra more alphas, and f(pub, n, extra_alphas, shift, positions,
    cur, dev) -> (values, status) at the opened points is added to the composition value (sp_felt_add_dev), its
    status ORed into the points'."""
    try:
        if not (isinstance(proof, dict) and isinstance(air, str) and air in AIR_IDS
                and proof.get("air", "pedersen") == name):
            return False, "malformed"
        view = proof if name == air else dict(proof, air=air)  # shape rules and Merkle part are the base AIR's
        if not (_wellformed(view) and _is_int(final_log) and 0 <= final_log <= 30):
            return False, "malformed"
    except Exception:  # an object that misbehaves when inspected is malformed too
        return False, "malformed"
    spec = AIRS[air]
    n, seed, shift, queries = proof["n"], proof["seed"], proof["shift"], proof["queries"]
    pub = list(proof.get("public_inputs", ()))
    if not public_ok(air, n, pub):
        return False, "public inputs"
    m = n << BLOWUP_LOG
    log_m = m.bit_length() - 1
    n_layers = log_m - final_log
    reason = _fri_shape_reason(proof, n_layers, final_log, n_queries)
    if reason:
        return False, reason
    nc = spec["n_constraints"]
    n_extra, boundary_at = boundary or (0, None)
    tr = Transcript(name, n, shift, seed, pub)
    tr.absorb("trace_root", proof["trace_root"])
    alphas = [tr.challenge("alpha", k) for k in range(nc + n_extra)]
    betas, indices = _replay_fri_challenges(tr, proof, m)
    torch = _torch()
    final_t = felts_to_tensor(proof["final_layer"])
    reason = _final_layer_reason(final_t, n, n_layers)
    if reason:
        return False, reason
    if not queries:
        return True, "ok"
    openings = iter(check_merkle_openings(view))
    per = periodic_lde(n, shift, "cuda", air)
    dev = per.device
    positions = torch.tensor([pos for j in indices for pos in (j, j + m // 2)], dtype=torch.int64, device=dev)
    cur = felts_to_tensor([v for q in queries for side in (0, 1) for v in q["trace"][2 * side]["values"]], dev)
    nxt = felts_to_tensor([v for q in queries for side in (0, 1) for v in q["trace"][2 * side + 1]["values"]], dev)
    shape = (positions.shape[0], spec["n_cols"], 4)
    cur, nxt = cur.reshape(shape), nxt.reshape(shape)
    comp, comp_st = air_eval_points(air, n, per, alphas[:nc], shift, positions, cur, nxt)
    bnd_st = None
    if boundary_at:
        bnd, bnd_st = boundary_at(pub, n, alphas[nc:], shift, positions, cur, dev)
        comp = felt_add(comp, bnd)
    fold_st = _fold_statuses(queries, indices, betas, shift, log_m, final_t, dev)
    comp, comp_st = tensor_to_felts(comp), comp_st.cpu().tolist()
    if bnd_st is not None:
        comp_st = [a | b for a, b in zip(comp_st, bnd_st.cpu().tolist())]
    for qi, (q, j) in enumerate(zip(queries, indices)):
        trace_ok = [next(openings)[1] for _ in range(4)]
        layer_ok = [[next(openings)[1] for _ in range(2)] for _ in range(n_layers)]
        if q["index"] != j:
            return False, "query index"
        if [t["row"] for t in q["trace"]] != [j, (j + 4) % m, j + m // 2, (j + m // 2 + 4) % m]:
            return False, "trace rows"
        if not all(trace_ok):
            return False, "trace path"
        reason = _composition_reason(q, qi, comp, comp_st) or _layers_reason(q, j, m, layer_ok, fold_st[qi])
        if reason:
            return False, reason
    return True, "ok"


def verify(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of the proofs of prove_trace and its wrappers (prove, prove_ec_ladders, prove_ecdsa,
    prove_range_checks): returns (ok, reason) with the reasons of oracle/stark_ref.verify_proof, the first failure
    in that function's order - "public inputs", "shape", "final layer degree", then per query "query index", "trace
    rows", "trace path", "composition value" and per layer "layer positions", "layer path", "fold consistency at
    layer k" - or (True, "ok").  `final_log` is the prover's; a given `n_queries` must be the number of queries
    ("shape").

    Where it runs: the transcript (alphas, betas, query indices) and the comparisons of indices, rows and positions
    on the host; every hash on the GPU through check_merkle_openings (two calls); the composition value of the 2 Q
    opened points in ONE sp_air_eval_points_dev launch and the Q n_layers fold steps in ONE
    sp_fri_check_queries_dev launch; the final layer's coefficients through ntt.  Everything is computed, then the
    first failure is reported.

    A malformed proof - a missing key, a non-integer, a felt outside [0, p), a path of the wrong length, an unknown
    air, an n that is no power of two of at least the AIR's period, a shift that is 0 or puts the coset onto the
    trace domain - returns (False, "malformed") before the library is initialised: nothing raises and no such value
    reaches the device.  A prove_builtins proof (air == "builtins") raises ValueError: its verifier needs the
    second-phase column and the challenge z and is a function of its own, verify_builtins.

    The caveat of prove_trace holds here too: this verifies a benchmark-grade argument, NOT a sound proof system -
    no boundary constraint binds the public inputs (they are only absorbed, and range-checked as the oracle does),
    and Q queries at blowup 4 give about 2 Q bits."""
    if isinstance(proof, dict) and proof.get("air") == "builtins":
        raise ValueError("stark.verify does not take prove_builtins proofs (the builtins verifier is "
                         "stark.verify_builtins)")
    air = proof.get("air", "pedersen") if isinstance(proof, dict) else None
    return _verify_trace_proof(proof, final_log, n_queries, air, air, _public_inputs_ok)


# ---- Pedersen proofs that bind their statement: h_i = pedersen_hash(x_i, y_i) for k given triples -----------------
# DESIGN.md 6.4.  Three boundary quotients join the composition of the Pedersen-step AIR with three more challenges:
# s at row 512 i is x_i, s at row 512 i + 256 is y_i, px at row 512 i + 511 is h_i.  Definition in integers:
# tests/hash_io_ref.py (on oracle/stark_ref.py); kernels: csrc/hash_io.hip.
HASH_IO_AIR = "pedersen_io"
N_HASH_IO_ALPHAS = 3
HASH_IO_ROWS = (0, 256, 511)  # the row of a hash's 512 at which x_i, y_i, h_i stand (columns s, s, px)


def _root_of_unity(n):
    return pow(FIELD_GEN, (FIELD_PRIME - 1) // n, FIELD_PRIME)


def hash_io_public_lde(public_inputs, n, shift=FIELD_GEN, device="cuda"):
    """[3, 4n, 4]: the polynomials of degree < k = n / 512 through the x_i, the y_i and the h_i of public_inputs =
    [x_0, y_0, h_0, x_1, ...] over <g^512>, at the arguments the boundary constraints give them on the LDE coset -
    x_j, x_j g^-256 and x_j g^-511 for x_j = shift w_4n^j.  Three sp_lde_dev calls of k points at blowup 2048."""
    torch = _torch()
    k = n // 512
    assert len(public_inputs) == 3 * k
    g = _root_of_unity(n)
    cols = [lde(felts_to_tensor(public_inputs[c::3], device).unsqueeze(0), 11,
                shift * pow(g, -r, FIELD_PRIME) % FIELD_PRIME)[0] for c, r in enumerate(HASH_IO_ROWS)]
    return torch.stack(cols)


def hash_io_boundary(trace_lde, pub_lde, n, alphas, shift=FIELD_GEN, acc=None, out=None):
    """out[j] = (acc[j] if acc is given else 0) + B(x_j) on the whole LDE coset (sp_hash_io_boundary_dev): trace_lde
    the committed [4, 4n, 4] trace LDE (columns s and px are read), pub_lde from hash_io_public_lde, alphas the three
    boundary challenges.  `out` may be `acc`."""
    torch = _torch()
    lib = _lib.ensure_init()
    M = 4 * n
    assert len(alphas) == N_HASH_IO_ALPHAS and trace_lde.shape[0] >= 2 and trace_lde.shape[1] == M
    assert tuple(pub_lde.shape) == (3, M, 4) and pub_lde.is_contiguous()
    _, _, stride = _table_shape(trace_lde)
    if out is None:
        out = torch.empty((M, 4), dtype=torch.int64, device=trace_lde.device)
    assert tuple(out.shape) == (M, 4) and out.is_contiguous() and (acc is None or (tuple(acc.shape) == (M, 4)
                                                                                    and acc.is_contiguous()))
    _lib.check(lib.sp_hash_io_boundary_dev(trace_lde.data_ptr(), stride, pub_lde.data_ptr(), n.bit_length() - 1,
                                           pack_felts(alphas), pack_felts([shift]),
                                           None if acc is None else acc.data_ptr(), out.data_ptr(), _stream()),
               "sp_hash_io_boundary_dev")
    return out


def hash_io_coefficients(public_inputs, n, device="cuda"):
    """[3, k, 4]: the coefficients, in natural order, of the three public polynomials (three inverse ntt calls; at
    k = 1 they are the values)."""
    torch = _torch()
    cols = [felts_to_tensor(public_inputs[c::3], device) for c in range(3)]
    return torch.stack([col if n == 512 else ntt(col, inverse=True) for col in cols]).contiguous()


def hash_io_boundary_points(n, coef, alphas, shift, pos, cur):
    """B at arbitrary LDE positions from opened rows (sp_hash_io_boundary_points_dev): coef [3, k, 4] from
    hash_io_coefficients, pos [q] int64 tensor of LDE indices, cur [q, 4, 4] the trace rows there.  Returns (out
    [q, 4], status [q] uint8): what hash_io_boundary adds at those indices, and POINT_OK / POINT_OUT_OF_RANGE."""
    torch = _torch()
    lib = _lib.ensure_init()
    q = pos.shape[0]
    assert len(alphas) == N_HASH_IO_ALPHAS and tuple(coef.shape) == (3, n // 512, 4) and coef.is_contiguous()
    assert pos.dtype == torch.int64 and pos.is_contiguous() and tuple(cur.shape) == (q, 4, 4) and cur.is_contiguous()
    out = torch.empty((q, 4), dtype=torch.int64, device=cur.device)
    status = torch.empty((q,), dtype=torch.uint8, device=cur.device)
    _lib.check(lib.sp_hash_io_boundary_points_dev(n.bit_length() - 1, coef.data_ptr(), pack_felts(alphas),
                                                  pack_felts([shift]), q, pos.data_ptr(), cur.data_ptr(),
                                                  out.data_ptr(), status.data_ptr(), _stream()),
               "sp_hash_io_boundary_points_dev")
    return out, status


def prove_hashes(xs, ys, n_queries: int = 8, seed: int = 0, final_log: int = 6, shift: int = FIELD_GEN, outs=None):
    """A proof of a statement: h_i = pedersen_hash(x_i, y_i) for the k triples of public_inputs = [x_0, y_0, h_0, x_1,
    ...].  xs, ys: [k, 4] device tensors as for prove, k a power of two up to 2^15; h_i is read from the trace (px at
    row 512 i + 511).  `outs`, when given, is the list of CLAIMED outputs, taken instead - it exists so that a test
    can make the prover lie consistently: such a proof is rejected ("final layer degree").

    What is bound, and was not by prove: both inputs and the output of EVERY hash.  On top of the eleven constraints
    of the Pedersen-step AIR three boundary quotients with challenges of their own (14 alphas, AIR name
    "pedersen_io") tie s at rows 512 i and 512 i + 256 and px at row 512 i + 511 to the polynomials through the x_i,
    y_i and h_i; the composition is sp_air_eval_dev plus sp_hash_io_boundary_dev.  Commitments, FRI and the query
    phase are prove_trace's and the proof has its shape.  Verifier: verify_hashes (verify answers "malformed").

    What still is not: there is no zero knowledge (the opened rows are trace values), and Q queries at blowup 4 give
    about 2 Q bits of soundness - the statement is now the right one, the argument is still benchmark-grade."""
    k = xs.shape[0]
    assert k >= 1 and k & (k - 1) == 0 and k <= 1 << 15 and tuple(ys.shape) == tuple(xs.shape)
    n = 512 * k
    trace = pedersen_trace(xs, ys)
    hs = tensor_to_felts(trace[1, 511::512]) if outs is None else [int(v) for v in outs]
    assert len(hs) == k
    public = [v for triple in zip(tensor_to_felts(xs), tensor_to_felts(ys), hs) for v in triple]

    def add_boundary(trace_lde, comp, alphas):
        return hash_io_boundary(trace_lde, hash_io_public_lde(public, n, shift, trace_lde.device), n, alphas, shift,
                                acc=comp, out=comp)
    c = _commit_trace(trace, "pedersen", seed, final_log, shift, public, (HASH_IO_AIR, N_HASH_IO_ALPHAS, add_boundary))
    return _query_trace(c, n_queries)


def verify_hashes(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of prove_hashes: (True, "ok") says that h_i = pedersen_hash(x_i, y_i) for every triple of
    proof["public_inputs"] = [x_0, y_0, h_0, x_1, ...] - inputs and output of every hash are bound by the boundary
    constraints - up to the soundness of the argument: about 2 Q bits for Q queries at blowup 4, and no zero
    knowledge.  Reasons, their order and the "malformed" rules are verify's; "public inputs" when the list does not
    hold 3 n / 512 felts.  A proof of another AIR is "malformed" here, as this AIR is for verify.

    Where it runs: as verify - transcript and comparisons on the host (14 alphas), Merkle openings through
    check_merkle_openings, folds through sp_fri_check_queries_dev - with the composition value of the 2 Q opened
    points as the sum (sp_felt_add_dev) of sp_air_eval_points_dev for the eleven AIR constraints and
    sp_hash_io_boundary_points_dev for the three boundary quotients, which takes the public polynomials'
    coefficients from three inverse ntt calls made once per proof."""
    def public_ok(air, n, pub):
        return len(pub) == 3 * (n // 512) and all(_is_felt(v) for v in pub)

    def boundary_at(pub, n, alphas, shift, positions, cur, dev):
        return hash_io_boundary_points(n, hash_io_coefficients(pub, n, dev), alphas, shift, positions, cur)
    return _verify_trace_proof(proof, final_log, n_queries, HASH_IO_AIR, "pedersen", public_ok,
                               (N_HASH_IO_ALPHAS, boundary_at))


# ---- boundary constraints from a descriptor: ECDSA and range-check proofs that bind their statement --------------
# DESIGN.md 6.5.  What hash_io does for the Pedersen AIR, general over the AIR: a descriptor names boundary groups (a
# row below the period each) and terms (column, group); one challenge per term; ONE public polynomial per group.
# Definition in integers: tests/boundary_ref.py (on oracle/stark_ref.py); kernels: csrc/boundary.hip.
BOUNDARY_DESCRIPTORS = {
    # m = z_i at row 0; m = r_i, qx = Qx_i, qy = Qy_i at row 256; m = w_i = s_i^-1 mod N at row 512
    "ecdsa_io": {"air": "ecdsa", "rows": (0, 256, 512), "terms": ((0, 0), (0, 1), (3, 1), (4, 1), (0, 2))},
    "range_check_io": {"air": "range_check", "rows": (0,), "terms": ((0, 0),)},  # v = value_i at row 0
    # the statement of prove_hashes (which keeps its own kernels): the cross-check of the two implementations
    "pedersen_io": {"air": "pedersen", "rows": HASH_IO_ROWS, "terms": ((0, 0), (0, 1), (1, 2))},
    # the rc16 segment of a combined builtin trace (prove_builtin_usage): acc = value_i at a value's last limb, row 7.
    # Period 8 is below what sp_boundary_dev takes: this one runs through sp_builtins_boundary_dev only.
    "rc16_io": {"air": "rc16", "rows": (7,), "terms": ((1, 0),)},
}


def _descriptor(desc):
    """A descriptor by name, or a dict of one's own: "rows", "terms" as (column, group), and either "air" or
    "period" and "n_cols" themselves."""
    return BOUNDARY_DESCRIPTORS[desc] if isinstance(desc, str) else desc


def _descriptor_shape(desc):
    spec = AIRS.get(desc.get("air"), {})
    return desc.get("period", spec.get("period")), desc.get("n_cols", spec.get("n_cols"))


def _descriptor_args(desc):
    """The seven descriptor arguments of sp_boundary_dev / sp_boundary_points_dev (the arrays must outlive the call:
    the caller keeps the returned list)."""
    import ctypes
    period, n_cols = _descriptor_shape(desc)
    rows, terms = desc["rows"], desc["terms"]
    return [period.bit_length() - 1, n_cols, len(rows), (ctypes.c_uint * len(rows))(*rows), len(terms),
            (ctypes.c_uint * len(terms))(*[c for c, _ in terms]), (ctypes.c_uint * len(terms))(*[d for _, d in terms])]


def _inverses_mod(values, modulus):
    """[v^-1 mod modulus] behind ONE modular inversion (Montgomery's trick): prefix products up, the running inverse
    down.  Raises ValueError, as pow does, when a value has no inverse."""
    prefix, run = [], 1
    for v in values:
        prefix.append(run)
        run = run * v % modulus
    inv, out = pow(run, -1, modulus), [0] * len(prefix)
    for i in range(len(prefix) - 1, -1, -1):
        out[i] = inv * prefix[i] % modulus
        inv = inv * values[i] % modulus
    return out


def boundary_term_values(name, public_inputs):
    """The public list v_t of every term of a named descriptor from a proof's public inputs."""
    pub = list(public_inputs)
    if name == "ecdsa_io":  # [z, r, s, Qx, Qy] per signature; the third ladder's scalar is w = s^-1 mod N
        return [pub[0::5], pub[1::5], pub[3::5], pub[4::5], _inverses_mod(pub[2::5], EC_ORDER)]
    if name == "range_check_io":
        return [pub]
    if name == "pedersen_io":
        return [pub[0::3], pub[1::3], pub[2::3]]
    raise KeyError(name)


def _boundary_combined(desc, values, alphas, device):
    """[n_groups, k, 4]: per group sum_{t in d} a_t v_t[i] - k-sized work in Python integers, before any extension."""
    torch = _torch()
    assert len(values) == len(alphas) == len(desc["terms"]) and len({len(v) for v in values}) == 1
    cols = [[0] * len(values[0]) for _ in desc["rows"]]
    for (_, d), v, a in zip(desc["terms"], values, alphas):
        cols[d] = [(acc + a * int(x)) % FIELD_PRIME for acc, x in zip(cols[d], v)]
    return torch.stack([felts_to_tensor(c, device) for c in cols])


def boundary_public_lde(desc, values, n, alphas, shift=FIELD_GEN, device="cuda"):
    """[n_groups, 4n, 4]: C_d, the polynomial of degree < k = n / period through sum_{t in d} a_t v_t[i] over
    <g^period>, at x_j g^-o_d for x_j = shift w_4n^j.  `values` = one list of k felts per term, `alphas` the terms'
    challenges.  One sp_lde_dev call of k points at blowup 4 * period per group."""
    torch = _torch()
    desc = _descriptor(desc)
    period, _ = _descriptor_shape(desc)
    assert len(values[0]) == n // period
    g = _root_of_unity(n)
    comb = _boundary_combined(desc, values, alphas, device)
    return torch.stack([lde(comb[d].unsqueeze(0), period.bit_length() + 1,
                            shift * pow(g, -o, FIELD_PRIME) % FIELD_PRIME)[0] for d, o in enumerate(desc["rows"])])


def boundary(desc, trace_lde, pub_lde, n, alphas, shift=FIELD_GEN, acc=None, out=None):
    """out[j] = (acc[j] if acc is given else 0) + B(x_j) on the whole LDE coset (sp_boundary_dev): trace_lde the
    committed [n_cols, 4n, 4] trace LDE (the terms' columns are read), pub_lde from boundary_public_lde with the same
    alphas.  `out` may be `acc`."""
    torch = _torch()
    lib = _lib.ensure_init()
    desc = _descriptor(desc)
    M = 4 * n
    assert len(alphas) == len(desc["terms"]) and trace_lde.shape[0] == _descriptor_shape(desc)[1]
    assert trace_lde.shape[1] == M and tuple(pub_lde.shape) == (len(desc["rows"]), M, 4) and pub_lde.is_contiguous()
    _, _, stride = _table_shape(trace_lde)
    if out is None:
        out = torch.empty((M, 4), dtype=torch.int64, device=trace_lde.device)
    assert tuple(out.shape) == (M, 4) and out.is_contiguous() and (acc is None or (tuple(acc.shape) == (M, 4)
                                                                                    and acc.is_contiguous()))
    args = _descriptor_args(desc)
    _lib.check(lib.sp_boundary_dev(*args, trace_lde.data_ptr(), stride, pub_lde.data_ptr(), n.bit_length() - 1,
                                   pack_felts(alphas), pack_felts([shift]), None if acc is None else acc.data_ptr(),
                                   out.data_ptr(), _stream()), "sp_boundary_dev")
    return out


def boundary_coefficients(desc, values, n, alphas, device="cuda"):
    """[n_groups, k, 4]: the coefficients, in natural order, of the C_d (one inverse ntt call per group; at k = 1
    they are the values)."""
    torch = _torch()
    desc = _descriptor(desc)
    comb = _boundary_combined(desc, values, alphas, device)
    if comb.shape[1] == 1:
        return comb.contiguous()
    return torch.stack([ntt(col, inverse=True) for col in comb]).contiguous()


def boundary_points(desc, n, coef, alphas, shift, pos, cur):
    """B at arbitrary LDE positions from opened rows (sp_boundary_points_dev): coef [n_groups, k, 4] from
    boundary_coefficients with the same alphas, pos [q] int64 tensor of LDE indices, cur [q, n_cols, 4] the trace rows
    there.  Returns (out [q, 4], status [q] uint8): what boundary adds at those indices, and POINT_OK /
    POINT_OUT_OF_RANGE."""
    torch = _torch()
    lib = _lib.ensure_init()
    desc = _descriptor(desc)
    period, n_cols = _descriptor_shape(desc)
    q = pos.shape[0]
    assert len(alphas) == len(desc["terms"]) and coef.is_contiguous()
    assert tuple(coef.shape) == (len(desc["rows"]), n // period, 4)
    assert pos.dtype == torch.int64 and pos.is_contiguous() and cur.is_contiguous()
    assert tuple(cur.shape) == (q, n_cols, 4)
    out = torch.empty((q, 4), dtype=torch.int64, device=cur.device)
    status = torch.empty((q,), dtype=torch.uint8, device=cur.device)
    args = _descriptor_args(desc)
    _lib.check(lib.sp_boundary_points_dev(*args, n.bit_length() - 1, coef.data_ptr(), pack_felts(alphas),
                                          pack_felts([shift]), q, pos.data_ptr(), cur.data_ptr(), out.data_ptr(),
                                          status.data_ptr(), _stream()), "sp_boundary_points_dev")
    return out, status


def _prove_bound(name, trace, public, n_queries, seed, final_log, shift):
    """prove_trace with the boundary quotients of a named descriptor: `public` is absorbed, bound and published."""
    desc = BOUNDARY_DESCRIPTORS[name]
    n = trace.shape[1]
    values = boundary_term_values(name, public)

    def add_boundary(trace_lde, comp, alphas):
        pub_lde = boundary_public_lde(desc, values, n, alphas, shift, trace_lde.device)
        return boundary(desc, trace_lde, pub_lde, n, alphas, shift, acc=comp, out=comp)
    c = _commit_trace(trace, desc["air"], seed, final_log, shift, public, (name, len(desc["terms"]), add_boundary))
    return _query_trace(c, n_queries)


def prove_signatures(msg_hashes, rs, ss, public_keys, n_queries: int = 8, seed: int = 0, final_log: int = 6,
                     shift: int = FIELD_GEN, claims=None):
    """A proof of a statement: every (z_i, r_i, s_i, Q_i) of public_inputs = [z_0, r_0, s_0, Qx_0, Qy_0, z_1, ...] is
    a signature the reference's verify accepts.  Arguments as for prove_ecdsa (Python ints, a power-of-two count up
    to 2^14).  `claims`, when given, is the public-input list taken INSTEAD of the true one - in the transcript, the
    composition and FRI alike; it exists so that a test can make the prover lie consistently: such a proof is
    rejected ("final layer degree").

    What is bound, and was not by prove_ecdsa: on top of the 26 constraints of the ECDSA AIR five boundary terms with
    challenges of their own (31 alphas, AIR name "ecdsa_io") in three quotients tie the scalar column m at rows
    1024 i, 1024 i + 256 and 1024 i + 512 to z_i, r_i and w_i = s_i^-1 mod N, and qx, qy at row 1024 i + 256 to Q_i.
    With the AIR's own gbase, oncurve, addb, rload and fin constraints that is x(w_i (z_i G + r_i Q_i)) = r_i for
    every i.  The composition is sp_air_eval_ecdsa_dev plus sp_boundary_dev; commitments, FRI and the query phase are
    prove_trace's and the proof has its shape.  Verifier: verify_signatures (verify answers "malformed").

    What still is not: no zero knowledge, and Q queries at blowup 4 give about 2 Q bits of soundness."""
    dev = "cuda"
    k = len(msg_hashes)
    assert k >= 1 and k & (k - 1) == 0 and k <= 1 << 14 and len(rs) == len(ss) == len(public_keys) == k
    ws = [pow(s, -1, EC_ORDER) for s in ss]
    for z, r, w in zip(msg_hashes, rs, ws):
        assert 0 < z < 2**251 and 1 <= r < 2**251 and 1 <= w < 2**251
    trace = ecdsa_trace(*(felts_to_tensor(v, dev) for v in (msg_hashes, rs, ws, [q[0] for q in public_keys],
                                                          [q[1] for q in public_keys])))
    public = [v for z, r, s, q in zip(msg_hashes, rs, ss, public_keys) for v in (z, r, s, q[0], q[1])]
    if claims is not None:
        public = [int(v) for v in claims]
        assert len(public) == 5 * k
    return _prove_bound("ecdsa_io", trace, public, n_queries, seed, final_log, shift)


def prove_ranges(values, n_queries: int = 8, seed: int = 0, final_log: int = 6, shift: int = FIELD_GEN, claims=None):
    """A proof of a statement: every value of public_inputs lies in [0, 2^128).  Arguments as for prove_range_checks
    (a power-of-two count up to 2^17); `claims` as for prove_signatures.  On top of the two constraints of the
    range-check AIR one boundary quotient with a challenge of its own (3 alphas, AIR name "range_check_io") ties the
    column at row 128 i to value_i: the decomposed value is the published one.  Verifier: verify_ranges."""
    values = list(values)
    k = len(values)
    assert k >= 1 and k & (k - 1) == 0 and k <= 1 << 17
    for v in values:
        assert 0 <= v < FIELD_PRIME
    trace = range_check_trace(felts_to_tensor(values, "cuda"))
    public = values if claims is None else [int(v) for v in claims]
    assert len(public) == k
    return _prove_bound("range_check_io", trace, public, n_queries, seed, final_log, shift)


def _verify_bound(name, proof, final_log, n_queries):
    """The verifier core for a named descriptor of BOUNDARY_DESCRIPTORS: the statement rules are the base AIR's."""
    desc = BOUNDARY_DESCRIPTORS[name]

    def boundary_at(pub, n, alphas, shift, positions, cur, dev):
        coef = boundary_coefficients(desc, boundary_term_values(name, pub), n, alphas, dev)
        return boundary_points(desc, n, coef, alphas, shift, positions, cur)
    return _verify_trace_proof(proof, final_log, n_queries, name, desc["air"], _public_inputs_ok,
                               (len(desc["terms"]), boundary_at))


def verify_signatures(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of prove_signatures: (True, "ok") says that x(w_i (z_i G + r_i Q_i)) = r_i with w_i = s_i^-1 mod N for
    every (z_i, r_i, s_i, Qx_i, Qy_i) of proof["public_inputs"] - up to the soundness of the argument: about 2 Q
    bits for Q queries at blowup 4, and no zero knowledge.  Reasons, their order and the "malformed" rules are
    verify's, "public inputs" by the rules of the ECDSA AIR; a proof of another AIR is "malformed" here, as this AIR
    is for verify.

    Where it runs: as verify_hashes - the composition value of the 2 Q opened points is the sum (sp_felt_add_dev) of
    sp_air_eval_points_dev for the 26 AIR constraints and sp_boundary_points_dev for the three boundary quotients,
    which takes the coefficients of the three combined public polynomials from inverse ntt calls made once per proof;
    w_i is derived from s_i on the host."""
    return _verify_bound("ecdsa_io", proof, final_log, n_queries)


def verify_ranges(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of prove_ranges: (True, "ok") says that every value of proof["public_inputs"] lies in [0, 2^128) -
    the decomposed values are the published ones - up to the soundness of the argument.  A sibling of
    verify_signatures: the same reasons and rules, "public inputs" by the rules of the range-check AIR."""
    return _verify_bound("range_check_io", proof, final_log, n_queries)


# ---- the range-check builtin's encoding and ONE trace for the three builtins --------------------
# Definition: oracle/stark_ref.py ("rc16", BUILTIN_SEGMENTS, verify_builtins_proof).  The Cairo program is
# `%builtins output pedersen range_check ecdsa` (services/perpetual/cairo/main.cairo:1); no VM is needed for the
# builtin segments - the instance lists (hash inputs, signatures, range-checked values) are the input.
def rc16_fill(values, total_values):
    """values (each < 2^128) -> (padded list of total_values values, rc_min, rc_max); the padding values' limbs
    fill the holes of the limb range (the builtin's unused cells)."""
    pads, filler, lo, hi = _rc16_fill_parts(values, total_values)
    return list(values) + pads + [filler] * (total_values - len(values) - len(pads)), lo, hi


def _rc16_fill_parts(values, total_values):
    """(pads, filler, rc_min, rc_max) of rc16_fill: everything but the padded list itself."""
    limbs = set()
    for v in values:
        assert 0 <= v < 1 << 128
        for k in range(RC16_LIMBS):
            limbs.add((v >> (16 * k)) & 0xFFFF)
    lo, hi = min(limbs), max(limbs)
    holes = [x for x in range(lo, hi + 1) if x not in limbs]
    pads = []
    for i in range(0, len(holes), RC16_LIMBS):
        group = holes[i : i + RC16_LIMBS]
        group += [lo] * (RC16_LIMBS - len(group))
        pads.append(sum(l << (16 * (RC16_LIMBS - 1 - k)) for k, l in enumerate(group)))
    if len(values) + len(pads) > total_values:
        raise ValueError("the trace is too short to fill the %d holes of the limb range" % len(holes))
    filler = sum(lo << (16 * k) for k in range(RC16_LIMBS))
    return pads, filler, lo, hi


def rc16_fill_tensor(values, total_values, device="cuda"):
    """(padded [total_values, 4] device tensor, rc_min, rc_max): rc16_fill without total_values Python integers - the
    given values and the pads are converted, the filler is broadcast (NumPy)."""
    import numpy as np
    pads, filler, lo, hi = _rc16_fill_parts(values, total_values)
    head = list(values) + pads
    arr = np.empty((total_values, 4), dtype="<i8")
    arr[:] = np.frombuffer(filler.to_bytes(32, "little"), dtype="<i8")
    arr[:len(head)] = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in head), dtype="<i8").reshape(-1, 4)
    return _torch().from_numpy(arr).to(device), lo, hi


def rc16_columns(values):
    """values: [k, 4] device tensor (already padded, rc16_fill) -> [3, 8 k, 4]: a (limb), acc (running value), s
    (the limb column sorted)."""
    torch = _torch()
    lib = _lib.ensure_init()
    k = values.shape[0]
    cols = torch.zeros((3, RC16_LIMBS * k, 4), dtype=torch.int64, device=values.device)
    _lib.check(lib.sp_rc16_trace_dev(values.data_ptr(), k, cols.data_ptr(), _stream()), "sp_rc16_trace_dev")
    cols[2, :, 0] = torch.sort(cols[0, :, 0]).values  # limbs are < 2^16: the low word is the felt
    return cols


def rc16_product(a, s, z):
    """The second-phase column p_i = prod_{j <= i} (z - a_j) / (z - s_j) (a, s: [n, 4] device tensors)."""
    torch = _torch()
    lib = _lib.ensure_init()
    n = a.shape[0]
    p = torch.empty((n, 4), dtype=torch.int64, device=a.device)
    _lib.check(lib.sp_rc16_product_dev(a.contiguous().data_ptr(), s.contiguous().data_ptr(), n, pack_felts([z]),
                                       p.data_ptr(), _stream()), "sp_rc16_product_dev")
    return p


def air_eval_rc16(cols_lde, p_lde, per_lde, n, alphas, z, rc_min, rc_max, shift=FIELD_GEN):
    torch = _torch()
    lib = _lib.ensure_init()
    assert cols_lde.shape[0] == 3 and cols_lde.shape[1] == 4 * n and len(alphas) == N_RC16_CONSTRAINTS
    out = torch.empty((4 * n, 4), dtype=torch.int64, device=cols_lde.device)
    _lib.check(lib.sp_air_eval_rc16_dev(cols_lde.data_ptr(), p_lde.data_ptr(), per_lde.data_ptr(), n.bit_length() - 1,
                                        pack_felts(alphas), pack_felts([shift]), pack_felts([z]), rc_min, rc_max,
                                        out.data_ptr(), _stream()), "sp_air_eval_rc16_dev")
    return out


def felt_add(a, b):
    torch = _torch()
    lib = _lib.ensure_init()
    out = torch.empty_like(a)
    _lib.check(lib.sp_felt_add_dev(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], _stream()), "sp_felt_add_dev")
    return out


def _cycle(items, count):
    return [items[i % len(items)] for i in range(count)]


def prove_builtins(hash_inputs=None, signatures=None, rc_values=None, n_queries: int = 8, seed: int = 0,
                   final_log: int = 6, shift: int = FIELD_GEN, log_rows: int = None):
    """ONE trace, ONE composition, ONE proof for the builtin usage of a batch: Pedersen hashes
    (hash_inputs: [(x, y)]), ECDSA verifications (signatures: [(z, r, s, (Qx, Qy))]) and range checks (rc_values:
    ints < 2^128) laid side by side at fixed ratios - per 1024 rows two hashes, one verification and 128 rc16
    cells (16 values).  The trace length is the power of two the largest segment needs; the other segments repeat
    their instances (unused builtin cells).  Two committed phases: the builtin columns, then - after the
    challenge z - the permutation product of the range-check segment.  Benchmark-grade like prove_trace (no
    boundary constraint ties the instances to the public inputs except rc_min / rc_max; ~2 bits per query;
    prove_builtin_usage is this proof with its hashes, signatures and values bound).
    Verifier: verify_builtins (on the GPU; its oracle is oracle/stark_ref.verify_builtins_proof)."""
    return _query_builtins(_commit_builtins(hash_inputs, signatures, rc_values, seed, final_log, shift, log_rows),
                           n_queries)


def _commit_builtins(hash_inputs, signatures, rc_values, seed, final_log, shift, log_rows, statement=None):
    """The commit phase of prove_builtins (both committed phases, the composition, the FRI layers); returns what the
    query phase needs.  `statement` (prove_builtin_usage), the hook _commit_trace has: a function of what the prover
    holds once the trace stands - n, the segments, the trace, the instance tensors it was built from - that returns
    (name, public, flat_pub, n_extra, add): the AIR name, the public inputs and their flat transcript list taken
    instead of this function's, how many challenges are drawn after the AIRs' own in the same way, and
    add(trace_lde, comp, extra_alphas) -> comp of what they bring to the composition."""
    torch = _torch()
    dev = "cuda"
    P = FIELD_PRIME
    segments = [name for name, arg in zip(BUILTIN_SEGMENTS, (hash_inputs, signatures, rc_values)) if arg]
    assert segments, "no builtin instance given"
    need = 8
    if hash_inputs:
        need = max(need, 512 * len(hash_inputs))
    if signatures:
        need = max(need, 1024 * len(signatures))
    rc_need = 0
    if rc_values:
        limbs = {(v >> (16 * k)) & 0xFFFF for v in rc_values for k in range(RC16_LIMBS)}
        rc_need = len(rc_values) + -(-(max(limbs) - min(limbs) + 1 - len(limbs)) // RC16_LIMBS)
        need = max(need, RC16_LIMBS * rc_need)
    n = 1 << max((need - 1).bit_length(), log_rows or 0)
    M = n << BLOWUP_LOG
    groups, public, flat_pub = [], {}, [len(segments)] + [BUILTIN_SEGMENTS.index(s) for s in segments]
    rc_min = rc_max = 0
    if rc_values:
        padded, rc_min, rc_max = rc16_fill(list(rc_values), n // RC16_LIMBS)
        public.update({"rc_min": rc_min, "rc_max": rc_max})
        flat_pub += [rc_min, rc_max]
    if signatures:
        sigs = _cycle(list(signatures), n // 1024)
        ws = [pow(s_, -1, EC_ORDER) for _, _, s_, _ in sigs]
        for (z_, r_, _, _), w_ in zip(sigs, ws):
            assert 0 < z_ < 2**251 and 1 <= r_ < 2**251 and 1 <= w_ < 2**251
        public["signatures"] = [[z_, r_, s_, q[0], q[1]] for z_, r_, s_, q in sigs]
        flat_pub += [v for sig in public["signatures"] for v in sig]
    held = {"n": n, "segments": segments}  # what a statement hook may read
    if hash_inputs:
        hs = _cycle(list(hash_inputs), n // 512)
        held["hashes"] = hs
        held["hash_xy"] = (felts_to_tensor([x for x, _ in hs], dev), felts_to_tensor([y for _, y in hs], dev))
        groups.append(pedersen_trace(*held["hash_xy"]))
    if signatures:
        held["sig_zrwq"] = tuple(felts_to_tensor(v, dev) for v in (
            [z_ for z_, _, _, _ in sigs], [r_ for _, r_, _, _ in sigs], ws, [q[0] for *_, q in sigs],
            [q[1] for *_, q in sigs]))
        groups.append(ecdsa_trace(*held["sig_zrwq"]))
    if rc_values:
        held["rc_padded"] = felts_to_tensor(padded, dev)
        groups.append(rc16_columns(held["rc_padded"]))
    trace = torch.cat(groups)
    del groups
    n_cols = trace.shape[0]
    name, n_extra, add = "builtins", 0, None
    if statement is not None:
        held["trace"] = trace
        name, public, flat_pub, n_extra, add = statement(dict(held, public=public))
        rc_min, rc_max = public.get("rc_min", rc_min), public.get("rc_max", rc_max)  # a lying claim, consistently
    del held
    tr = Transcript(name, n, shift, seed, flat_pub)
    # ---- phase 1: the builtin columns ----
    trace_lde = lde(trace)
    lv1 = commit_rows(trace_lde)
    root1 = root_of(lv1)
    tr.absorb("phase1_root", root1)
    # ---- phase 2: the permutation product of the range-check segment, after its challenge ----
    z, p_lde, lv2, root2 = 0, None, None, None
    if rc_values:
        z = tr.challenge("rc16_z")
        p = rc16_product(trace[n_cols - 3], trace[n_cols - 1], z)
        p_lde = lde(p.unsqueeze(0))[0]
        lv2 = commit_rows(p_lde.unsqueeze(0))
        root2 = root_of(lv2)
        tr.absorb("phase2_root", root2)
    del trace
    n_alphas = sum(AIRS[s]["n_constraints"] for s in segments)
    alphas = [tr.challenge("alpha", k) for k in range(n_alphas + n_extra)]
    comp, c0, a0 = None, 0, 0
    for seg in segments:
        spec = AIRS[seg]
        sl = trace_lde[c0 : c0 + spec["n_cols"]]
        al = alphas[a0 : a0 + spec["n_constraints"]]
        per = periodic_lde(n, shift, dev, seg)
        part = (air_eval_rc16(sl, p_lde, per, n, al, z, rc_min, rc_max, shift) if seg == "rc16"
                else air_eval(sl, per, n, al, shift, seg))
        comp = part if comp is None else felt_add(comp, part)
        c0 += spec["n_cols"]
        a0 += spec["n_constraints"]
    if add is not None:
        comp = add(trace_lde, comp, alphas[n_alphas:])
    layers, level_bufs, roots = [comp], [], []
    s = shift
    while True:
        cur = layers[-1]
        lv = commit_rows(cur.unsqueeze(0))
        level_bufs.append(lv)
        roots.append(root_of(lv))
        tr.absorb("layer_root", roots[-1])
        beta = tr.challenge("beta", len(roots))
        nxt = fri_fold(cur, beta, s)
        s = s * s % P
        layers.append(nxt)
        if nxt.shape[0] <= (1 << final_log):
            break
    final = tensor_to_felts(layers[-1])
    tr.absorb("final_layer", *final)
    return {"tr": tr, "M": M, "trace_lde": trace_lde, "lv1": lv1, "p_lde": p_lde, "lv2": lv2, "layers": layers,
            "level_bufs": level_bufs,
            "head": {"n": n, "air": name, "segments": segments, "seed": seed, "shift": shift,
                     "public_inputs": public, "phase1_root": root1, "phase2_root": root2, "layer_roots": roots,
                     "final_layer": final}}


def _query_builtins(c, n_queries, opener=None):
    """The query phase of prove_builtins, shaped as _query_trace: per query four phase-1 rows, the same four rows of
    phase 2 when it exists, one pair per layer - all picks of the proof in ONE opener call."""
    opener = opener or open_rows
    M, layers, two = c["M"], c["layers"][:-1], c["lv2"] is not None
    tables = [(c["trace_lde"], c["lv1"])] + ([(c["p_lde"], c["lv2"])] if two else [])
    first_layer = len(tables)
    tables += list(zip(layers, c["level_bufs"]))
    indices = [c["tr"].challenge("query", q, modulus=M // 2) for q in range(n_queries)]
    picks = []
    for j in indices:
        for pos in (j, j + M // 2):
            for row in (pos, (pos + (1 << BLOWUP_LOG)) % M):
                picks.append((0, row))
                if two:
                    picks.append((1, row))
        for k, pair in enumerate(_layer_positions(j, layers)):
            picks += [(first_layer + k, pos) for pos in pair]
    opened = iter(zip(picks, opener(tables, picks)))
    queries = []
    for j in indices:
        entry = {"index": j, "phase1": [], "phase2": [], "layers": []}
        for _ in range(4):
            (_, row), (values, _, path) = next(opened)
            entry["phase1"].append({"row": row, "values": values, "path": path})
            if two:
                (_, row), (values, _, path) = next(opened)
                entry["phase2"].append({"row": row, "value": values[0], "path": path})
        for _ in layers:
            pair = []
            for _ in range(2):
                (_, pos), (values, _, path) = next(opened)
                pair.append({"pos": pos, "value": values[0], "path": path})
            entry["layers"].append(pair)
        queries.append(entry)
    return dict(c["head"], queries=queries)


# ---- the verifier of prove_builtins proofs ----------------------------------------------------------------------
# Product twin of oracle/stark_ref.verify_builtins_proof: the same checks in the same order with the same reasons.
# Host: the transcript and the integer comparisons.  Device: every hash (check_builtins_openings, two calls), the
# 2 Q composition values over all segments (ONE sp_builtins_eval_points_dev launch, csrc/verify_builtins.hip), the
# Q n_layers fold steps (ONE sp_fri_check_queries_dev launch), the final layer's coefficients (ntt).
SEG_BITS = {"pedersen": 1, "ecdsa": 2, "rc16": 4}  # SP_SEG_* of include/starkperp.h


def builtins_eval_points(segments, n, pers, alphas, shift, z, rc_min, rc_max, pos, cur, nxt, pcur=None, pnxt=None):
    """The composition value of a combined builtin trace at arbitrary LDE positions from opened rows
    (sp_builtins_eval_points_dev): `segments` the list of names as in a proof, `pers` a dict from name to its
    periodic_lde table, `alphas` the 11 + 26 + 8 of the present segments in that order, pos [k] int64 tensor of LDE
    indices, cur / nxt [k, n_cols, 4] the phase-1 rows at pos and at (pos + 4) mod 4n, pcur / pnxt [k, 4] the
    phase-2 column at those rows (with rc16 only; z, rc_min, rc_max are read only then).  Returns (out [k, 4],
    status [k] uint8): what _commit_builtins builds at those indices, and POINT_OK / POINT_OUT_OF_RANGE per point."""
    torch = _torch()
    lib = _lib.ensure_init()
    segments = list(segments)
    assert segments and segments == [s for s in BUILTIN_SEGMENTS if s in segments]
    n_cols = sum(AIRS[s]["n_cols"] for s in segments)
    k = pos.shape[0]
    assert len(alphas) == sum(AIRS[s]["n_constraints"] for s in segments)
    assert tuple(cur.shape) == tuple(nxt.shape) == (k, n_cols, 4)
    assert pos.dtype == torch.int64 and pos.is_contiguous() and cur.is_contiguous() and nxt.is_contiguous()
    has_rc = "rc16" in segments
    if has_rc:
        assert tuple(pcur.shape) == tuple(pnxt.shape) == (k, 4) and pcur.is_contiguous() and pnxt.is_contiguous()
    tables = [pers[s].data_ptr() if s in segments else None for s in BUILTIN_SEGMENTS]
    out = torch.empty((k, 4), dtype=torch.int64, device=cur.device)
    status = torch.empty((k,), dtype=torch.uint8, device=cur.device)
    _lib.check(lib.sp_builtins_eval_points_dev(
        sum(SEG_BITS[s] for s in segments), n.bit_length() - 1, tables[0], tables[1], tables[2], pack_felts(alphas),
        pack_felts([shift]), pack_felts([z]) if has_rc else None, rc_min if has_rc else 0, rc_max if has_rc else 0, k,
        pos.data_ptr(), cur.data_ptr(), nxt.data_ptr(), pcur.data_ptr() if has_rc else None,
        pnxt.data_ptr() if has_rc else None, out.data_ptr(), status.data_ptr(), _stream()),
        "sp_builtins_eval_points_dev")
    return out, status


def check_builtins_openings(proof) -> List[Tuple[str, bool]]:
    """check_merkle_openings for a prove_builtins proof: one (label, ok) per opening in proof order - per query the
    four phase-1 rows, each followed by its phase-2 value when the proof has a second phase, then the layer pairs -
    labelled "q3/phase1/row 517" (against phase1_root), "q3/phase2/row 517" (against phase2_root; the leaf is the
    value itself, the table has one column) and "q3/layer 2/pos 40" (against layer_roots[2]).  The same two library
    calls: one ragged chain call hashes the leaves of the phase-1 rows, ONE sp_merkle_verify_paths call with offsets
    and per-item expected roots checks every path.  A value outside [0, p) makes its opening False; so does a
    phase-1 row without values.  The Merkle part ONLY: the rest is verify_builtins's."""
    import numpy as np
    from . import batch_np
    P = FIELD_PRIME
    felt = lambda v: v if 0 <= v < 2**256 else P  # unrepresentable: p itself, which the device flags as out of range
    two = proof.get("phase2_root") is not None
    labels, keys, expected, paths, leaves = [], [], [], [], []
    rows, row_slot, empty = [], [], []  # the chains of the phase-1 rows and the openings they belong to

    def add(label, key, root, path, leaf):
        labels.append(label)
        keys.append(key)
        expected.append(root)
        paths.append([felt(v) for v in path])
        leaves.append(leaf)

    for qi, q in enumerate(proof["queries"]):
        phase2 = iter(q["phase2"]) if two else None
        for t in q["phase1"]:
            row_slot.append(len(labels))
            empty.append(len(t["values"]) == 0)
            rows.append([felt(v) for v in t["values"]] or [0])
            add("q%d/phase1/row %d" % (qi, t["row"]), t["row"], proof["phase1_root"], t["path"], 0)
            t2 = next(phase2, None) if two else None
            if t2 is not None:
                add("q%d/phase2/row %d" % (qi, t2["row"]), t2["row"], proof["phase2_root"], t2["path"], felt(t2["value"]))
        for t2 in phase2 or ():  # more phase-2 openings than phase-1 rows: still in proof order
            add("q%d/phase2/row %d" % (qi, t2["row"]), t2["row"], proof["phase2_root"], t2["path"], felt(t2["value"]))
        for k, pair in enumerate(q["layers"]):
            for o in pair:
                add("q%d/layer %d/pos %d" % (qi, k, o["pos"]), o["pos"], proof["layer_roots"][k], o["path"], felt(o["value"]))
    n = len(labels)
    if n == 0:
        return []
    leaf_arr = batch_np.felts_from_ints(leaves)
    leaf_bad = np.zeros(n, dtype=bool)
    if rows:
        row_off = np.zeros(len(rows) + 1, dtype=np.uint32)
        row_off[1:] = np.cumsum([len(r) for r in rows])
        hashed, row_st = batch_np.pedersen_chains_ragged(batch_np.felts_from_ints([v for r in rows for v in r]), row_off)
        slots = np.array(row_slot)
        bad = (row_st != 0) | np.array(empty)
        leaf_arr[slots] = hashed
        leaf_bad[slots] = bad
        leaf_arr[slots[bad]] = 0  # what a failed chain leaves is unspecified; the opening is False anyway
    # a position that does not fit its path's height cannot be opened by it
    fits = np.array([len(p) <= 64 and 0 <= k < (1 << len(p)) for k, p in zip(keys, paths)])
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) if f else 0 for p, f in zip(paths, fits)])
    flat = [v for p, f in zip(paths, fits) if f for v in p]
    sib = batch_np.felts_from_ints(flat) if flat else np.zeros((0, 4), dtype=np.uint64)
    key_arr = np.array([k if f else 0 for k, f in zip(keys, fits)], dtype=np.uint64)
    verdict, _ = batch_np.merkle_verify_paths(leaf_arr, sib, key_arr, batch_np.felts_from_ints([felt(v) for v in expected]),
                                              offsets=off)
    ok = verdict & fits & ~leaf_bad
    return list(zip(labels, [bool(v) for v in ok]))


def _wellformed_builtins(proof, name="builtins"):
    """_wellformed for a prove_builtins proof: the keys and types, every felt in [0, p), every integer an int, every
    path of its tree's height.  What the oracle answers with a reason - the segment list's contents, the public
    inputs' values, the lengths of layer_roots and final_layer, the number of values of a phase-1 row - is left to
    verify_builtins.  With name = "builtins_io" (prove_builtin_usage) the proof must carry that name and the public
    inputs the bound statement adds, every one an integer below 2^256."""
    if not isinstance(proof, dict) or proof.get("air", "builtins" if name == "builtins" else None) != name:
        return False
    segments, n, shift = proof.get("segments"), proof.get("n"), proof.get("shift")
    if not (isinstance(segments, (list, tuple)) and all(isinstance(s, str) for s in segments)):
        return False
    has_rc = "rc16" in segments
    # 2^24 rows is the bound of the dense rc16 composition: no prover made a longer proof with that segment
    if not (_is_int(n) and 1 <= n <= 1 << (24 if has_rc else 30) and n & (n - 1) == 0):
        return False
    if not (_is_felt(shift) and shift != 0 and pow(shift, 4 * n, FIELD_PRIME) != 1):
        return False
    if not (_is_int(proof.get("seed")) and 0 <= proof["seed"] < 1 << 256 and _is_felt(proof.get("phase1_root"))):
        return False
    if has_rc and not _is_felt(proof.get("phase2_root")):
        return False
    pub = proof.get("public_inputs")
    if not isinstance(pub, dict):
        return False
    if has_rc and not (_is_int(pub.get("rc_min")) and _is_int(pub.get("rc_max"))):
        return False
    if "ecdsa" in segments:
        sigs = pub.get("signatures")
        if not (isinstance(sigs, (list, tuple)) and all(
                isinstance(sig, (list, tuple)) and len(sig) == 5 and all(_is_int(v) and 0 <= v < 1 << 256 for v in sig)
                for sig in sigs)):
            return False
    if name == BUILTINS_IO_AIR:
        word = lambda v: _is_int(v) and 0 <= v < 1 << 256
        if has_rc and not (isinstance(pub.get("rc_values"), (list, tuple)) and all(word(v) for v in pub["rc_values"])):
            return False
        if "pedersen" in segments and not (isinstance(pub.get("hashes"), (list, tuple)) and all(
                isinstance(t, (list, tuple)) and len(t) == 3 and all(word(v) for v in t) for t in pub["hashes"])):
            return False
    if not (_felt_list(proof.get("layer_roots")) and _felt_list(proof.get("final_layer"))):
        return False
    queries = proof.get("queries")
    if not isinstance(queries, (list, tuple)):
        return False
    log_m = n.bit_length() + 1
    for q in queries:
        if not (isinstance(q, dict) and _is_int(q.get("index")) and isinstance(q.get("phase1"), (list, tuple))
                and isinstance(q.get("phase2"), (list, tuple)) and isinstance(q.get("layers"), (list, tuple))
                and len(q["phase1"]) == 4 and (len(q["phase2"]) == 4 or not has_rc)):
            return False
        for t in q["phase1"]:
            if not (isinstance(t, dict) and _is_int(t.get("row")) and _felt_list(t.get("values"))
                    and _felt_list(t.get("path"), log_m)):
                return False
        for t in q["phase2"] if has_rc else ():  # without rc16 nothing reads the second phase
            if not (isinstance(t, dict) and _is_int(t.get("row")) and _is_felt(t.get("value"))
                    and _felt_list(t.get("path"), log_m)):
                return False
        for k, pair in enumerate(q["layers"]):
            if not (isinstance(pair, (list, tuple)) and len(pair) == 2):
                return False
            for o in pair:
                if not (isinstance(o, dict) and _is_int(o.get("pos")) and _is_felt(o.get("value"))
                        and _felt_list(o.get("path"), max(log_m - k, 0))):
                    return False
    return True


def verify_builtins(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of prove_builtins proofs: returns (ok, reason) with the reasons of
    oracle/stark_ref.verify_builtins_proof, the first failure in that function's order - "segments", "public inputs"
    (the rc16 limb range, the signatures' side conditions, n against each segment's period), "shape" (also fewer
    than one layer, and a given `n_queries` that is not the number of queries), "final layer degree", then per query
    "query index", "opened rows", "phase 1 path", "phase 2 path", "composition value" and per layer "layer
    positions", "layer path", "fold consistency at layer k" - or (True, "ok").  `final_log` is the prover's.

    Where it runs: the SHA-256 transcript - the flattened public inputs exactly as the prover absorbs them, then
    phase1_root, the challenge rc16_z, phase2_root, the alphas, the betas, the query indices - and the comparisons of
    indices, rows and positions on the host; every hash on the GPU through check_builtins_openings (two calls); the
    composition value of the 2 Q opened points, summed over the segments, in ONE sp_builtins_eval_points_dev launch
    and the Q n_layers fold steps in ONE sp_fri_check_queries_dev launch; the final layer's coefficients through
    ntt.  Everything is computed, then the first failure is reported.  A phase-1 row with the wrong number of values
    is "opened rows" at that row's turn; the composition launch covers the queries before the first such query.
    Without rc16 there is no second phase: phase2 is empty, phase2_root None and z = 0.

    A malformed proof - a missing key, a non-integer, a felt outside [0, p), a path of the wrong length, `segments`
    not a list of strings, `public_inputs` not the dict the segments need, an n that is no power of two, a shift
    that is 0 or puts the coset onto the trace domain - returns (False, "malformed") before the library is
    initialised: nothing raises and no such value reaches the device.

    The caveat of prove_trace holds here too: this verifies a benchmark-grade argument, NOT a sound proof system -
    no boundary constraint binds the instances to the public inputs except rc_min / rc_max (the rest is only
    absorbed, and checked as the oracle does), and Q queries at blowup 4 give about 2 Q bits."""
    return _verify_builtins_proof(proof, final_log, n_queries)


def _verify_builtins_proof(proof, final_log, n_queries, statement=None):
    """The one verifier of prove_builtins-shaped proofs; verify_builtins and verify_builtin_usage are its wrappers and
    document it.  `statement`, when given, is (name, public_ok, flat, n_extra, boundary_at) - what _verify_trace_proof
    takes as `name` and `boundary`: the AIR name the proof and the transcript carry; public_ok(pub, n, segments), the
    statement's further rules ("public inputs", after the unbound proof's own); flat(pub, segments), the transcript
    list; n_extra(segments) more alphas drawn after the AIRs' own; and boundary_at(pub, n, segments, extra_alphas,
    shift, positions, cur, dev) -> (values, status) at the opened points, added to the composition value
    (sp_felt_add_dev), its status ORed into the points'."""
    name, public_ok, flat_of, n_extra_of, boundary_at = statement or ("builtins", None, None, None, None)
    try:
        if not (_wellformed_builtins(proof, name) and _is_int(final_log) and 0 <= final_log <= 30):
            return False, "malformed"
    except Exception:  # an object that misbehaves when inspected is malformed too
        return False, "malformed"
    n, seed, shift, segments = proof["n"], proof["seed"], proof["shift"], list(proof["segments"])
    if not segments or segments != [s for s in BUILTIN_SEGMENTS if s in segments]:
        return False, "segments"
    n_cols = sum(AIRS[s]["n_cols"] for s in segments)
    n_alphas = sum(AIRS[s]["n_constraints"] for s in segments)
    has_rc = "rc16" in segments
    pub = proof["public_inputs"]
    rc_min = rc_max = 0
    if has_rc:
        rc_min, rc_max = pub["rc_min"], pub["rc_max"]
        if not 0 <= rc_min <= rc_max < 1 << 16 or n % RC16_LIMBS:
            return False, "public inputs"
    if "ecdsa" in segments:
        sigs = pub["signatures"]
        if n % 1024 or len(sigs) != n // 1024 or not _public_inputs_ok("ecdsa", n, [v for sig in sigs for v in sig]):
            return False, "public inputs"
    if "pedersen" in segments and n % 512:
        return False, "public inputs"
    if public_ok is not None and not public_ok(pub, n, segments):
        return False, "public inputs"
    m = n << BLOWUP_LOG
    log_m = m.bit_length() - 1
    queries = proof["queries"]
    n_layers = log_m - final_log
    reason = _fri_shape_reason(proof, n_layers, final_log, n_queries)
    if reason:
        return False, reason
    if flat_of is not None:
        flat_pub = flat_of(pub, segments)
    else:
        flat_pub = [len(segments)] + [BUILTIN_SEGMENTS.index(s) for s in segments]
        if has_rc:
            flat_pub += [rc_min, rc_max]
        if "ecdsa" in segments:
            flat_pub += [v for sig in pub["signatures"] for v in sig]
    n_extra = n_extra_of(segments) if n_extra_of else 0
    tr = Transcript(name, n, shift, seed, flat_pub)
    tr.absorb("phase1_root", proof["phase1_root"])
    z = 0
    if has_rc:
        z = tr.challenge("rc16_z")
        tr.absorb("phase2_root", proof["phase2_root"])
    alphas = [tr.challenge("alpha", k) for k in range(n_alphas + n_extra)]
    betas, indices = _replay_fri_challenges(tr, proof, m)
    torch = _torch()
    final_t = felts_to_tensor(proof["final_layer"])
    reason = _final_layer_reason(final_t, n, n_layers)
    if reason:
        return False, reason
    if not queries:
        return True, "ok"
    openings = iter(check_builtins_openings(dict(proof, phase2_root=proof["phase2_root"] if has_rc else None)))
    dev = final_t.device
    # the composition launch stops before the first query with an ill-shaped phase-1 row: the answer is "opened
    # rows" at that row's turn at the latest
    shaped = 0
    while shaped < len(queries) and all(len(t["values"]) == n_cols for t in queries[shaped]["phase1"]):
        shaped += 1
    comp, comp_st = [], []
    if shaped:
        head = queries[:shaped]
        pers = {s: periodic_lde(n, shift, dev, s) for s in segments}
        positions = [pos for j in indices[:shaped] for pos in (j, j + m // 2)]
        cur = felts_to_tensor([v for q in head for side in (0, 1) for v in q["phase1"][2 * side]["values"]], dev)
        nxt = felts_to_tensor([v for q in head for side in (0, 1) for v in q["phase1"][2 * side + 1]["values"]], dev)
        pcur = pnxt = None
        if has_rc:
            pcur = felts_to_tensor([q["phase2"][2 * side]["value"] for q in head for side in (0, 1)], dev)
            pnxt = felts_to_tensor([q["phase2"][2 * side + 1]["value"] for q in head for side in (0, 1)], dev)
        shape = (len(positions), n_cols, 4)
        positions = torch.tensor(positions, dtype=torch.int64, device=dev)
        cur = cur.reshape(shape)
        comp, comp_st = builtins_eval_points(segments, n, pers, alphas[:n_alphas], shift, z, rc_min, rc_max, positions,
                                             cur, nxt.reshape(shape), pcur, pnxt)
        if boundary_at is not None:
            bnd, bnd_st = boundary_at(pub, n, segments, alphas[n_alphas:], shift, positions, cur, dev)
            comp, comp_st = felt_add(comp, bnd), comp_st | bnd_st
    fold_st = _fold_statuses(queries, indices, betas, shift, log_m, final_t, dev)
    if shaped:
        comp, comp_st = tensor_to_felts(comp), comp_st.cpu().tolist()
    for qi, (q, j) in enumerate(zip(queries, indices)):
        phase1_ok, phase2_ok = [], []
        for _ in range(4):
            phase1_ok.append(next(openings)[1])
            if has_rc:
                phase2_ok.append(next(openings)[1])
        layer_ok = [[next(openings)[1] for _ in range(2)] for _ in range(n_layers)]
        if q["index"] != j:
            return False, "query index"
        want_rows = [j, (j + 4) % m, j + m // 2, (j + m // 2 + 4) % m]
        if [t["row"] for t in q["phase1"]] != want_rows or (has_rc and [t["row"] for t in q["phase2"]] != want_rows):
            return False, "opened rows"
        for t, ok in zip(q["phase1"], phase1_ok):
            if len(t["values"]) != n_cols:
                return False, "opened rows"
            if not ok:
                return False, "phase 1 path"
        if not all(phase2_ok):
            return False, "phase 2 path"
        reason = _composition_reason(q, qi, comp, comp_st) or _layers_reason(q, j, m, layer_ok, fold_st[qi])
        if reason:
            return False, reason
    return True, "ok"


# ---- the builtins proof bound to its statement: hashes, signatures, range-checked values --------------------------
# DESIGN.md 6.6.  Every present segment of the combined trace brings the boundary groups of its descriptor - pedersen_io,
# ecdsa_io, rc16_io - with challenges of its own (3 + 5 + 1, drawn after the 11 + 26 + 8 of the AIRs); B is the sum over
# all groups, each with its own segment's period.  Definition in integers: tests/builtins_io_ref.py (on
# oracle/stark_ref.py and tests/boundary_ref.py); kernels: csrc/builtins_boundary.hip.
BUILTINS_IO_AIR = "builtins_io"
BUILTIN_BOUNDARY = {"pedersen": "pedersen_io", "ecdsa": "ecdsa_io", "rc16": "rc16_io"}  # segment -> its descriptor


def _builtin_boundary_shape(segments):
    """(terms, groups) of the present segments' descriptors together."""
    descs = [BOUNDARY_DESCRIPTORS[BUILTIN_BOUNDARY[s]] for s in segments]
    return sum(len(d["terms"]) for d in descs), sum(len(d["rows"]) for d in descs)


def _ordered_segments(segments):
    segments = list(segments)
    assert segments and segments == [s for s in BUILTIN_SEGMENTS if s in segments]
    return segments


def boundary_combine(term_groups, n_groups, columns, alphas):
    """[n_groups, k, 4]: out[d][i] = sum_{t in d} a_t v_t[i] mod p on the device (sp_boundary_combine_dev) - what
    _boundary_combined does in Python integers, bit for bit.  `columns`: one [k, 4] device tensor per term (any layout;
    made contiguous here), term_groups[t] the term's group."""
    import ctypes
    torch = _torch()
    lib = _lib.ensure_init()
    columns = [c.contiguous() for c in columns]
    k = columns[0].shape[0]
    assert len(columns) == len(alphas) == len(term_groups) and all(tuple(c.shape) == (k, 4) for c in columns)
    out = torch.empty((n_groups, k, 4), dtype=torch.int64, device=columns[0].device)
    _lib.check(lib.sp_boundary_combine_dev(n_groups, len(columns), (ctypes.c_uint * len(columns))(*term_groups),
                                           (ctypes.c_void_p * len(columns))(*[c.data_ptr() for c in columns]), k,
                                           pack_felts(alphas), out.data_ptr(), _stream()), "sp_boundary_combine_dev")
    return out


def _builtin_combined(segments, columns, alphas):
    """Per present segment the [n_groups, k_s, 4] combined public columns; `columns`: segment -> its terms' tensors."""
    out, a0 = [], 0
    for seg in segments:
        terms = BOUNDARY_DESCRIPTORS[BUILTIN_BOUNDARY[seg]]["terms"]
        out.append(boundary_combine([d for _, d in terms], 1 + max(d for _, d in terms), columns[seg],
                                    alphas[a0 : a0 + len(terms)]))
        a0 += len(terms)
    return out


def builtins_boundary_public_lde(segments, columns, n, alphas, shift=FIELD_GEN):
    """[3 + 3 + 1, 4n, 4] of the present segments: per group C_d at x_j g^-o_d.  The terms' public columns are combined
    on the device, then ONE sp_lde_dev call per group writes its column of the result (k_s points at blowup 4 p_s)."""
    torch = _torch()
    lib = _lib.ensure_init()
    segments = _ordered_segments(segments)
    g = _root_of_unity(n)
    combined = _builtin_combined(segments, columns, alphas)
    out = torch.empty((_builtin_boundary_shape(segments)[1], 4 * n, 4), dtype=torch.int64, device=combined[0].device)
    at = 0
    for seg, comb in zip(segments, combined):
        period = AIRS[seg]["period"]
        assert comb.shape[1] == n // period
        for d, o in enumerate(BOUNDARY_DESCRIPTORS[BUILTIN_BOUNDARY[seg]]["rows"]):
            _lib.check(lib.sp_lde_dev(comb[d].data_ptr(), out[at].data_ptr(), 1, comb.shape[1].bit_length() - 1,
                                      period.bit_length() + 1, pack_felts([shift * pow(g, -o, FIELD_PRIME) % FIELD_PRIME]),
                                      _stream()), "sp_lde_dev")
            at += 1
    return out


def builtins_boundary(segments, trace_lde, pub_lde, n, alphas, shift=FIELD_GEN, acc=None, out=None):
    """out[j] = (acc[j] if acc is given else 0) + B(x_j) on the whole LDE coset (sp_builtins_boundary_dev): trace_lde
    the committed phase-1 LDE of the present segments, pub_lde from builtins_boundary_public_lde with the same
    alphas.  `out` may be `acc`."""
    torch = _torch()
    lib = _lib.ensure_init()
    segments = _ordered_segments(segments)
    M = 4 * n
    n_terms, n_groups = _builtin_boundary_shape(segments)
    assert len(alphas) == n_terms and trace_lde.shape[0] == sum(AIRS[s]["n_cols"] for s in segments)
    assert trace_lde.shape[1] == M and tuple(pub_lde.shape) == (n_groups, M, 4) and pub_lde.is_contiguous()
    _, _, stride = _table_shape(trace_lde)
    if out is None:
        out = torch.empty((M, 4), dtype=torch.int64, device=trace_lde.device)
    assert tuple(out.shape) == (M, 4) and out.is_contiguous() and (acc is None or (tuple(acc.shape) == (M, 4)
                                                                                    and acc.is_contiguous()))
    _lib.check(lib.sp_builtins_boundary_dev(sum(SEG_BITS[s] for s in segments), n.bit_length() - 1, trace_lde.data_ptr(),
                                            stride, pub_lde.data_ptr(), pack_felts(alphas), pack_felts([shift]),
                                            None if acc is None else acc.data_ptr(), out.data_ptr(), _stream()),
               "sp_builtins_boundary_dev")
    return out


def builtins_boundary_coefficients(segments, columns, n, alphas):
    """[3 k_pedersen + 3 k_ecdsa + k_rc16, 4]: the coefficients, in natural order, of every group's C_d back to back
    (combined on the device, one inverse ntt call per group; at k = 1 they are the values)."""
    torch = _torch()
    segments = _ordered_segments(segments)
    parts = []
    for comb in _builtin_combined(segments, columns, alphas):
        parts += [col if col.shape[0] == 1 else ntt(col, inverse=True) for col in comb]
    return torch.cat(parts).contiguous()


def builtins_boundary_points(segments, n, coef, alphas, shift, pos, cur):
    """B at arbitrary LDE positions from opened rows (sp_builtins_boundary_points_dev): coef from
    builtins_boundary_coefficients with the same alphas, pos [q] int64 tensor of LDE indices, cur [q, n_cols, 4] the
    WHOLE phase-1 rows there.  Returns (out [q, 4], status [q] uint8)."""
    torch = _torch()
    lib = _lib.ensure_init()
    segments = _ordered_segments(segments)
    q = pos.shape[0]
    n_cols = sum(AIRS[s]["n_cols"] for s in segments)
    n_coef = sum(len(BOUNDARY_DESCRIPTORS[BUILTIN_BOUNDARY[s]]["rows"]) * (n // AIRS[s]["period"]) for s in segments)
    assert len(alphas) == _builtin_boundary_shape(segments)[0] and tuple(coef.shape) == (n_coef, 4) and coef.is_contiguous()
    assert pos.dtype == torch.int64 and pos.is_contiguous() and cur.is_contiguous() and tuple(cur.shape) == (q, n_cols, 4)
    out = torch.empty((q, 4), dtype=torch.int64, device=cur.device)
    status = torch.empty((q,), dtype=torch.uint8, device=cur.device)
    _lib.check(lib.sp_builtins_boundary_points_dev(sum(SEG_BITS[s] for s in segments), n.bit_length() - 1,
                                                   coef.data_ptr(), pack_felts(alphas), pack_felts([shift]), q,
                                                   pos.data_ptr(), cur.data_ptr(), out.data_ptr(), status.data_ptr(),
                                                   _stream()), "sp_builtins_boundary_points_dev")
    return out, status


def _builtin_usage_flat(pub, segments):
    """The flat transcript list of a builtins_io statement: the segment ids, then rc_min, rc_max, the count and the
    values, then the signatures, then the hash triples."""
    flat = [len(segments)] + [BUILTIN_SEGMENTS.index(s) for s in segments]
    if "rc16" in segments:
        flat += [pub["rc_min"], pub["rc_max"], len(pub["rc_values"])] + list(pub["rc_values"])
    if "ecdsa" in segments:
        flat += [v for sig in pub["signatures"] for v in sig]
    if "pedersen" in segments:
        flat += [v for triple in pub["hashes"] for v in triple]
    return flat


def _builtin_usage_columns(pub, n, segments, dev, padded=None):
    """segment -> the public value column of each of its terms, as device tensors, from a statement's public inputs:
    x, y, h | z, r, Qx, Qy, w = s^-1 mod N (ONE modular inversion) | the padded rc16 values (rc16_fill_tensor)."""
    cols = {}
    if "pedersen" in segments:
        cols["pedersen"] = [felts_to_tensor([t[c] for t in pub["hashes"]], dev) for c in range(3)]
    if "ecdsa" in segments:
        sigs = pub["signatures"]
        cols["ecdsa"] = [felts_to_tensor(v, dev) for v in ([s[0] for s in sigs], [s[1] for s in sigs], [s[3] for s in sigs],
                                                           [s[4] for s in sigs],
                                                           _inverses_mod([s[2] for s in sigs], EC_ORDER))]
    if "rc16" in segments:
        cols["rc16"] = [padded if padded is not None else rc16_fill_tensor(pub["rc_values"], n // RC16_LIMBS, dev)[0]]
    return cols


def prove_builtin_usage(hash_inputs=None, signatures=None, rc_values=None, n_queries: int = 8, seed: int = 0,
                        final_log: int = 6, shift: int = FIELD_GEN, log_rows: int = None, claims=None):
    """prove_builtins as a proof of a STATEMENT: arguments, trace, phases, FRI and query phase are prove_builtins's, and
    the public inputs (a dict, AIR name "builtins_io", the keys of the present segments only) are bound:
      hashes      one [x, y, h] per Pedersen instance of the trace (n / 512, the caller's list cycled): h = H(x, y);
      signatures  one [z, r, s, Qx, Qy] per ECDSA instance (n / 1024, cycled): a signature the reference accepts;
      rc_values   the caller's values with rc_min, rc_max: each below 2^128.  The rc16 segment holds
                  rc16_fill(rc_values, n / 8) - the values, the hole-filling pads, the filler - a function of
                  rc_values and n that the verifier recomputes.
    On top of the 11 + 26 + 8 constraints the present segments bring the 3 + 5 + 1 boundary terms of pedersen_io,
    ecdsa_io and rc16_io (acc at row 8 i + 7 is the i-th padded value) with challenges of their own, drawn after the
    AIRs'.  The public value columns come from tensors the prover holds (h is px at rows 512 i + 511 of the trace),
    are combined on the device (sp_boundary_combine_dev), extended with one sp_lde_dev call per group and enter the
    composition through ONE sp_builtins_boundary_dev call.  `claims`, when given, is a dict that replaces any of
    "hashes", "signatures", "rc_values" of the public inputs - in the transcript, the composition and FRI alike; it
    exists so that a test can make the prover lie consistently: such a proof is rejected ("final layer degree").
    Verifier: verify_builtin_usage (verify and verify_builtins answer "malformed").

    What still is not: no zero knowledge, and Q queries at blowup 4 give about 2 Q bits of soundness."""
    claims = dict(claims or {})
    assert set(claims) <= {"hashes", "signatures", "rc_values"}

    def statement(held):
        n, segments, dev = held["n"], held["segments"], held["trace"].device
        assert set(claims) <= {{"pedersen": "hashes", "ecdsa": "signatures", "rc16": "rc_values"}[s] for s in segments}
        public, given, padded = {}, {}, None  # `given`: the columns the prover holds already
        if "rc16" in segments:
            if "rc_values" in claims:
                public["rc_values"] = [int(v) for v in claims["rc_values"]]
                _, _, public["rc_min"], public["rc_max"] = _rc16_fill_parts(public["rc_values"], n // RC16_LIMBS)
            else:
                public.update(held["public"], rc_values=[int(v) for v in rc_values])
                public.pop("signatures", None)
                padded = held["rc_padded"]
        if "ecdsa" in segments:
            public["signatures"] = [[int(v) for v in sig] for sig in claims.get("signatures", held["public"]["signatures"])]
            assert len(public["signatures"]) == n // 1024
            if "signatures" not in claims:
                z_t, r_t, w_t, qx_t, qy_t = held["sig_zrwq"]
                given["ecdsa"] = [z_t, r_t, qx_t, qy_t, w_t]
        if "pedersen" in segments:
            if "hashes" in claims:
                public["hashes"] = [[int(v) for v in t] for t in claims["hashes"]]
                assert len(public["hashes"]) == n // 512
            else:
                h_t = held["trace"][1, 511::512].contiguous()
                public["hashes"] = [[x, y, h] for (x, y), h in zip(held["hashes"], tensor_to_felts(h_t))]
                given["pedersen"] = list(held["hash_xy"]) + [h_t]
        columns = dict(_builtin_usage_columns(public, n, [s for s in segments if s not in given], dev, padded), **given)

        def add_boundary(trace_lde, comp, alphas):
            pub_lde = builtins_boundary_public_lde(segments, columns, n, alphas, shift)
            return builtins_boundary(segments, trace_lde, pub_lde, n, alphas, shift, acc=comp, out=comp)
        return (BUILTINS_IO_AIR, public, _builtin_usage_flat(public, segments), _builtin_boundary_shape(segments)[0],
                add_boundary)
    return _query_builtins(_commit_builtins(hash_inputs, signatures, rc_values, seed, final_log, shift, log_rows,
                                            statement), n_queries)


def verify_builtin_usage(proof, final_log: int = 6, n_queries: int = None) -> Tuple[bool, str]:
    """Verifier of prove_builtin_usage: (True, "ok") says that every [x, y, h] of public_inputs["hashes"] is a
    Pedersen hash, every [z, r, s, Qx, Qy] of ["signatures"] a signature the reference accepts and every value of
    ["rc_values"] below 2^128 - the instances of the trace ARE the published ones - up to the soundness of the
    argument: about 2 Q bits for Q queries at blowup 4, and no zero knowledge.  Reasons, their order and the
    "malformed" rules are verify_builtins's; "public inputs", at that reason's turn, also for a list of the wrong
    length (n / 512 triples, n / 1024 signatures), a hash value that is no felt, a range-checked value of 2^128 or more,
    values whose fill does not fit the n / 8 cells, and rc_min / rc_max other than the fill's.  A proof of another AIR
    is "malformed" here, as this AIR is for verify and verify_builtins.

    Where it runs: as verify_builtins, with 3 + 5 + 1 more alphas.  The public inputs are packed on the host - the
    padded range-check list by rc16_fill_tensor, w_i = s_i^-1 mod N behind one modular inversion - combined on the
    device (sp_boundary_combine_dev) and turned into coefficients by one inverse ntt per group, once per proof; ONE
    sp_builtins_boundary_points_dev launch gives B at the 2 Q opened points, added with sp_felt_add_dev."""
    kept = {}

    def public_ok(pub, n, segments):
        if "pedersen" in segments and not (len(pub["hashes"]) == n // 512 and all(_is_felt(v) for t in pub["hashes"]
                                                                                   for v in t)):
            return False
        if "rc16" in segments:
            values = pub["rc_values"]
            if not values or not all(v < 1 << RANGE_CHECK_BITS for v in values):
                return False
            try:
                kept["padded"], lo, hi = rc16_fill_tensor(values, n // RC16_LIMBS, "cpu")
            except ValueError:  # the fill does not fit
                return False
            if (lo, hi) != (pub["rc_min"], pub["rc_max"]):
                return False
        return True

    def boundary_at(pub, n, segments, alphas, shift, positions, cur, dev):
        padded = kept["padded"].to(dev) if "rc16" in segments else None
        coef = builtins_boundary_coefficients(segments, _builtin_usage_columns(pub, n, segments, dev, padded), n, alphas)
        return builtins_boundary_points(segments, n, coef, alphas, shift, positions, cur)
    return _verify_builtins_proof(proof, final_log, n_queries,
                                  (BUILTINS_IO_AIR, public_ok, _builtin_usage_flat,
                                   lambda segments: _builtin_boundary_shape(segments)[0], boundary_at))
