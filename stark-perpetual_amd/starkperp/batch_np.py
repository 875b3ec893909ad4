"""NumPy batch entry points: the same C-ABI calls as starkperp.batch with felts as `uint64[n, 4]`
little-endian limb arrays (the ABI's own layout), so that a 4096-order batch does not pay a Python
int <-> bytes conversion per field element (round 1: ~5 ms of the 17 ms host-inclusive C3 batch).
Range errors are reported the way the list API reports them (AssertionError for what signature.py
asserts); the arrays are handed to the library without a copy when they are C-contiguous uint64."""
import ctypes

import numpy as np

from . import _lib
from .batch import (EC_INFINITY, EC_NOT_ON_CURVE, EC_OK, EC_ORDER, EC_OUT_OF_RANGE, FIELD_PRIME, HASH_OUT_OF_RANGE, HASH_UNHASHABLE, SIGN_BAD_INPUT, SIGN_OK, SIGN_RETRY,
                    SQRT_NON_RESIDUE, SQRT_OK, SQRT_OUT_OF_RANGE,
                    VERIFY_TRUE, WITNESS_HASH_MISMATCH, WITNESS_LINK_MISMATCH, WITNESS_ROOT_MISMATCH,
                    WITNESS_SIBLING_CHANGED, _raise_hash_status, raise_for_verify_code)

_P_LIMBS = np.array([(FIELD_PRIME >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def felts_from_ints(values) -> np.ndarray:
    """ints (0 <= v < 2^256) -> uint64[n, 4]."""
    raw = b"".join([int(v).to_bytes(32, "little") for v in values])
    return np.frombuffer(raw, dtype="<u8").reshape(len(values), 4).copy()


def ints_from_felts(arr) -> list:
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(len(raw) // 32)]


def _felts(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == 4 and (n is None or a.shape[0] == n), "felts are uint64[n, 4]"
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pack_fields(n, fields) -> np.ndarray:
    """Bit-packs 64-bit fields into felts: fields = [(uint64[n] values or an int, bit offset)], offsets
    non-overlapping - the word layouts of perpetual_messages.py without big-integer arithmetic."""
    out = np.zeros((n, 4), dtype=np.uint64)
    for values, offset in fields:
        v = np.broadcast_to(np.asarray(values, dtype=np.uint64), (n,))
        k, sh = divmod(offset, 64)
        out[:, k] |= v << np.uint64(sh)
        if sh and k + 1 < 4:
            out[:, k + 1] |= v >> np.uint64(64 - sh)
    return out


def pedersen_hash_many(x, y) -> np.ndarray:
    """uint64[n, 4] x, y -> uint64[n, 4] hashes (signature.py:296-318 per row)."""
    x = _felts(x)
    n = x.shape[0]
    y = _felts(y, n)
    out = np.empty((n, 4), dtype=np.uint64)
    if n == 0:
        return out
    st = np.zeros(n, dtype=np.uint8)
    _lib.check(_lib.ensure_init().sp_pedersen_batch(_ptr(x), _ptr(y), _ptr(out), _ptr(st), n), "sp_pedersen_batch")
    bad = np.flatnonzero(st)
    if bad.size:
        _raise_hash_status(int(st[bad[0]]))
    return out


def pedersen_chains(words) -> np.ndarray:
    """words uint64[depth, n, 4]: row i of the result = H(...H(H(w[0][i], w[1][i]), w[2][i])..., w[-1][i])."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert w.ndim == 3 and w.shape[2] == 4 and w.shape[0] >= 1
    depth, n = w.shape[0], w.shape[1]
    out = np.empty((n, 4), dtype=np.uint64)
    if n == 0:
        return out
    st = np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.ensure_init().sp_pedersen_chains(_ptr(w), n, depth, _ptr(out), _ptr(st)), "sp_pedersen_chains")
    if st[0]:
        _raise_hash_status(HASH_UNHASHABLE if st[0] & 2 else HASH_OUT_OF_RANGE)
    return out


def pedersen_chains_ragged(words, offsets):
    """Chains of unequal length in one call (sp_pedersen_chains_ragged): words uint64[total, 4] chain after chain,
    offsets uint32[n + 1] (offsets[0] = 0, rising by at least 1, offsets[n] = total); chain i folds the rows
    offsets[i] .. offsets[i + 1) from the left, a chain of one row being that row.
    Returns (hashes uint64[n, 4], status uint8[n]).  Unlike its neighbours this call does NOT raise for a word
    outside [0, p) or an unhashable step: status[i] carries HASH_OUT_OF_RANGE / HASH_UNHASHABLE bits for chain i
    alone and the other rows are good - a mixed transaction batch wants to know WHICH item was bad."""
    w = _felts(words)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    assert off.ndim == 1 and off.shape[0] >= 1, "offsets are uint32[n + 1]"
    n = off.shape[0] - 1
    assert int(off[-1]) == w.shape[0], "offsets[n] must be the number of rows"
    out = np.empty((n, 4), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return out, st
    _lib.check(_lib.ensure_init().sp_pedersen_chains_ragged(_ptr(w), _ptr(off), n, _ptr(out), _ptr(st)),
               "sp_pedersen_chains_ragged")
    return out, st


def merkle_path_args(leaves, siblings, keys, height=None, offsets=None):
    """The arguments of the Merkle path calls, checked: (leaves uint64[n, 4], siblings uint64[total, 4], offsets
    uint32[n + 1] or None, height, keys uint64[n]).  Exactly one of `height` (every path has `height` siblings:
    siblings uint64[n, height, 4] or [n * height, 4], the output of tree_prove) and `offsets` (uint32[n + 1],
    offsets[0] = 0, non-decreasing by at most 64, offsets[n] = rows of siblings) is given.  Pure host code."""
    lv = _felts(leaves)
    n = lv.shape[0]
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    assert k.ndim == 1 and k.shape[0] == n, "keys are uint64[n]"
    assert (height is None) != (offsets is None), "give either height or offsets"
    sib = np.ascontiguousarray(siblings, dtype=np.uint64)
    if height is not None:
        height = int(height)
        assert 0 <= height <= 64, "height is 0 .. 64"
        sib = sib.reshape(n * height, 4)
        return lv, sib, None, height, k
    assert sib.ndim == 2 and sib.shape[1] == 4, "felts are uint64[n, 4]"
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    assert off.ndim == 1 and off.shape[0] == n + 1, "offsets are uint32[n + 1]"
    assert int(off[-1]) == sib.shape[0], "offsets[n] must be the number of sibling rows"
    return lv, sib, off, 0, k


def uniform_path_offsets(n, height) -> np.ndarray:
    """The offsets that describe n paths of `height` siblings each: what the library builds when offsets is None."""
    return (np.arange(n + 1, dtype=np.uint64) * np.uint64(height)).astype(np.uint32)


def merkle_fold_paths(leaves, siblings, keys, height=None, offsets=None):
    """Merkle paths folded on the device in one call (sp_merkle_fold_paths): path i starts from leaves[i]; at level l
    bit l of keys[i] says whether the running node is the right child (merkle_tree.py:4-26), node = H(left, right).
    Arguments as merkle_path_args.  Returns (roots uint64[n, 4], status uint8[n]); like pedersen_chains_ragged it
    does not raise for a value outside [0, p): status[i] carries the HASH_* bits of path i alone."""
    lv, sib, off, height, k = merkle_path_args(leaves, siblings, keys, height, offsets)
    n = lv.shape[0]
    roots = np.empty((n, 4), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return roots, st
    _lib.check(_lib.ensure_init().sp_merkle_fold_paths(_ptr(lv), _ptr(sib), None if off is None else _ptr(off), height,
                                                       _ptr(k), n, _ptr(roots), _ptr(st)), "sp_merkle_fold_paths")
    return roots, st


def merkle_verify_paths(leaves, siblings, keys, expected, height=None, offsets=None):
    """Inclusion proofs checked on the device in one call (sp_merkle_verify_paths): expected = uint64[4] / [1, 4]
    (one root for all paths) or uint64[n, 4].  Returns (verdict bool[n], status uint8[n]); verdict[i] is True only
    if status[i] is 0 and path i folds to its expected root.  Only these bytes come back from the device."""
    lv, sib, off, height, k = merkle_path_args(leaves, siblings, keys, height, offsets)
    n = lv.shape[0]
    exp = np.ascontiguousarray(expected, dtype=np.uint64).reshape(-1, 4)
    assert exp.shape[0] in (1, n), "expected holds 1 or n roots"
    verdict = np.zeros(n, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return verdict.astype(bool), st
    _lib.check(_lib.ensure_init().sp_merkle_verify_paths(_ptr(lv), _ptr(sib), None if off is None else _ptr(off), height,
                                                         _ptr(k), n, _ptr(exp), exp.shape[0], _ptr(verdict), _ptr(st)),
               "sp_merkle_verify_paths")
    return verdict == 1, st


def verify_codes(z, r, s, qx, qy=None, key_tables=None) -> np.ndarray:
    """Result codes (include/starkperp.h SP_VERIFY_*) of verify(z, r, s, key) per row; qy None = x-only
    keys (signature.py:229-238).  key_tables as in starkperp.batch.verify_codes."""
    z = _felts(z)
    n = z.shape[0]
    r, s, qx = _felts(r, n), _felts(s, n), _felts(qx, n)
    qy = None if qy is None else _felts(qy, n)
    res = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return res
    lib = _lib.ensure_init()
    fn = lib.sp_ecdsa_verify_batch if key_tables is None else (
        lib.sp_ecdsa_verify_batch_keyed if key_tables else None)
    if fn is None:
        raise ValueError("key_tables=False (forced ladder) is only offered by the list API")
    _lib.check(fn(_ptr(z), _ptr(r), _ptr(s), _ptr(qx), None if qy is None else _ptr(qy), _ptr(res), n),
               "sp_ecdsa_verify_batch")
    return res


def verify_many(z, r, s, qx, qy=None) -> np.ndarray:
    """bool[n]; raises the reference's AssertionError for the first row that violates a pre-assert."""
    codes = verify_codes(z, r, s, qx, qy)
    bad = np.flatnonzero(codes > VERIFY_TRUE)
    if bad.size:
        i = int(bad[0])
        zi, ri, si = (ints_from_felts(a[i : i + 1])[0] for a in (_felts(z), _felts(r), _felts(s)))
        raise_for_verify_code(int(codes[i]), zi, ri, si)
    return codes == VERIFY_TRUE


def _root_call(fn, a, want_root):
    a = _felts(a)
    n = a.shape[0]
    out = np.zeros((n, 4), dtype=np.uint64) if want_root else None
    st = np.zeros(n, dtype=np.uint8)
    if n:
        _lib.check(getattr(_lib.ensure_init(), fn)(_ptr(a), None if out is None else _ptr(out), _ptr(st), n), fn)
    return out, st


def felt_sqrt(a):
    """uint64[n, 4] felts -> (roots uint64[n, 4], status uint8[n]): sqrt_mod(a, FIELD_PRIME) per row (math_utils.py:43-47,
    the smaller root; sp_felt_sqrt_batch).  status SQRT_OK / SQRT_NON_RESIDUE / SQRT_OUT_OF_RANGE (a felt that is not
    below p is passed through and reported, not reduced); the root of a row that is not SQRT_OK stays zero."""
    return _root_call("sp_felt_sqrt_batch", a, True)


def stark_key_y(qx, want_y=True):
    """x-only keys uint64[n, 4] -> (qy uint64[n, 4] or None, status uint8[n]): get_y_coordinate per row
    (signature.py:84-96; sp_stark_key_y_batch), SQRT_NON_RESIDUE where the reference raises InvalidPublicKeyError.
    want_y=False: is_valid_stark_key alone (signature.py:204-214) - no root is extracted."""
    return _root_call("sp_stark_key_y_batch", qx, want_y)


def _ec_call(fn, inputs, extra=()):
    inputs = [_felts(inputs[0])] + [_felts(a, len(inputs[0])) for a in inputs[1:]]
    n = inputs[0].shape[0]
    rx, ry = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    if n:
        _lib.check(getattr(_lib.ensure_init(), fn)(*[_ptr(a) for a in inputs], *extra, _ptr(rx), _ptr(ry), _ptr(st), n), fn)
    return rx, ry, st


def ec_mult(k, px, py):
    """uint64[n, 4] scalars and affine points -> (rx, ry, status): k P per row on the Stark curve (sp_ec_mult_batch;
    math_utils.py:91-100).  status EC_OK / EC_INFINITY / EC_OUT_OF_RANGE / EC_NOT_ON_CURVE of starkperp.batch; nothing is
    reduced, and the rows that are not EC_OK stay zero."""
    return _ec_call("sp_ec_mult_batch", [k, px, py])


def ec_lincomb(a, b, px, py):
    """(rx, ry, status) of a EC_GEN + b P per row (sp_ec_lincomb_batch); rows that are not EC_OK stay zero."""
    return _ec_call("sp_ec_lincomb_batch", [a, b, px, py])


def ec_add(px, py, qx, qy, subtract=False):
    """(rx, ry, status) of P + Q per row, P - Q with subtract (sp_ec_add_batch): every pair, equal and opposite points
    included; rows that are not EC_OK stay zero."""
    return _ec_call("sp_ec_add_batch", [px, py, qx, qy], (1 if subtract else 0,))


def sign_many(z, d, seeds=None):
    """sign(z, d, seed) per row (signature.py:137-173: RFC 6979 nonce, attempt and retry rule on the device,
    sp_ecdsa_sign_rfc6979_batch) without a Python int per field element: z, d uint64[n, 4], seeds uint64[n] or
    None (0 = no seed) -> (r, s) uint64[n, 4].  Raises the reference's AssertionError for a message >= 2^251
    and for a key outside [1, EC_ORDER) (starkperp.batch.sign_many); an item the device hands back after eight
    rejected nonces (a 2^-55 event each) is finished by the list API's host nonce generator."""
    z = _felts(z)
    n = z.shape[0]
    d = _felts(d, n)
    r, s = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    if n == 0:
        return r, s
    st = np.zeros(n, dtype=np.uint8)
    sd = None
    if seeds is not None:
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert sd.shape == (n,), "seeds are uint64[n]"
    lib = _lib.ensure_init()
    _lib.check(lib.sp_ecdsa_sign_rfc6979_batch(_ptr(z), _ptr(d), None if sd is None else _ptr(sd), _ptr(r), _ptr(s),
                                               _ptr(st), n), "sp_ecdsa_sign_rfc6979_batch")
    bad = np.flatnonzero(st == SIGN_BAD_INPUT)
    if bad.size:
        i = int(bad[0])
        zi, di = ints_from_felts(z[i : i + 1])[0], ints_from_felts(d[i : i + 1])[0]
        assert 0 <= zi < 2**251, "Message not signable."
        raise AssertionError("private key must be in [1, EC_ORDER), got %s" % hex(di))
    left = np.flatnonzero(st == SIGN_RETRY)
    if left.size:
        from .batch import _sign_many_host_nonces
        zs, ds = ints_from_felts(z[left]), ints_from_felts(d[left])
        sl = [None if sd is None or int(sd[i]) == 0 else int(sd[i]) for i in left]
        sigs = _sign_many_host_nonces(zs, ds, sl)
        r[left] = felts_from_ints([a for a, _ in sigs])
        s[left] = felts_from_ints([b for _, b in sigs])
    return r, s


def order_ids(message_hashes) -> np.ndarray:
    """order/order.cairo:23-59: the 64 most significant bits of the 251-bit message hash, uint64[n]."""
    h = _felts(message_hashes)
    # 0 <= message_hash < SIGNED_MESSAGE_BOUND (order.cairo:22): a larger hash has no 64-bit order id
    assert not np.any(h[:, 3] >> np.uint64(59)), "message hash >= 2**251"
    return (h[:, 2] >> np.uint64(59)) | (h[:, 3] << np.uint64(5))


def limit_order_words(asset_sell, asset_buy, asset_fee, amount_sell, amount_buy, amount_fee, nonce, position_id,
                      expiration_timestamp) -> np.ndarray:
    """The five hash inputs of get_limit_order_msg_without_bounds (perpetual_messages.py:253-286) for n
    orders: uint64[5, n, 4].  Assets are felts (uint64[n, 4]); amounts / position ids uint64[n]; nonce and
    expiration below 2^32.  sell / buy are the caller's choice (is_buying_synthetic picks them)."""
    a_s, a_b, a_f = _felts(asset_sell), _felts(asset_buy), _felts(asset_fee)
    n = a_s.shape[0]
    u = lambda v: np.broadcast_to(np.asarray(v, dtype=np.uint64), (n,))
    assert int(u(nonce).max(initial=0)) < 2**32 and int(u(expiration_timestamp).max(initial=0)) < 2**32
    word0 = pack_fields(n, [(u(nonce), 0), (u(amount_fee), 32), (u(amount_buy), 96), (u(amount_sell), 160)])
    pos = u(position_id)
    word1 = pack_fields(n, [(u(expiration_timestamp), 17), (pos, 49), (pos, 113), (pos, 177), (3, 241)])
    return np.stack([a_s, a_b, a_f, word0, word1])


def limit_order_msgs(*args) -> np.ndarray:
    """Message hashes of n limit orders: four batched launches, arrays in and out."""
    return pedersen_chains(limit_order_words(*args))


TREE_NOT_COMMITTED = 0x80  # include/starkperp.h SP_TREE_NOT_COMMITTED


def order_batch(words, r, s, qx, tree, leaves, qy=None, id_shift=187):
    """BASELINE.json configs[2] in ONE library call (sp_order_batch): message-hash chains of the n orders
    (words uint64[depth, n, 4], e.g. limit_order_words; depth 1 = the message hashes themselves) -> verification of
    (z, r, s, key) through the key tables (z >= 2^251 is no signed message: verdict VERIFY_ASSERT_MSG = 5 and nothing
    is committed, constants.cairo:57) -> order ids (the top 64 bits of the 251-bit hash) -> update of `tree` (a state.LibrarySparseTree)
    with leaves[i] at order id i.  The verification overlaps the tree's level hashing on the device; the tree
    is committed only when every signature verified.
    Returns (z uint64[n, 4], verdict codes uint8[n], old_root, new_root, committed)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert w.ndim == 3 and w.shape[2] == 4 and w.shape[0] >= 1
    depth, n = w.shape[0], w.shape[1]
    r, s, qx, leaves = _felts(r, n), _felts(s, n), _felts(qx, n), _felts(leaves, n)
    qy = None if qy is None else _felts(qy, n)
    z = np.empty((n, 4), dtype=np.uint64)
    verdicts = np.zeros(n, dtype=np.uint8)
    old, new, st = _lib.new_felts(1), _lib.new_felts(1), np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.ensure_init().sp_order_batch(_ptr(w), depth, n, _ptr(r), _ptr(s), _ptr(qx),
                                                 None if qy is None else _ptr(qy), tree._handle, _ptr(leaves), id_shift,
                                                 _ptr(z), _ptr(verdicts), old, new, _ptr(st)), "sp_order_batch")
    if st[0] & (HASH_OUT_OF_RANGE | HASH_UNHASHABLE):
        _raise_hash_status(HASH_UNHASHABLE if st[0] & 2 else HASH_OUT_OF_RANGE)
    return z, verdicts, _lib.unpack_felts(old, 1)[0], _lib.unpack_felts(new, 1)[0], st[0] == 0


STATE_PREV_MISMATCH = 0x10  # include/starkperp.h SP_STATE_PREV_MISMATCH


def state_batch(positions_tree, orders_tree, pos_keys, prev_words, prev_off, new_words, new_off, ord_keys, ord_prev,
                ord_new):
    """The whole state update of a batch in ONE library call (sp_state_batch; state/state.cairo:135-186): previous and
    new leaf of every touched position, update of the positions tree and of the orders tree (state.LibrarySparseTree
    both), all or nothing across the two.
      pos_keys uint64[n_pos], ord_keys uint64[n_ord]   strictly increasing, squashed (state.squash_updates)
      prev_words uint64[*, 4], prev_off uint32[n_pos + 1]   the previous leaf of position i is the left-fold chain over
                 rows prev_off[i] .. prev_off[i + 1] (the convention of pedersen_chains_ragged)
      new_words, new_off   the new leaf likewise; new_off[i + 1] == new_off[i]: the position is unchanged
      ord_prev, ord_new uint64[n_ord, 4]   the orders-tree leaves before and after
    state.pack_state_batch builds these arrays from squashed updates.  Nothing is raised for data-dependent outcomes:
    returns ((pos_old_root, pos_new_root), (ord_old_root, ord_new_root), pos_status uint8[n_pos], ord_status
    uint8[n_ord], batch_status) - batch_status 0 = committed, otherwise TREE_NOT_COMMITTED | the status bits met
    (HASH_OUT_OF_RANGE, HASH_UNHASHABLE, STATE_PREV_MISMATCH) with both trees as they were."""
    pos_keys = np.ascontiguousarray(pos_keys, dtype=np.uint64)
    ord_keys = np.ascontiguousarray(ord_keys, dtype=np.uint64)
    prev_off = np.ascontiguousarray(prev_off, dtype=np.uint32)
    new_off = np.ascontiguousarray(new_off, dtype=np.uint32)
    assert pos_keys.ndim == 1 and ord_keys.ndim == 1 and prev_off.ndim == 1 and new_off.ndim == 1
    n_pos, n_ord = pos_keys.shape[0], ord_keys.shape[0]
    assert prev_off.shape[0] == n_pos + 1 and new_off.shape[0] == n_pos + 1, "offsets are uint32[n_pos + 1]"
    prev_words, new_words = _felts(prev_words), _felts(new_words)
    assert int(prev_off[-1]) <= prev_words.shape[0] and int(new_off[-1]) <= new_words.shape[0], \
        "offsets point behind the words"
    ord_prev, ord_new = _felts(ord_prev, n_ord), _felts(ord_new, n_ord)
    roots = np.zeros((4, 4), dtype=np.uint64)
    pos_st, ord_st = np.zeros(n_pos, dtype=np.uint8), np.zeros(n_ord, dtype=np.uint8)
    batch_st = np.zeros(1, dtype=np.uint8)
    _lib.check(_lib.ensure_init().sp_state_batch(
        positions_tree._handle, orders_tree._handle, _ptr(pos_keys), n_pos, _ptr(prev_words), _ptr(prev_off),
        _ptr(new_words), _ptr(new_off), _ptr(ord_keys), _ptr(ord_prev), _ptr(ord_new), n_ord, _ptr(roots[0:1]),
        _ptr(roots[1:2]), _ptr(roots[2:3]), _ptr(roots[3:4]), _ptr(pos_st), _ptr(ord_st), _ptr(batch_st)),
        "sp_state_batch")
    r = ints_from_felts(roots)
    return (r[0], r[1]), (r[2], r[3]), pos_st, ord_st, int(batch_st[0])


def tree_witness_size(height, keys) -> int:
    """Number of records sp_tree_witness returns for `keys` (uint64[n], strictly increasing) in a tree of `height`:
    host arithmetic inside the library, no GPU and no sp_init needed."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.ndim == 1
    count = ctypes.c_size_t()
    _lib.check(_lib.load().sp_tree_witness_size(height, _ptr(keys), keys.shape[0], ctypes.byref(count)),
               "sp_tree_witness_size")
    return count.value


def tree_witness(tree, keys):
    """The merkle_facts (main.cairo:39-40, 61-64) of the subtree induced by `keys` (uint64[n], strictly increasing) in
    `tree` (a state.LibrarySparseTree) as it stands: one record per inner node, level 1 (parents of leaves) up to the
    root, ascending index inside a level.  Returns (level uint8[R], index uint64[R], node, left, right uint64[R, 4])."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.ndim == 1
    n = keys.shape[0]
    cap = tree_witness_size(tree.height, keys)
    level, index = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint64)
    node, left, right = (np.zeros((cap, 4), dtype=np.uint64) for _ in range(3))
    count = ctypes.c_size_t()
    _lib.check(_lib.ensure_init().sp_tree_witness(tree._handle, _ptr(keys), n, cap, _ptr(level), _ptr(index), _ptr(node),
                                                  _ptr(left), _ptr(right), ctypes.byref(count)), "sp_tree_witness")
    assert count.value == cap
    return level, index, node, left, right


def tree_prove(tree, keys):
    """Inclusion proofs of `keys` (uint64[n], any order, repeats allowed) in `tree` (a state.LibrarySparseTree): returns
    (leaves uint64[n, 4], siblings uint64[n, height, 4]); siblings[i, l] sits at level l beside the path of keys[i]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.ndim == 1
    n, height = keys.shape[0], tree.height
    leaves = np.zeros((n, 4), dtype=np.uint64)
    siblings = np.zeros((n, height, 4), dtype=np.uint64)
    _lib.check(_lib.ensure_init().sp_tree_prove(tree._handle, _ptr(keys), n, _ptr(leaves), _ptr(siblings)),
               "sp_tree_prove")
    return leaves, siblings


TREE_SCAN_MAX = 1 << 22  # SP_TREE_SCAN_MAX: the largest page of one sp_tree_scan call


def tree_scan(handle, lo, hi, capacity):
    """One page of the ordered range scan (sp_tree_scan) of the tree behind `handle` (a state.LibrarySparseTree or its
    integer handle): the first `capacity` keys k, lo <= k <= hi inclusive, whose leaf is not the tree's empty leaf.
    Returns (keys uint64[n] ascending, leaves uint64[n, 4], more bool); more: further such keys exist in the range,
    resume with lo = keys[-1] + 1."""
    handle = getattr(handle, "_handle", handle)
    cap = min(int(capacity), TREE_SCAN_MAX)
    keys, leaves = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros((max(cap, 1), 4), dtype=np.uint64)
    count, more = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(_lib.ensure_init().sp_tree_scan(handle, lo, hi, capacity, _ptr(keys), _ptr(leaves), ctypes.byref(count),
                                               ctypes.byref(more)), "sp_tree_scan")
    return keys[:count.value], leaves[:count.value], bool(more.value)


def tree_clone(handle):
    """A second handle holding the same tree (sp_tree_clone): the node table is copied on the device, nothing is hashed.
    Returns the new integer handle; the caller destroys it (state.LibrarySparseTree.clone wraps it)."""
    handle = getattr(handle, "_handle", handle)
    out = ctypes.c_int()
    _lib.check(_lib.ensure_init().sp_tree_clone(handle, ctypes.byref(out)), "sp_tree_clone")
    return out.value


TREE_DIFF_MAX = TREE_SCAN_MAX  # SP_TREE_DIFF_MAX: the largest page of one sp_tree_diff call


def tree_diff(a, b, lo, hi, capacity):
    """One page of the ordered diff (sp_tree_diff) of the trees behind `a` and `b` (state.LibrarySparseTree or integer
    handles): the first `capacity` keys k, lo <= k <= hi inclusive, whose leaf in a differs from the leaf in b.
    Returns (keys uint64[n] ascending, leaves_a uint64[n, 4], leaves_b uint64[n, 4], more bool); a key one tree does
    not hold reads as the empty leaf there; more: further differing keys exist in the range, resume with
    lo = keys[-1] + 1."""
    a, b = getattr(a, "_handle", a), getattr(b, "_handle", b)
    cap = max(min(int(capacity), TREE_DIFF_MAX), 1)
    keys = np.zeros(cap, dtype=np.uint64)
    leaves_a, leaves_b = np.zeros((cap, 4), dtype=np.uint64), np.zeros((cap, 4), dtype=np.uint64)
    count, more = ctypes.c_size_t(), ctypes.c_int()
    _lib.check(_lib.ensure_init().sp_tree_diff(a, b, lo, hi, capacity, _ptr(keys), _ptr(leaves_a), _ptr(leaves_b),
                                               ctypes.byref(count), ctypes.byref(more)), "sp_tree_diff")
    return keys[:count.value], leaves_a[:count.value], leaves_b[:count.value], bool(more.value)


def tree_table_size(handle):
    """(entries, slots) of the tree's node table as it stands (sp_tree_table_size): slots in use - it never shrinks -
    and the slot count."""
    handle = getattr(handle, "_handle", handle)
    entries, slots = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.ensure_init().sp_tree_table_size(handle, ctypes.byref(entries), ctypes.byref(slots)),
               "sp_tree_table_size")
    return entries.value, slots.value


def merkle_verify_update(height, keys, prev_leaves, new_leaves, prev_root, new_root, before, after):
    """The statement of merkle_multi_update(prev_leaves, new_leaves, height, prev_root, new_root)
    (state/state.cairo:155-173) checked against two witnesses in ONE library call (sp_merkle_verify_update): every
    record hashed once in a bulk launch, the links between the records, the leaves, the roots and the untouched siblings
    compared on the device.
      keys uint64[n] strictly increasing; prev_leaves, new_leaves uint64[n, 4]; prev_root, new_root ints or uint64[4]
      before, after   the tuples tree_witness returned for `keys` before and after the update (level and index are
                      not read: the library derives every position from the keys)
    Returns (verdict bool, status uint8[2, R]): status[0] for the before records, status[1] for the after records, a
    byte being the OR of HASH_OUT_OF_RANGE, HASH_UNHASHABLE and the WITNESS_* bits of starkperp.batch; the verdict is
    True iff every byte is 0.  Nothing is raised for a data-dependent outcome."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.ndim == 1
    n = keys.shape[0]
    prev_leaves, new_leaves = _felts(prev_leaves, n), _felts(new_leaves, n)
    roots = [felts_from_ints([r]) if isinstance(r, int) else _felts(np.reshape(r, (1, 4)), 1) for r in (prev_root, new_root)]
    node, left, right = (np.ascontiguousarray(np.concatenate([_felts(before[i]), _felts(after[i])]))
                         for i in (2, 3, 4))
    records = _felts(before[2]).shape[0]
    assert _felts(after[2]).shape[0] == records and left.shape[0] == 2 * records and right.shape[0] == 2 * records, \
        "before and after hold the same number of records"
    verdict = np.zeros(1, dtype=np.uint8)
    status = np.zeros((2, records), dtype=np.uint8)
    _lib.check(_lib.ensure_init().sp_merkle_verify_update(
        height, _ptr(keys), n, _ptr(prev_leaves), _ptr(new_leaves), _ptr(roots[0]), _ptr(roots[1]), _ptr(node),
        _ptr(left), _ptr(right), records, _ptr(verdict), _ptr(status)), "sp_merkle_verify_update")
    return bool(verdict[0] == 1), status
