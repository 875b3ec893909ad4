"""ctypes wrapper of oracle/starkref.c (ORACLE - test infrastructure only).  Builds the shared
library on first use (gcc -O3 -fopenmp) into oracle/_build/ (git-ignored)."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libstarkref.so")
_SRC = os.path.join(_HERE, "starkref.c")
_lib = None


def build():
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    subprocess.check_call(["gcc", "-O3", "-fopenmp", "-shared", "-fPIC", _SRC, "-o", _SO])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
            build()
        _lib = ctypes.CDLL(_SO)
        _lib.cref_max_threads.restype = ctypes.c_int
    return _lib


def _pack(values):
    raw = b"".join(int(v).to_bytes(32, "little") for v in values)
    return (ctypes.c_uint64 * (4 * len(values))).from_buffer_copy(raw)


def _unpack(buf, n):
    raw = bytes(buf)
    return [int.from_bytes(raw[32 * i : 32 * i + 32], "little") for i in range(n)]


def max_threads():
    return int(lib().cref_max_threads())


def pedersen_hash_many(xs, ys):
    """Returns (outputs, status bytes): the 252-step affine loop of signature.py:300-318 in C."""
    n = len(xs)
    out = (ctypes.c_uint64 * (4 * n))()
    st = (ctypes.c_uint8 * n)()
    lib().cref_pedersen_batch(_pack(xs), _pack(ys), out, st, ctypes.c_size_t(n))
    return _unpack(out, n), list(bytes(st))


def pedersen_chain_right(elements):
    """H(e0, H(e1, ... H(e_{n-2}, e_{n-1}))) in one C call (12 000 links in about a second)."""
    n = len(elements)
    out = (ctypes.c_uint64 * 4)()
    status = lib().cref_pedersen_chain_right(_pack(elements), ctypes.c_size_t(n), out)
    assert status == 0, "unhashable link"
    return _unpack(out, 1)[0]


def opt_pedersen_hash_many(xs, ys):
    """The optimised comparator (windowed tables + batched affine additions): same outputs."""
    n = len(xs)
    out = (ctypes.c_uint64 * (4 * n))()
    st = (ctypes.c_uint8 * n)()
    lib().cref_opt_pedersen_batch(_pack(xs), _pack(ys), out, st, ctypes.c_size_t(n))
    return _unpack(out, n), list(bytes(st))


def opt_merkle_levels(leaves):
    n = len(leaves)
    height = n.bit_length() - 1
    assert n == 1 << height
    buf = (ctypes.c_uint64 * (4 * (2 * n - 1)))()
    ctypes.memmove(buf, _pack(leaves), 32 * n)
    lib().cref_opt_merkle_build(buf, ctypes.c_uint(height))
    flat = _unpack(buf, 2 * n - 1)
    levels, off, width = [], 0, n
    while width >= 1:
        levels.append(flat[off : off + width])
        off += width
        width //= 2
    return levels


def opt_merkle_timed(leaves, min_seconds=2.0, max_reps=256):
    """Repeats the optimised rebuild on one marshalled buffer (the leaves stay in place, the upper levels
    are overwritten): returns (levels, repetitions, seconds inside the C library)."""
    import time
    n = len(leaves)
    height = n.bit_length() - 1
    assert n == 1 << height
    buf = (ctypes.c_uint64 * (4 * (2 * n - 1)))()
    ctypes.memmove(buf, _pack(leaves), 32 * n)
    lib().cref_opt_merkle_build(buf, ctypes.c_uint(height))  # builds the window table on first use
    reps, t0, dt = 0, time.time(), 0.0
    while dt < min_seconds and reps < max_reps:
        lib().cref_opt_merkle_build(buf, ctypes.c_uint(height))
        reps += 1
        dt = time.time() - t0
    flat = _unpack(buf, 2 * n - 1)
    levels, off, width = [], 0, n
    while width >= 1:
        levels.append(flat[off : off + width])
        off += width
        width //= 2
    return levels, reps, dt


def merkle_levels(leaves):
    n = len(leaves)
    height = n.bit_length() - 1
    buf = (ctypes.c_uint64 * (4 * (2 * n - 1)))()
    ctypes.memmove(buf, _pack(leaves), 32 * n)
    lib().cref_merkle_build(buf, ctypes.c_uint(height))
    flat = _unpack(buf, 2 * n - 1)
    out, pos, width = [], 0, n
    while width >= 1:
        out.append(flat[pos : pos + width])
        pos += width
        width //= 2
    return out


def public_keys_many(ds):
    n = len(ds)
    qx, qy = (ctypes.c_uint64 * (4 * n))(), (ctypes.c_uint64 * (4 * n))()
    lib().cref_public_key_batch(_pack(ds), qx, qy, ctypes.c_size_t(n))
    return list(zip(_unpack(qx, n), _unpack(qy, n)))


def verify_codes(zs, rs, ss, points):
    """Point keys only; codes: 0 False, 1 True, 2..6 = which pre-assert (include/starkperp.h)."""
    n = len(zs)
    res = (ctypes.c_uint8 * n)()
    lib().cref_verify_batch(_pack(zs), _pack(rs), _pack(ss), _pack([p[0] for p in points]),
                            _pack([p[1] for p in points]), res, ctypes.c_size_t(n))
    return list(bytes(res))


# ---- dense transforms over GF(p): NumPy uint64[n, 4] in and out (four little-endian words per felt) ----------
def _felt_array(a):
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == 4, a.shape
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _log2(n):
    log_n = int(n).bit_length() - 1
    assert n == 1 << log_n, "size %d is not a power of two" % n
    return log_n


def _felt_words(v):
    return (ctypes.c_uint64 * 4).from_buffer_copy(int(v).to_bytes(32, "little"))


def _ok(rc, what):
    if rc != 0:
        raise MemoryError("%s: out of memory in the C oracle" % what)


def ntt_dense(col, inverse=False):
    """stark_ref.ntt(col, root_of_unity(log_n)) / stark_ref.intt of one column, natural order on both sides."""
    out = _felt_array(col).copy()
    _ok(lib().cref_ntt(_ptr(out), ctypes.c_uint(_log2(out.shape[0])), ctypes.c_int(1 if inverse else 0)), "cref_ntt")
    return out


def lde_dense(cols, log_blowup, shift):
    """stark_ref.lde(column, 1 << log_blowup, shift) of every column: uint64[ncols, n, 4] -> [ncols, n << log_blowup, 4]."""
    import numpy as np
    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    assert cols.ndim == 3 and cols.shape[2] == 4, cols.shape
    ncols, n = cols.shape[0], cols.shape[1]
    out = np.empty((ncols, n << log_blowup, 4), dtype=np.uint64)
    sh = _felt_words(shift)
    for c in range(ncols):
        _ok(lib().cref_lde(_ptr(cols[c]), _ptr(out[c]), ctypes.c_uint(_log2(n)), ctypes.c_uint(log_blowup), sh), "cref_lde")
    return out


def interpolate_dense(col):
    """What sp_interpolate_dev leaves: n times the coefficients of the interpolant over <w_n>, bit-reversed order."""
    col = _felt_array(col)
    out = col.copy()
    _ok(lib().cref_interpolate(_ptr(col), _ptr(out), ctypes.c_uint(_log2(col.shape[0]))), "cref_interpolate")
    return out


def coset_eval_dense(coef, shift):
    """The output of interpolate_dense -> the interpolant's values on shift * <w_n>, natural order (sp_coset_eval_dev)."""
    coef = _felt_array(coef)
    out = coef.copy()
    _ok(lib().cref_coset_eval(_ptr(coef), _ptr(out), ctypes.c_uint(_log2(coef.shape[0])), _felt_words(shift)),
        "cref_coset_eval")
    return out


def horner_dense(coef, points):
    """sum_k coef[k] x^k at every x of `points` (Python ints), by Horner's rule; returns uint64[len(points), 4]."""
    import numpy as np
    coef = _felt_array(coef)
    k = len(points)
    pts = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in points), dtype="<u8").reshape(k, 4)
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    out = np.empty((k, 4), dtype=np.uint64)
    lib().cref_horner(_ptr(coef), ctypes.c_size_t(coef.shape[0]), _ptr(pts), ctypes.c_size_t(k), _ptr(out))
    return out
