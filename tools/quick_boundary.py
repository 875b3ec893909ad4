#!/usr/bin/env python3
"""What binding the statement of an ECDSA proof costs: stark.prove_signatures beside stark.prove_ecdsa and
stark.verify_signatures beside stark.verify on 4096 signatures (a 2^22-row, 10-column trace; M = 2^24, 18 committed
FRI layers) at 8 and at 64 queries, same inputs, same process.  Provers: median of 5 calls after one warm-up each.
Verifiers: median of 24 calls after one warm-up.  Device part of the two new calls (sp_boundary_dev: table build + the
elementwise launch, one bracket; sp_boundary_points_dev: one launch) from sp_profile_begin / sp_profile_end around each
call, in passes of their own so that the bracket's waits stay out of the wall figures.  The dense call's bytes are those
of the arrays it streams once - the three distinct trace columns of the five terms, three public columns, acc, out:
eight felts a point; the 384 KiB table stays in L2 - beside the seven felts of sp_hash_io_boundary_dev in
profiles/hash_io.txt.  No threshold is fixed in advance: the file records what was measured, against the unbound proof
of the same run.

    python tools/quick_boundary.py [output file]      # default profiles/boundary.txt"""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stark-perpetual_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SIGNATURES, QUERIES, PROVE_RUNS, VERIFY_RUNS = 4096, (8, 64), 5, 24
DENSE_FELTS = 8  # m, qx, qy; C_0, C_1, C_2; acc; out


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "boundary.txt")
    import torch
    from starkperp import _lib, batch, stark
    lib = _lib.ensure_init()
    rng = random.Random(20)
    keys = [rng.randrange(1, stark.EC_ORDER) for _ in range(SIGNATURES)]
    zs = [rng.randrange(1, 2**251) for _ in range(SIGNATURES)]
    sigs = batch.sign_many(zs, keys)
    args = (zs, [r for r, _ in sigs], [s for _, s in sigs], [tuple(q) for q in batch.public_keys_many(keys)])
    device = {}

    def bracketed(fn, key):
        def call(*a, **kw):
            _lib.check(lib.sp_profile_begin(2), "sp_profile_begin")
            result = fn(*a, **kw)
            ms, launches = ctypes.c_double(), ctypes.c_uint64()
            _lib.check(lib.sp_profile_end(ctypes.byref(ms), ctypes.byref(launches), None), "sp_profile_end")
            assert launches.value == 1, (key, launches.value)
            device.setdefault(key, []).append(ms.value)
            return result
        return call

    def wall_of(fn, runs):
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return out, result

    n = 1024 * SIGNATURES
    lines = ["tools/quick_boundary.py: a %d-row ECDSA trace (%d signatures, 10 columns, log_m 24, 18 layers), unbound "
             "(stark.prove_ecdsa / stark.verify, 26 constraints) beside bound to its %d public felts "
             "(stark.prove_signatures / stark.verify_signatures, 26 + 5 boundary terms in 3 quotients); wall time of one "
             "call, provers median of %d, verifiers median of %d (spread = max - min), one warm-up each; device part = "
             "sp_profile brackets around the two new calls, passes of their own; TB/s = %d felts a point (3 distinct "
             "trace columns, 3 public columns, acc, out) over the dense call's device time"
             % (n, SIGNATURES, 5 * SIGNATURES, PROVE_RUNS, VERIFY_RUNS, DENSE_FELTS),
             "device %s, library %s" % (torch.cuda.get_device_name(0), lib.sp_build_info().decode())]
    plain_dense, plain_points = stark.boundary, stark.boundary_points
    for nq in QUERIES:
        stark.prove_ecdsa(*args, n_queries=nq, seed=nq)  # warm-up
        prove_ms, plain = wall_of(lambda: stark.prove_ecdsa(*args, n_queries=nq, seed=nq), PROVE_RUNS)
        stark.prove_signatures(*args, n_queries=nq, seed=nq)
        bound_ms, bound = wall_of(lambda: stark.prove_signatures(*args, n_queries=nq, seed=nq), PROVE_RUNS)
        assert stark.verify(plain, n_queries=nq) == (True, "ok")
        assert stark.verify_signatures(bound, n_queries=nq) == (True, "ok")
        verify_ms, ok = wall_of(lambda: stark.verify(plain), VERIFY_RUNS)
        assert ok == (True, "ok")
        verify_io_ms, ok = wall_of(lambda: stark.verify_signatures(bound), VERIFY_RUNS)
        assert ok == (True, "ok")
        device.clear()
        stark.boundary, stark.boundary_points = bracketed(plain_dense, "dense"), bracketed(plain_points, "points")
        try:
            for _ in range(PROVE_RUNS):
                stark.prove_signatures(*args, n_queries=nq, seed=nq)
            for _ in range(VERIFY_RUNS):
                assert stark.verify_signatures(bound) == (True, "ok")
        finally:
            stark.boundary, stark.boundary_points = plain_dense, plain_points
        pm, ps = median_spread(prove_ms)
        bm, bs = median_spread(bound_ms)
        vm, vs = median_spread(verify_ms)
        im, isp = median_spread(verify_io_ms)
        dm, ds = median_spread(device["dense"])
        qm, qs = median_spread(device["points"])
        lines.append("n_queries %2d   prove_ecdsa %9.3f ms (spread %8.3f)   prove_signatures %9.3f ms (spread %8.3f)   "
                     "verify %8.3f ms (spread %7.3f)   verify_signatures %8.3f ms (spread %7.3f)   sp_boundary_dev, 2^24 "
                     "points %.4f ms (spread %.4f) = %.2f TB/s   sp_boundary_points_dev, %3d points %.4f ms (spread %.4f)"
                     % (nq, pm, ps, bm, bs, vm, vs, im, isp, dm, ds, 32 * DENSE_FELTS * 4 * n / (dm * 1e-3) / 1e12,
                        2 * nq, qm, qs))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
