#!/usr/bin/env python3
"""What binding the statement costs: stark.prove_hashes beside stark.prove and stark.verify_hashes beside stark.verify on
the 2^20-row Pedersen trace (2048 hashes; M = 2^22, 16 committed FRI layers) at 8 and at 64 queries, same inputs, same
process.  Provers: median of 5 calls after one warm-up each.  Verifiers: median of 24 calls after one warm-up.  Device
part of the two new calls (sp_hash_io_boundary_dev: table build + the elementwise launch, one bracket;
sp_hash_io_boundary_points_dev: one launch) from sp_profile_begin / sp_profile_end around each call, in passes of
their own so that the bracket's waits stay out of the wall figures.  No threshold is fixed in advance: the file records
what was measured, against the unbound proof of the same run.

    python tools/quick_hash_io.py [output file]      # default profiles/hash_io.txt"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stark-perpetual_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
HASHES, QUERIES, PROVE_RUNS, VERIFY_RUNS = 2048, (8, 64), 5, 24


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hash_io.txt")
    import torch
    import workloads as wl
    from starkperp import _lib, stark
    lib = _lib.ensure_init()
    pairs = wl.pedersen_pairs(HASHES, seed=20)
    xs = stark.felts_to_tensor([a for a, _ in pairs])
    ys = stark.felts_to_tensor([b for _, b in pairs])
    device = {}

    def bracketed(fn, key):
        def call(*args, **kw):
            _lib.check(lib.sp_profile_begin(2), "sp_profile_begin")
            result = fn(*args, **kw)
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

    lines = ["tools/quick_hash_io.py: a %d-row Pedersen trace (%d hashes, log_m 22, 16 layers), unbound (stark.prove / "
             "stark.verify, 11 constraints) beside bound to its %d public felts (stark.prove_hashes / stark.verify_hashes, 11 "
             "+ 3 boundary quotients); wall time of one call, provers median of %d, verifiers median of %d (spread = max - "
             "min), one warm-up each; device part = sp_profile brackets around the two new calls, passes of their own"
             % (512 * HASHES, HASHES, 3 * HASHES, PROVE_RUNS, VERIFY_RUNS),
             "device %s, library %s" % (torch.cuda.get_device_name(0), lib.sp_build_info().decode())]
    plain_dense, plain_points = stark.hash_io_boundary, stark.hash_io_boundary_points
    for nq in QUERIES:
        stark.prove(xs, ys, n_queries=nq, seed=nq)  # warm-up
        prove_ms, plain = wall_of(lambda: stark.prove(xs, ys, n_queries=nq, seed=nq), PROVE_RUNS)
        stark.prove_hashes(xs, ys, n_queries=nq, seed=nq)
        bound_ms, bound = wall_of(lambda: stark.prove_hashes(xs, ys, n_queries=nq, seed=nq), PROVE_RUNS)
        assert stark.verify(plain, n_queries=nq) == (True, "ok") and stark.verify_hashes(bound, n_queries=nq) == (True, "ok")
        verify_ms, ok = wall_of(lambda: stark.verify(plain), VERIFY_RUNS)
        assert ok == (True, "ok")
        verify_io_ms, ok = wall_of(lambda: stark.verify_hashes(bound), VERIFY_RUNS)
        assert ok == (True, "ok")
        device.clear()
        stark.hash_io_boundary, stark.hash_io_boundary_points = bracketed(plain_dense, "dense"), bracketed(plain_points, "points")
        try:
            for _ in range(PROVE_RUNS):
                stark.prove_hashes(xs, ys, n_queries=nq, seed=nq)
            for _ in range(VERIFY_RUNS):
                assert stark.verify_hashes(bound) == (True, "ok")
        finally:
            stark.hash_io_boundary, stark.hash_io_boundary_points = plain_dense, plain_points
        pm, ps = median_spread(prove_ms)
        bm, bs = median_spread(bound_ms)
        vm, vs = median_spread(verify_ms)
        im, isp = median_spread(verify_io_ms)
        dm, ds = median_spread(device["dense"])
        qm, qs = median_spread(device["points"])
        lines.append("n_queries %2d   prove %9.3f ms (spread %8.3f)   prove_hashes %9.3f ms (spread %8.3f)   verify %8.3f ms "
                     "(spread %7.3f)   verify_hashes %8.3f ms (spread %7.3f)   sp_hash_io_boundary_dev, 2^22 points %.4f ms "
                     "(spread %.4f)   sp_hash_io_boundary_points_dev, %3d points %.4f ms (spread %.4f)"
                     % (nq, pm, ps, bm, bs, vm, vs, im, isp, dm, ds, 2 * nq, qm, qs))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
