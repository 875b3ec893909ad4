#!/usr/bin/env python3
"""stark.verify on a 2^20-row Pedersen proof (2048 hashes; M = 2^22, 16 committed FRI layers) at 8 and at 64 queries:
the median of 24 calls (after one warm-up call), the device part of its two own launches (air_points_kernel and
fri_check_kernel, from sp_profile_begin / sp_profile_end around each call, in a second pass of 24 so that the bracket's
waits stay out of the first figure), and oracle/stark_ref.verify_proof with the C oracle's hash on the same proof
and box (median of 3).  No ratio is fixed in advance: the file records what was measured.

    python tools/quick_stark_verify.py [output file]      # default profiles/stark_verify.txt"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stark-perpetual_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
HASHES, QUERIES, RUNS, ORACLE_RUNS = 2048, (8, 64), 24, 3


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stark_verify.txt")
    import torch
    import workloads as wl
    from oracle import cref
    from oracle import stark_ref as S
    from starkperp import _lib, stark
    lib = _lib.ensure_init()
    pairs = wl.pedersen_pairs(HASHES, seed=20)
    xs = stark.felts_to_tensor([a for a, _ in pairs])
    ys = stark.felts_to_tensor([b for _, b in pairs])
    chash = lambda a, b: cref.pedersen_hash_many([a], [b])[0][0]
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

    lines = ["tools/quick_stark_verify.py: stark.verify of a %d-row Pedersen proof (%d hashes, log_m 22, 16 layers); wall "
             "time of one call, median of %d (spread = max - min) after one warm-up; device part = the one launch of each "
             "of the two verifier kernels, second pass of %d; oracle = oracle/stark_ref.verify_proof with the C oracle's "
             "hash, median of %d, same proof, same box" % (512 * HASHES, HASHES, RUNS, RUNS, ORACLE_RUNS),
             "device %s, library %s" % (torch.cuda.get_device_name(0), lib.sp_build_info().decode())]
    plain_points, plain_fri = stark.air_eval_points, stark.fri_check_queries
    for nq in QUERIES:
        proof = stark.prove(xs, ys, n_queries=nq, seed=nq)
        assert stark.verify(proof, n_queries=nq) == (True, "ok")  # warm-up
        wall = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ok = stark.verify(proof)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert ok == (True, "ok")
        device.clear()
        stark.air_eval_points, stark.fri_check_queries = bracketed(plain_points, "points"), bracketed(plain_fri, "fri")
        try:
            for _ in range(RUNS):
                assert stark.verify(proof) == (True, "ok")
        finally:
            stark.air_eval_points, stark.fri_check_queries = plain_points, plain_fri
        oracle = []
        for _ in range(ORACLE_RUNS):
            t0 = time.perf_counter()
            ok = S.verify_proof(proof, hash2=chash)
            oracle.append(1e3 * (time.perf_counter() - t0))
            assert ok == (True, "ok")
        wm, ws = median_spread(wall)
        pm, ps = median_spread(device["points"])
        fm, fs = median_spread(device["fri"])
        om, osp = median_spread(oracle)
        lines.append("n_queries %2d   stark.verify %9.3f ms (spread %7.3f)   air_points_kernel, %3d points %.4f ms (spread "
                     "%.4f)   fri_check_kernel, %4d items %.4f ms (spread %.4f)   oracle verify_proof %10.3f ms (spread "
                     "%8.3f)" % (nq, wm, ws, 2 * nq, pm, ps, 16 * nq, fm, fs, om, osp))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
