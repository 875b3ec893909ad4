#!/usr/bin/env python3
"""stark.verify_builtins at 8 and at 64 queries on two prove_builtins proofs - the n = 2048 proof of
tests/test_gpu_builtins.py::test_combined_builtin_trace_proves_and_verifies (4 hashes, 2 signatures, 40 range checks)
and, unless --small is given, the 2^23-row order-batch proof of test_builtin_usage_of_a_4096_order_batch_in_one_trace:
the median of 24 calls (after one warm-up call), the device part of its one own launch (builtins_points_kernel, from
sp_profile_begin / sp_profile_end around each call, in a second pass of 24 so that the bracket's waits stay out of the
first figure), and oracle/stark_ref.verify_builtins_proof with the C oracle's hash on the same proof and box (median of
3; once for the large proof).  No ratio is fixed in advance: the file records what was measured.

    python tools/quick_builtins_verify.py [--small] [output file]      # default profiles/builtins_verify.txt"""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stark-perpetual_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
QUERIES, RUNS, ORACLE_RUNS = (8, 64), 24, 3


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def small_instances():
    from test_gpu_builtins import small_batch
    return small_batch(random.Random(62), 4, 2, 40)


def order_batch_instances():
    """The statement of test_builtin_usage_of_a_4096_order_batch_in_one_trace."""
    import workloads as wl
    from starkperp import batch, perpetual_messages as pm
    orders = wl.limit_orders(4096, seed=2)
    keys = wl.private_keys(1024, seed=12)
    words = [pm._limit_order_words(*wl.order_args(o)) for o in orders]
    hash_inputs, acc = [], [w[0] for w in words]
    for k in range(1, 5):
        ys = [w[k] for w in words]
        hash_inputs += list(zip(acc, ys))
        acc = batch.pedersen_hash_many(acc, ys)
    zs = [z % 2**251 for z in acc]
    pubs = batch.public_keys_many(keys)
    sigs = batch.sign_many(zs, [keys[o["key_index"]] for o in orders])
    signatures = [(z, r, s, pubs[o["key_index"]]) for z, (r, s), o in zip(zs, sigs, orders)]
    values = []
    for o, z in zip(orders, acc):
        values += [o["amount_synthetic"], o["amount_collateral"], o["max_amount_fee"], o["nonce"], o["position_id"],
                   o["expiration_timestamp"], z & (2**128 - 1), (z >> 128) & (2**59 - 1)]
    return hash_inputs, signatures, values


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small_only = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "builtins_verify.txt")
    import torch
    from oracle import cref
    from oracle import stark_ref as S
    from starkperp import _lib, stark
    lib = _lib.ensure_init()
    chash = lambda a, b: cref.pedersen_hash_many([a], [b])[0][0]
    device = []
    plain = stark.builtins_eval_points

    def bracketed(*a, **kw):
        _lib.check(lib.sp_profile_begin(2), "sp_profile_begin")
        result = plain(*a, **kw)
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        _lib.check(lib.sp_profile_end(ctypes.byref(ms), ctypes.byref(launches), None), "sp_profile_end")
        assert launches.value == 1, launches.value
        device.append(ms.value)
        return result

    lines = ["tools/quick_builtins_verify.py: stark.verify_builtins of prove_builtins proofs over pedersen + ecdsa + rc16; "
             "wall time of one call, median of %d (spread = max - min) after one warm-up; device part = the one launch of "
             "builtins_points_kernel, second pass of %d; oracle = oracle/stark_ref.verify_builtins_proof with the C "
             "oracle's hash, same proof, same box, median of %d (one run for the 2^23-row proof)" % (RUNS, RUNS, ORACLE_RUNS),
             "device %s, library %s" % (torch.cuda.get_device_name(0), lib.sp_build_info().decode())]
    print("\n".join(lines), flush=True)
    cases = [("n = 2048 (4 hashes, 2 signatures, 40 range checks)", small_instances, ORACLE_RUNS)]
    if not small_only:
        cases.append(("n = 2^23 (the 4096-order batch: 16384 hashes, 4096 signatures, 32768 range checks)",
                      order_batch_instances, 1))
    for title, make, oracle_runs in cases:
        hashes, signatures, values = make()
        for nq in QUERIES:
            proof = stark.prove_builtins(hashes, signatures, values, n_queries=nq, seed=nq)
            torch.cuda.empty_cache()
            assert stark.verify_builtins(proof, n_queries=nq) == (True, "ok")  # warm-up
            wall = []
            for _ in range(RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ok = stark.verify_builtins(proof)
                wall.append(1e3 * (time.perf_counter() - t0))
                assert ok == (True, "ok")
            del device[:]
            stark.builtins_eval_points = bracketed
            try:
                for _ in range(RUNS):
                    assert stark.verify_builtins(proof) == (True, "ok")
            finally:
                stark.builtins_eval_points = plain
            oracle = []
            for _ in range(oracle_runs):
                t0 = time.perf_counter()
                ok = S.verify_builtins_proof(proof, hash2=chash)
                oracle.append(1e3 * (time.perf_counter() - t0))
                assert ok == (True, "ok")
            wm, ws = median_spread(wall)
            dm, ds = median_spread(device)
            om, osp = median_spread(oracle)
            lines.append("%s, log_m %d, %d layers, n_queries %2d   stark.verify_builtins %9.3f ms (spread %7.3f)   "
                         "builtins_points_kernel, %3d points %.4f ms (spread %.4f)   oracle verify_builtins_proof %10.3f ms "
                         "(%d run%s, spread %8.3f)" % (title, proof["n"].bit_length() + 1, len(proof["layer_roots"]), nq, wm,
                                                       ws, 2 * nq, dm, ds, om, oracle_runs, "s" if oracle_runs > 1 else "",
                                                       osp))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
