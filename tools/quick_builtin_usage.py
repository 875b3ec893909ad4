#!/usr/bin/env python3
"""What binding the statement of the builtins proof costs: stark.prove_builtin_usage beside stark.prove_builtins and
stark.verify_builtin_usage beside stark.verify_builtins on the 4096-order batch (16 384 hashes, 4096 signatures, 32 768
range checks: n = 2^23, M = 2^25) at 8 and at 64 queries, same inputs, same process.  Provers: median of 5 calls after
one warm-up each.  Verifiers: median of 24 calls after one warm-up.

Device parts through sp_profile_begin / sp_profile_end, in passes of their own on the committed trace LDE of one
prover run with seeded public columns (the time does not depend on the values): sp_builtins_boundary_dev at mask 7;
at mask 3 beside the chain of two sp_boundary_dev calls (pedersen_io, then ecdsa_io with acc = out) on the same
columns; sp_builtins_boundary_points_dev at 16 and at 128 points, with and without the rc16 segment (whose 2^20
coefficients are 4096 Horner steps per lane); sp_boundary_combine_dev on the rc16 column (2^20 items) and on the
ECDSA terms.  Host shares of the verifier: packing the public inputs, the transcript's statement, w_i.  Peak device
memory of the two provers (torch's allocator).  No threshold is fixed in advance: the file records what was measured.

    python tools/quick_builtin_usage.py [--small] [output file]     # default profiles/builtin_usage.txt
--small runs the same passes on an n = 2048 statement (a smoke run of the tool, not a measurement to quote)."""
import ctypes
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stark-perpetual_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
QUERIES, PROVE_RUNS, VERIFY_RUNS, DEVICE_RUNS = (8, 64), 5, 24, 9
ALL = ["pedersen", "ecdsa", "rc16"]


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def main():
    args = [a for a in sys.argv[1:] if a != "--small"]
    small = "--small" in sys.argv[1:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "builtin_usage.txt")
    import torch
    import quick_builtins_verify as qbv
    from starkperp import _lib, stark
    lib = _lib.ensure_init()
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def wall_of(fn, runs):
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return out, result

    def device_of(fn, launches_want, runs=DEVICE_RUNS):
        out = []
        for _ in range(runs + 1):  # the first is a warm-up
            _lib.check(lib.sp_profile_begin(4), "sp_profile_begin")
            fn()
            ms, launches = ctypes.c_double(), ctypes.c_uint64()
            _lib.check(lib.sp_profile_end(ctypes.byref(ms), ctypes.byref(launches), None), "sp_profile_end")
            assert launches.value == launches_want, launches.value
            out.append(ms.value)
        return median_spread(out[1:])

    hashes, signatures, values = qbv.small_instances() if small else qbv.order_batch_instances()
    say("tools/quick_builtin_usage.py: the builtin usage of %d hashes, %d signatures and %d range checks in one trace, "
        "unbound (stark.prove_builtins / stark.verify_builtins, 11 + 26 + 8 constraints) beside bound to its statement "
        "(stark.prove_builtin_usage / stark.verify_builtin_usage, + 3 + 5 + 1 boundary terms in 7 quotients); wall time "
        "of one call, provers median of %d, verifiers median of %d (spread = max - min), one warm-up each; device parts = "
        "sp_profile brackets, median of %d after one warm-up, in passes of their own"
        % (len(hashes), len(signatures), len(values), PROVE_RUNS, VERIFY_RUNS, DEVICE_RUNS))
    say("device %s, library %s" % (torch.cuda.get_device_name(0), lib.sp_build_info().decode()))
    proofs = {}
    for nq in QUERIES:
        stark.prove_builtins(hashes, signatures, values, n_queries=nq, seed=nq)  # warm-up
        torch.cuda.reset_peak_memory_stats()
        prove_ms, plain = wall_of(lambda: stark.prove_builtins(hashes, signatures, values, n_queries=nq, seed=nq), PROVE_RUNS)
        peak_plain = torch.cuda.max_memory_allocated()
        stark.prove_builtin_usage(hashes, signatures, values, n_queries=nq, seed=nq)
        torch.cuda.reset_peak_memory_stats()
        bound_ms, bound = wall_of(lambda: stark.prove_builtin_usage(hashes, signatures, values, n_queries=nq, seed=nq),
                                  PROVE_RUNS)
        peak_bound = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
        assert stark.verify_builtins(plain, n_queries=nq) == (True, "ok")
        assert stark.verify_builtin_usage(bound, n_queries=nq) == (True, "ok")
        verify_ms, ok = wall_of(lambda: stark.verify_builtins(plain), VERIFY_RUNS)
        assert ok == (True, "ok")
        verify_io_ms, ok = wall_of(lambda: stark.verify_builtin_usage(bound), VERIFY_RUNS)
        assert ok == (True, "ok")
        proofs[nq] = bound
        n = bound["n"]
        say("n = %d, n_queries %2d   prove_builtins %10.3f ms (spread %9.3f)   prove_builtin_usage %10.3f ms (spread %9.3f)"
            "   verify_builtins %8.3f ms (spread %7.3f)   verify_builtin_usage %8.3f ms (spread %7.3f)   peak device "
            "memory of a prover call %.2f GiB unbound, %.2f GiB bound"
            % ((n, nq) + median_spread(prove_ms) + median_spread(bound_ms) + median_spread(verify_ms)
               + median_spread(verify_io_ms) + (peak_plain / 2**30, peak_bound / 2**30)))
        del plain
    # ---- host shares of the verifier, on the 8-query proof ----
    proof = proofs[QUERIES[0]]
    pub, n = proof["public_inputs"], proof["n"]
    shares = {}
    shares["packing (rc16_fill_tensor, the hash and signature columns)"], _ = wall_of(
        lambda: stark._builtin_usage_columns(dict(pub, signatures=[]), n, ["pedersen", "rc16"], "cuda"), 5)
    shares["w_i = s_i^-1 mod N (one modular inversion) and the signature columns"], _ = wall_of(
        lambda: stark._builtin_usage_columns(pub, n, ["ecdsa"], "cuda"), 5)
    shares["the transcript's statement (flat list and its SHA-256 absorb)"], _ = wall_of(
        lambda: stark.Transcript("builtins_io", n, proof["shift"], proof["seed"], stark._builtin_usage_flat(pub, ALL)), 5)
    shares["the signatures' side conditions (unbound verifier too)"], _ = wall_of(
        lambda: stark._public_inputs_ok("ecdsa", n, [v for sig in pub["signatures"] for v in sig]), 5)
    for what, ms in shares.items():
        say("host share of verify_builtin_usage: %-75s %9.3f ms (spread %8.3f), median of 5" % ((what,) + median_spread(ms)))
    # ---- device parts ----
    c = stark._commit_builtins(hashes, signatures, values, 1, 6, stark.FIELD_GEN, None)
    trace_lde = c["trace_lde"]
    del c
    torch.cuda.empty_cache()
    M = 4 * n
    g = torch.Generator(device="cuda").manual_seed(7)
    seeded = lambda *shape: torch.randint(0, 2**59, shape + (4,), dtype=torch.int64, device="cuda", generator=g)
    rng = random.Random(9)
    alphas = [rng.randrange(stark.FIELD_PRIME) for _ in range(9)]
    pub_lde = seeded(7, M)
    out = torch.empty((M, 4), dtype=torch.int64, device="cuda")
    d7 = device_of(lambda: stark.builtins_boundary(ALL, trace_lde, pub_lde, n, alphas, acc=out, out=out), 1)
    felts7 = 6 + 7 + 2  # s, px; m, qx, qy; acc - six distinct trace columns; seven public; acc and out
    say("sp_builtins_boundary_dev, mask 7, 2^%d points, acc = out: %.4f ms (spread %.4f) = %.2f TB/s over %d felts a point "
        "(6 distinct trace columns, 7 public columns, acc, out)"
        % ((M.bit_length() - 1,) + d7 + (32 * felts7 * M / (d7[0] * 1e-3) / 1e12, felts7)))
    two = ALL[:2]
    d3 = device_of(lambda: stark.builtins_boundary(two, trace_lde[:14], pub_lde[:6], n, alphas[:8], acc=out, out=out), 1)

    def chain():
        stark.boundary("pedersen_io", trace_lde[0:4], pub_lde[0:3], n, alphas[0:3], acc=out, out=out)
        stark.boundary("ecdsa_io", trace_lde[4:14], pub_lde[3:6], n, alphas[3:8], acc=out, out=out)
    dc = device_of(chain, 2)
    say("sp_builtins_boundary_dev, mask 3, acc = out: %.4f ms (spread %.4f)   beside the chain sp_boundary_dev(pedersen_io) "
        "+ sp_boundary_dev(ecdsa_io, acc = out) on the same columns: %.4f ms (spread %.4f)" % (d3 + dc))
    del pub_lde, out
    torch.cuda.empty_cache()
    cols = {"pedersen": [seeded(n // 512) for _ in range(3)], "ecdsa": [seeded(n // 1024) for _ in range(5)],
            "rc16": [seeded(n // 8)]}
    dr = device_of(lambda: stark.boundary_combine([0], 1, cols["rc16"], alphas[8:]), 1)
    de = device_of(lambda: stark.boundary_combine([0, 1, 1, 1, 2], 3, cols["ecdsa"], alphas[3:8]), 1)
    say("sp_boundary_combine_dev: the rc16 column, %d items %.4f ms (spread %.4f)   the five ECDSA terms, %d items %.4f ms "
        "(spread %.4f)" % ((n // 8,) + dr + (n // 1024,) + de))
    coef = stark.builtins_boundary_coefficients(ALL, cols, n, alphas)
    coef2 = stark.builtins_boundary_coefficients(two, cols, n, alphas[:8])
    for count in (16, 128):
        pos = torch.randint(0, M, (count,), dtype=torch.int64, device="cuda", generator=g)
        cur = trace_lde[:, pos, :].permute(1, 0, 2).contiguous()
        cur2 = cur[:, :14].contiguous()
        p7 = device_of(lambda: stark.builtins_boundary_points(ALL, n, coef, alphas, stark.FIELD_GEN, pos, cur), 1)
        p3 = device_of(lambda: stark.builtins_boundary_points(two, n, coef2, alphas[:8], stark.FIELD_GEN, pos, cur2), 1)
        say("sp_builtins_boundary_points_dev, %3d points: mask 7 %.4f ms (spread %.4f)   mask 3 (no rc16) %.4f ms (spread "
            "%.4f): the rc16 segment's %d coefficients are %d Horner steps per lane"
            % ((count,) + p7 + p3 + (n // 8, max(1, n // 8 // 256))))


if __name__ == "__main__":
    main()
