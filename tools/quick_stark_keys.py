#!/usr/bin/env python3
"""Batch square roots mod p (sp_felt_sqrt_batch) and key validity (sp_stark_key_y_batch with qy = NULL) at 2^12, 2^16
and 2^18 items: host-inclusive time of a call - NumPy buffers allocated outside the timing - and the kernel alone through
sp_profile_begin / sp_profile_end, median and p90 of the calls after a warm-up; beside them the host path the calls
replace (starkperp.math_utils.sqrt_mod, Python integers, timed on this machine's CPU in the same run) and what the code
predicts for a launch of one wave per SIMD.  No threshold is set: the numbers are recorded.  Every answer is checked
before anything is timed.  Each GPU step is a process of its own under its own `timeout` (one process at a time on the
device); the script stops at the first step that fails.
    python tools/quick_stark_keys.py [calls=24] [output file]"""
import ctypes
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stark-perpetual_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from starkperp import _lib, batch_np, math_utils  # noqa: E402
from evidence_stamp import lib_hash  # noqa: E402

STEP = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--step" else None
CALLS = int(sys.argv[3]) if STEP else (max(8, int(sys.argv[1])) if len(sys.argv) > 1 else 24)
WARMUP = 4
SIZES = (1 << 12, 1 << 16, 1 << 18)
P = batch_np.FIELD_PRIME
STEP_LIMIT = {"roots": 240, "valid": 240}  # seconds, per step
FIELD_OPS = 2338                           # csrc/fp29.hpp fe_sqrt
VALU_PER_OP = 156                          # instructions of one fe_mul (a fe_sqr has 126)
NS_PER_DEPENDENT = (2.5, 3.75)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(ms):
    ms = np.array(ms)
    return float(np.median(ms)), float(np.percentile(ms, 90))


def felts(n, seed):
    """n felts below p, about half of them squares."""
    a = np.random.default_rng(seed).integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(13)  # below 2^250
    return a


def step(name):
    lib = _lib.ensure_init()
    want_root = name == "roots"
    fn = lib.sp_felt_sqrt_batch if want_root else lib.sp_stark_key_y_batch
    result = {}
    for n in SIZES:
        a = felts(n, n)
        out = np.zeros((n, 4), dtype=np.uint64) if want_root else None
        st = np.zeros(n, dtype=np.uint8)

        def call():
            _lib.check(fn(ptr(a), None if out is None else ptr(out), ptr(st), n), name)

        call()
        # the answers, before anything is timed: a sample against Python integers
        vals = batch_np.ints_from_felts(a[:64])
        for i, v in enumerate(vals):
            c = v if want_root else (v * v * v + v + 0x6F21413EFBE40DE150E596D72F7A8C5609AD26C15C915C1F4CDFCB99CEE9E89) % P
            assert int(st[i]) == (0 if c == 0 or pow(c, (P - 1) // 2, P) == 1 else 1), i
            if want_root and st[i] == 0:
                r = batch_np.ints_from_felts(out[i:i + 1])[0]
                assert r * r % P == v and r <= P - r, i
        assert 0.3 < float((st == 0).mean()) < 0.7
        host = []
        for r in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            call()
            host.append(1e3 * (time.perf_counter() - t0))
        kernel = []
        ms, launches, units = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        for r in range(CALLS):
            _lib.check(lib.sp_profile_begin(1), "sp_profile_begin")
            call()
            _lib.check(lib.sp_profile_end(ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(units)), "sp_profile_end")
            assert launches.value == 1 and units.value == n
            kernel.append(ms.value)
        result[str(n)] = {"host": spread(host[WARMUP:]), "kernel": spread(kernel)}
    return result


def cpu_ms_per_root(count=64):
    """starkperp.math_utils.sqrt_mod (the Tonelli-Shanks loop the batch call replaces) on this machine's CPU."""
    rng = random.Random(1)
    squares = [pow(rng.randrange(1, P), 2, P) for _ in range(count)]
    t = []
    for a in squares:
        t0 = time.perf_counter()
        r = math_utils.sqrt_mod(a, P)
        t.append(1e3 * (time.perf_counter() - t0))
        assert r * r % P == a
    return spread(t)


def run_step(name):
    """One GPU step in a process of its own, under its own time limit; raises at the first failure."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT[name]), sys.executable, os.path.abspath(__file__), "--step", name, str(CALLS)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (name, out.returncode, out.stderr[-2000:]))
    print("step %s done" % name, flush=True)
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    if STEP:
        print("RESULT " + json.dumps(step(STEP)))
        return
    cpu = cpu_ms_per_root()
    results = {name: run_step(name) for name in ("roots", "valid")}
    chain = [FIELD_OPS * VALU_PER_OP * ns * 1e-6 for ns in NS_PER_DEPENDENT]
    lines = [
        "tools/quick_stark_keys.py: median / p90 of %d calls after %d; host = the whole host-pointer call, kernel = its one"
        " launch (sp_profile_begin/_end)" % (CALLS, WARMUP),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "host path replaced: starkperp.math_utils.sqrt_mod, Python integers, this machine's CPU: %.2f ms per root"
        " (p90 %.2f, 64 random squares)" % cpu,
        "predicted for one wave per SIMD (up to 2^16 items): %d field operations x %d dependent VALU instructions x"
        " %.2f - %.2f ns = %.2f - %.2f ms" % ((FIELD_OPS, VALU_PER_OP) + NS_PER_DEPENDENT + tuple(chain)),
    ]
    for name, title in (("roots", "sp_felt_sqrt_batch (roots)"), ("valid", "sp_stark_key_y_batch, qy = NULL (validity only)")):
        lines.append(title)
        for n in SIZES:
            r = results[name][str(n)]
            line = "    2^%-2d items   host %9.3f ms  p90 %9.3f ms   kernel %9.3f ms  p90 %9.3f ms   %8.1f ns per item (kernel)" % (
                (n.bit_length() - 1,) + tuple(r["host"]) + tuple(r["kernel"]) + (1e6 * r["kernel"][0] / n,))
            if name == "roots":
                line += "   Python on this CPU / host call = %.0f x" % (cpu[0] * n / r["host"][0])
            lines.append(line)
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stark_keys.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
