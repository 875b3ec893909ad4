#!/usr/bin/env python3
"""Batch point arithmetic on the Stark curve (sp_ec_mult_batch, sp_ec_lincomb_batch, sp_ec_add_batch) at 2^12, 2^16 and
2^18 items: host-inclusive time of a call - NumPy buffers allocated outside the timing - and the kernel alone through
sp_profile_begin / sp_profile_end, median and p90 of the calls after a warm-up.  In the same run the yardstick: the
ladder verification (sp_ecdsa_verify_batch under SP_VERIFY_POLICY_LADDER, point keys, valid signatures) at the same
sizes - host-inclusive, and its kernel between two events around sp_ecdsa_verify_batch_dev on device tensors (that
launch is not bracketed by sp_profile_begin).  Beside them the host path the calls replace
(starkperp.math_utils.ec_mult, Python integers, timed on this machine's CPU).  No threshold is set: the numbers are
recorded.  A sample of every answer is checked against Python integers before anything is timed.  Each GPU step is a
process of its own under its own `timeout` (one process at a time on the device); the script stops at the first step
that fails.
    python tools/quick_ec_points.py [calls=24] [output file]"""
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
P, N = batch_np.FIELD_PRIME, batch_np.EC_ORDER
GEN = (0x1EF15C18599971B7BECED415A40F0C7DEACFD9B0D1819E03D723D8BC943CFCA,
       0x5668060AA49730B7BE4801DF46EC62DE53ECD11ABE43A32873000C36E8DC1F)
STEPS = ("mult", "lincomb", "add", "verify", "alternate")
STEP_LIMIT = 300  # seconds, per step
SP_VERIFY_POLICY_LADDER = 1


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(ms):
    ms = np.array(ms)
    return float(np.median(ms)), float(np.percentile(ms, 90))


def scalars(n, seed):
    """n scalars in [1, 2^251), all below EC_ORDER."""
    a = np.random.default_rng(seed).integers(1, 2**63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(12)
    return a


def public_keys(lib, d):
    n = d.shape[0]
    qx, qy = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _lib.check(lib.sp_public_key_batch(ptr(d), ptr(qx), ptr(qy), ptr(st), n), "sp_public_key_batch")
    assert not st.any()
    return qx, qy


def ref_lincomb(a, b, pt):
    """a G + b pt in Python integers (math_utils, as the reference computes it)."""
    return math_utils.ec_add(math_utils.ec_mult(a, GEN, 1, P), math_utils.ec_mult(b, pt, 1, P), P)


def step_points(lib, name):
    fn = getattr(lib, "sp_ec_%s_batch" % name)
    result = {}
    for n in SIZES:
        px, py = public_keys(lib, scalars(n, n + 1))
        k, b = scalars(n, n + 2), scalars(n, n + 3)
        qx, qy = public_keys(lib, scalars(n, n + 4))
        rx, ry = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        args = {"mult": [k, px, py], "lincomb": [k, b, px, py], "add": [px, py, qx, qy]}[name]
        extra = [0] if name == "add" else []

        def call():
            _lib.check(fn(*[ptr(a) for a in args], *extra, ptr(rx), ptr(ry), ptr(st), n), name)

        call()
        assert not st.any()
        # the answers, before anything is timed: a sample against Python integers
        cols = [batch_np.ints_from_felts(a[:6]) for a in args]
        got = list(zip(batch_np.ints_from_felts(rx[:6]), batch_np.ints_from_felts(ry[:6])))
        for i in range(6):
            if name == "mult":
                want = math_utils.ec_mult(cols[0][i], (cols[1][i], cols[2][i]), 1, P)
            elif name == "lincomb":
                want = ref_lincomb(cols[0][i], cols[1][i], (cols[2][i], cols[3][i]))
            else:
                want = math_utils.ec_add((cols[0][i], cols[1][i]), (cols[2][i], cols[3][i]), P)
            assert got[i] == tuple(want), (name, n, i)
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


def step_verify(lib):
    import torch
    _lib.check(lib.sp_ecdsa_set_verify_policy(SP_VERIFY_POLICY_LADDER), "sp_ecdsa_set_verify_policy")
    result = {}
    for n in SIZES:
        d, z = scalars(n, n + 5), scalars(n, n + 6)
        z[:, 3] >>= np.uint64(1)  # below 2^250
        qx, qy = public_keys(lib, d)
        r, s = batch_np.sign_many(z, d)
        res = np.zeros(n, dtype=np.uint8)

        def call():
            _lib.check(lib.sp_ecdsa_verify_batch(ptr(z), ptr(r), ptr(s), ptr(qx), ptr(qy), ptr(res), n), "verify")

        call()
        assert (res == 1).all()
        host = []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            call()
            host.append(1e3 * (time.perf_counter() - t0))
        dev = [torch.from_numpy(a.view(np.int64)).cuda() for a in (z, r, s, qx, qy)]
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        kernel = []
        for i in range(WARMUP + CALLS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            _lib.check(lib.sp_ecdsa_verify_batch_dev(*[a.data_ptr() for a in dev], out.data_ptr(), n, stream.cuda_stream),
                       "sp_ecdsa_verify_batch_dev")
            t1.record(stream)
            t1.synchronize()
            kernel.append(t0.elapsed_time(t1))
        assert bool((out == 1).all())
        result[str(n)] = {"host": spread(host[WARMUP:]), "kernel": spread(kernel[WARMUP:])}
    return result


def step_alternate(lib):
    """The comparison the ratios are taken from: the three ladder kernels in ONE process, on device tensors of one
    stream, alternating call by call, each between two events - the same clock, the same clock state."""
    import torch
    result = {}
    for n in SIZES:
        d, z = scalars(n, n + 5), scalars(n, n + 6)
        z[:, 3] >>= np.uint64(1)
        qx, qy = public_keys(lib, d)
        r, s = batch_np.sign_many(z, d)
        to_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()  # noqa: E731
        z, r, s, qx, qy, k, b = (to_dev(a) for a in (z, r, s, qx, qy, scalars(n, n + 2), scalars(n, n + 3)))
        rx, ry = torch.zeros_like(qx), torch.zeros_like(qy)
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        h = stream.cuda_stream
        calls = {
            "verify": lambda: lib.sp_ecdsa_verify_batch_dev(*[a.data_ptr() for a in (z, r, s, qx, qy)], out.data_ptr(), n, h),
            "mult": lambda: lib.sp_ec_mult_batch_dev(*[a.data_ptr() for a in (k, qx, qy, rx, ry)], out.data_ptr(), n, h),
            "lincomb": lambda: lib.sp_ec_lincomb_batch_dev(*[a.data_ptr() for a in (k, b, qx, qy, rx, ry)], out.data_ptr(), n, h),
        }
        times = {name: [] for name in calls}
        for i in range(WARMUP + CALLS):
            for name, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                _lib.check(fn(), name)
                t1.record(stream)
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
                assert bool((out == (1 if name == "verify" else 0)).all()), name
        result[str(n)] = {name: spread(t[WARMUP:]) for name, t in times.items()}
    return result


def cpu_ms_per_mult(count=50):
    """starkperp.math_utils.ec_mult (the double-and-add the batch call replaces) on this machine's CPU."""
    rng = random.Random(1)
    t = []
    for _ in range(count):
        k = rng.randrange(1, N)
        t0 = time.perf_counter()
        math_utils.ec_mult(k, GEN, 1, P)
        t.append(1e3 * (time.perf_counter() - t0))
    return spread(t)


def run_step(name):
    """One GPU step in a process of its own, under its own time limit; raises at the first failure."""
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", name, str(CALLS)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit("step %s failed (%d): %s" % (name, out.returncode, out.stderr[-2000:]))
    print("step %s done" % name, flush=True)
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    if STEP:
        lib = _lib.ensure_init()
        steps = {"verify": step_verify, "alternate": step_alternate}
        print("RESULT " + json.dumps(steps[STEP](lib) if STEP in steps else step_points(lib, STEP)))
        return
    cpu = cpu_ms_per_mult()
    results = {name: run_step(name) for name in STEPS}
    lines = [
        "tools/quick_ec_points.py: median / p90 of %d calls after %d; host = the whole host-pointer call, kernel = its one"
        " launch (sp_profile_begin/_end; the verification's: events around sp_ecdsa_verify_batch_dev)" % (CALLS, WARMUP),
        "library sha256 %s" % lib_hash(_lib.LIB_PATH),
        "host path replaced: starkperp.math_utils.ec_mult, Python integers, this machine's CPU: %.2f ms per multiplication"
        " (p90 %.2f, 50 seeded scalars on EC_GEN)" % cpu,
    ]
    titles = (("mult", "sp_ec_mult_batch (k P)"), ("lincomb", "sp_ec_lincomb_batch (a G + b P)"),
              ("add", "sp_ec_add_batch (P + Q)"),
              ("verify", "yardstick: sp_ecdsa_verify_batch, SP_VERIFY_POLICY_LADDER, point keys, valid signatures"))
    for name, title in titles:
        lines.append(title)
        for n in SIZES:
            r = results[name][str(n)]
            line = "    2^%-2d items   host %9.3f ms  p90 %9.3f ms   kernel %9.3f ms  p90 %9.3f ms   %8.1f ns per item (kernel)" % (
                (n.bit_length() - 1,) + tuple(r["host"]) + tuple(r["kernel"]) + (1e6 * r["kernel"][0] / n,))
            line += "   %.2e /s" % (n / (1e-3 * r["kernel"][0]))
            if name == "mult":
                line += "   Python on this CPU / host call = %.0f x" % (cpu[0] * n / r["host"][0])
            lines.append(line)
    lines.append("the three ladder kernels alternating in one process (_dev calls on one stream, events around each): the"
                 " figures the ratios are taken from (the kernel columns above are taken inside host calls, with the"
                 " copies of a call between two launches, the verification's between back-to-back _dev calls)")
    for n in SIZES:
        r = results["alternate"][str(n)]
        lines.append("    2^%-2d items   verification %7.3f ms  p90 %7.3f   mult %7.3f ms  p90 %7.3f  (%.2f of the verification's)"
                     "   lincomb %7.3f ms  p90 %7.3f  (%.2f)" % (
                         (n.bit_length() - 1,) + tuple(r["verify"]) + tuple(r["mult"]) + (r["mult"][0] / r["verify"][0],)
                         + tuple(r["lincomb"]) + (r["lincomb"][0] / r["verify"][0],)))
    text = "\n".join(lines)
    print(text)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ec_points.txt")
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
