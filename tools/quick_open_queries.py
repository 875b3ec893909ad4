#!/usr/bin/env python3
"""The prover's query phase alone, on this commit and on a checkout of its parent: stark.prove of a 2^20-row Pedersen
trace (2048 hashes; M = 2^22, 16 committed FRI layers) at n_queries 8 and 64.  The phase starts when the transcript has
absorbed the final layer - the device is drained at that point, so the commit phase is out of the figure - and ends
when prove returns.  Each figure is the median of three proves (after one warm-up prove), with the spread max - min.

Each tree is measured in a process of its own (its own package, its own library); the processes run one after the
other, parent first.  The hook is the same in both: Transcript.absorb("final_layer"), which the parent has too.  The
sha256 of every proof is compared across the trees: the proofs must be identical.  For this commit the device part of
the phase (the one commit_open_kernel launch, from sp_profile_end) is reported as well.

    python tools/quick_open_queries.py PARENT_TREE [output file]     # PARENT_TREE: a built checkout of the parent
    python tools/quick_open_queries.py --child TREE                  # (what the above starts; prints one JSON line)"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES, QUERIES, RUNS = 2048, (8, 64), 3


def child(tree):
    sys.path.insert(0, os.path.join(tree, "stark-perpetual_amd"))
    sys.path.insert(0, os.path.join(tree, "tests"))
    import ctypes
    import torch
    import workloads as wl
    from starkperp import _lib, stark
    lib = _lib.ensure_init()
    new = hasattr(lib, "sp_commit_open_dev")
    pairs = wl.pedersen_pairs(HASHES, seed=20)
    xs = stark.felts_to_tensor([a for a, _ in pairs])
    ys = stark.felts_to_tensor([b for _, b in pairs])
    mark = {}
    absorb = stark.Transcript.absorb

    def hooked(self, label, *values):
        absorb(self, label, *values)
        if label == "final_layer":  # the commit phase is over: drain it, then the query phase starts
            torch.cuda.synchronize()
            if new:
                _lib.check(lib.sp_profile_begin(8), "sp_profile_begin")
            mark["t0"] = time.perf_counter()

    stark.Transcript.absorb = hooked
    stark.prove(xs, ys, n_queries=1, seed=99)  # warm-up: twiddles, scratch, the allocator's pools
    if new:
        lib.sp_profile_end(None, None, None)
    out = {"tree": tree, "lib_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "new": new,
           "rows": 512 * HASHES, "runs": {}}
    for nq in QUERIES:
        runs = []
        for seed in range(RUNS):
            proof = stark.prove(xs, ys, n_queries=nq, seed=seed)
            ms = 1e3 * (time.perf_counter() - mark["t0"])
            run = {"ms": ms, "sha256": hashlib.sha256(json.dumps(proof, sort_keys=True).encode()).hexdigest()}
            if new:
                dev, launches = ctypes.c_double(), ctypes.c_uint64()
                _lib.check(lib.sp_profile_end(ctypes.byref(dev), ctypes.byref(launches), None), "sp_profile_end")
                run.update(device_ms=dev.value, launches=launches.value)
            runs.append(run)
        out["runs"][str(nq)] = runs
    print("RESULT " + json.dumps(out))


def measure(tree):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True,
                         timeout=900)
    lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
    if run.returncode != 0 or not lines:
        raise SystemExit("measuring %s failed (%d):\n%s\n%s" % (tree, run.returncode, run.stdout[-2000:], run.stderr[-2000:]))
    return json.loads(lines[-1][7:])


def median_spread(values):
    v = sorted(values)
    return v[len(v) // 2], v[-1] - v[0]


def main():
    parent_tree = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "open_queries.txt")
    parent, new = measure(parent_tree), measure(ROOT)
    assert not parent["new"] and new["new"], "the first tree must be the parent's, without sp_commit_open_dev"
    lines = ["tools/quick_open_queries.py: query phase of stark.prove, %d-row Pedersen trace (%d hashes), from the absorbed "
             "final layer (device drained) to the return; median of %d proves, spread = max - min; one process per tree, "
             "parent first" % (new["rows"], HASHES, RUNS),
             "parent library sha256 %s" % parent["lib_sha256"], "new library sha256    %s" % new["lib_sha256"]]
    ok = True
    for nq in QUERIES:
        p, n = parent["runs"][str(nq)], new["runs"][str(nq)]
        same = [a["sha256"] for a in p] == [b["sha256"] for b in n]
        pm, ps = median_spread([r["ms"] for r in p])
        nm, ns = median_spread([r["ms"] for r in n])
        dm, ds = median_spread([r["device_ms"] for r in n])
        launches = sorted({r["launches"] for r in n})
        lines.append("n_queries %2d   parent %9.3f ms (spread %7.3f)   new %8.3f ms (spread %6.3f)   parent / new %6.1f   "
                     "device part %.4f ms (spread %.4f) in %s launch(es)   proofs identical: %s" % (
                         nq, pm, ps, nm, ns, pm / nm, dm, ds, "/".join(str(v) for v in launches), "yes" if same else "NO"))
        ok = ok and same and nm < pm - ps
    lines.append("new shorter than parent by more than the parent's spread at both counts, proofs identical: %s" % (
        "yes" if ok else "NO"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    assert ok, "the recorded run does not show what profiles/open_queries.txt is there to show"


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(os.path.abspath(sys.argv[2]))
    elif len(sys.argv) >= 2:
        main()
    else:
        raise SystemExit(__doc__)
