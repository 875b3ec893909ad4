"""ISA-level check of the product-scanning field multiplication (csrc/fp29.hpp): compiled for gfx950 exactly as the
library compiles it, a scan form is multiply-adds and nothing that adds 64-bit values beside them - the carry of a
column enters the next column's chain as the addend of its first v_mad_i64_i32.  LLVM re-merges such a chain when it
can (it reassociates the carry behind the products and pays a v_lshl_add_u64 per column again); the register pin after
every accumulate step is what stops it, and this test is what notices if a compiler stops honouring it.

The probe (tests/isa/field_scan_probe.hip) has one kernel per operation and nothing else that multiplies, so the
counts are absolute.  The same probe built with the column forms must still show the 15 carry additions of fe_reduce:
that proves the probe counts what it claims to count.  tests/test_masked_walk_isa.py is the precedent."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stark-perpetual_amd", "csrc")
KERNELS = ("probe_fe_mul", "probe_fe_sqr", "probe_fe_mul_sub_mul")


def histograms(tmp, scan):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    out = tmp / ("field_scan_probe_%d.s" % scan)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), "-DPROBE_SCAN=%d" % scan,
           os.path.join(ROOT, "tests", "isa", "field_scan_probe.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    res = {}
    for k in KERNELS:
        a = text.index("\n%s:" % k)
        b = text.index("s_endpgm", a)
        body = [l.split(";")[0].strip() for l in text[a:b].splitlines()]
        ops = [l.split()[0] for l in body if l and not l.startswith(".") and not l.endswith(":")]
        res[k] = collections.Counter(re.sub(r"_(e32|e64|dpp|sdwa)$", "", o) for o in ops)
    return res


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    return histograms(tmp_path_factory.mktemp("isa_scan"), 1)


@pytest.fixture(scope="module")
def column(tmp_path_factory):
    return histograms(tmp_path_factory.mktemp("isa_col"), 0)


@pytest.mark.parametrize("kernel,mads", [("probe_fe_mul", 99), ("probe_fe_sqr", 63), ("probe_fe_mul_sub_mul", 180)])
def test_scan_form_is_multiply_adds_without_carry_additions(scan, kernel, mads):
    h = scan[kernel]
    assert h["v_mad_i64_i32"] == mads, h  # products + 18 reduction steps, a subtracted product included
    assert h["v_lshl_add_u64"] == 0, h
    assert h["v_add_co_u32"] == 0 and h["v_addc_co_u32"] == 0, h
    assert h["v_sub_co_u32"] == 0 and h["v_subb_co_u32"] == 0, h  # no 64-bit subtraction behind a multiplication
    assert h["v_mad_u64_u32"] == 0, h  # every limb stayed a 32-bit multiplicand


@pytest.mark.parametrize("kernel,mads", [("probe_fe_mul", 99), ("probe_fe_sqr", 63), ("probe_fe_mul_sub_mul", 180)])
def test_the_probe_sees_the_carry_additions_of_the_column_form(column, kernel, mads):
    h = column[kernel]
    assert h["v_mad_i64_i32"] == mads, h
    assert h["v_lshl_add_u64"] + h["v_add_co_u32"] >= 15, h
