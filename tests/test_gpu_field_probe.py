"""The DEVICE build of csrc/fp29.hpp, csrc/curve.hpp and csrc/quad.hpp against Python integers.

tests/test_field_host.py and tests/test_field_scan_host.py compile the first two headers with g++; that build never
sees what sits behind __HIP_DEVICE_COMPILE__ (the alignbit unpack, the register pins of fe_reduce / fe_scan, the bare
v_rcp_f64 that steers lehmer_step, the wave votes that end the gcd loops), and quad.hpp does not compile for the host
at all.  Here a stand-alone probe (tests/gpu/field_probe.hip) runs one operation per process on raw limbs, and every
result is compared with Python integers (tests/field_probe_lib.py; tests/test_field_probe_cpu.py verifies that model
on the CPU).  The inputs are the ones whole hashes and signatures never produce: the divsteps fallback of the
double-steered inversion (taken by a whole wave when one lane asks for it), multiples of p, unreduced representatives,
P + P and P - P.  That the fallback really ran is read from lehmer_bezout's own answer, not assumed: for a
lane-private op from a launch of the lehmer_bezout op on the same input with the same n (the same waves), for a quad
op from a lane-private lehmer_bezout on the same values inside the same kernel.  Neither is the op's own branch; the
vote is the same function of the same wave.

All comparisons are exact.  After the first probe invocation that does not end with status 0 the module starts
nothing further on the GPU: the remaining tests fail."""
import numpy as np
import pytest

import field_probe_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return L.Probe(tmp_path_factory.mktemp("field_probe"))


@pytest.fixture(scope="module")
def twin():
    return L.Twin()


def report(op, items, fallback=None, extra=""):
    print("field_probe %-28s %7d items%s%s" % (op, items, "" if fallback is None else ", %5d through the fallback" % fallback, extra))


def test_a_pack_unpack(probe):
    vals, arr = L.pack_words()
    report("fe_pack(fe_unpack)", L.check_pack(vals, probe.run("pack_unpack", arr)[0], probe.run("unpack", arr)[0]))


def test_b_multiplications(probe, twin):
    """Scan limbs == column limbs, N-form, value 2^261 == the integer expression (mod p), and limb for limb what the
    host twin returns: the host's bound checks (SP_CHECK_BOUNDS) then speak for the device build too."""
    for name, inp in (("every 6-tuple of the extreme patterns", L.mul_tuples()), ("random N-form", L.mul_random())):
        out, _ = probe.run("mul_forms", inp)
        n = L.check_mul(inp, out)
        host, _ = twin.run("mul_forms", inp)
        bad = np.nonzero((out != host).any(axis=(1, 2)))[0]
        assert len(bad) == 0, "device limbs differ from the host twin's, first at item %d" % bad[0]
        report("5 forms x (column, scan)", n, extra=" (%s)" % name)


def test_c_small_ops(probe):
    for op, (inp, exp) in L.small_inputs().items():
        out, flags = probe.run(op, inp)
        report(op, L.check_small(op, inp, exp, out, flags))


def test_d_group_law(probe):
    for op in L.GROUP_OPS:
        inp, exp = L.group_inputs(op)
        out, flags = probe.run(op, inp)
        items, exceptional = L.check_group(op, exp, out, flags)
        report(op, items, extra=", %d exceptional (ZZ3 = 0)" % exceptional)


def wave_flags(flags, per=64):
    """lehmer_bezout's answer is wave-wide: every lane of a wave must report the same.  Returns one flag per wave."""
    f = flags[:, 0]
    waves = [f[i:i + per] for i in range(0, len(f), per)]
    assert all((w == w[0]).all() for w in waves), "lanes of one wave disagree about the wave's vote"
    return [int(w[0]) for w in waves]


def expect_fallback(which, waves):
    if which == 1:  # the seed of class R converges on the host twin (test_field_probe_cpu.py): nobody falls back
        assert all(w == 1 for w in waves), waves
    if which in (2, 3):  # one S lane takes its whole wave to the divsteps form
        assert all(w == 0 for w in waves), waves


@pytest.mark.parametrize("which", L.LAYOUTS)
def test_e_inversions(probe, which):
    for family, (ops, bezout, m, kw) in sorted(L.INV_FAMILIES.items()):
        got = L.inv_input(family, which)
        if got is None:
            continue
        inp, vals, cls = got
        for n in (len(inp) - L.PARTIAL, len(inp)):  # whole waves only, then with the partial last wave
            out, flags = probe.run(bezout, inp, n)
            L.check_bezout(bezout, vals, out, flags)
            waves = wave_flags(flags)
            expect_fallback(which, waves)
            fallback = int((flags[:, 0] == 0).sum())
            report(bezout, n, fallback, " (layout %d, %s)" % (which, family))
            for op in ops:
                L.check_inv(op, vals, probe.run(op, inp, n)[0])
                report(op, n, fallback if "lehmer" in op or op in ("fe_inv", "fn_inv_var") else None, " (layout %d)" % which)


@pytest.mark.parametrize("which", L.LAYOUTS)
def test_f_quad_inversions(probe, which):
    for op in L.QUAD_INV:
        got = L.quad_inv_input(op, which)
        if got is None:
            continue
        inp, vals, cls = got
        part = 4 * -(-L.PARTIAL // 4)
        for n in (len(inp) - part, len(inp)):
            out, flags = probe.run(op, inp, n)
            quads = L.check_quad_inv(op, vals, out)
            if op.endswith("divsteps"):  # no double-steered path in this op: nothing to read from the flag
                report(op, quads, None, " (layout %d)" % which)
                continue
            expect_fallback(which, wave_flags(flags))
            report(op, quads, int((flags[::4, 0] == 0).sum()), " (layout %d)" % which)


def test_g_shared_quad_inversion(probe):
    for log_distinct in (1, 2):
        inp, vals = L.shared_quad_input(log_distinct)
        for plain in (False, True):
            op = "inv_shared_quad_%d%s" % (log_distinct, "_plain" if plain else "")
            report(op, L.check_shared_quad(plain, vals, probe.run(op, inp)[0]))


def test_h_quad_additions(probe):
    for op in ("qadd", "qadd_x_only", "qmmadd"):
        inp, exp = L.quad_add_input(op)
        out, flags = probe.run(op, inp)
        quads, exceptional = L.check_quad_add(op, exp, out, flags)
        report(op, quads, extra=", %d exceptional (ZZ3 = 0 on every lane)" % exceptional)
