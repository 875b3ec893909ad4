"""The reference side of tests/test_gpu_field_probe.py, verified without a GPU.

  1. Every lane-private op of the device probe's op table (tests/gpu/field_probe_ops.hpp) runs in its HOST twin - g++
     with SP_CHECK_BOUNDS, so a limb or column that leaves its budget on any of these inputs aborts the process - on
     the same inputs as the GPU run, and goes through the same checks (tests/field_probe_lib.py): limb packing,
     Montgomery factors, expected values and input generators of the Python model are right before the device is
     asked anything.
  2. Every generated wave has the composition it claims: the counts of R / S / Z / U lanes, every S value makes
     lehmer_bezout ask for the divsteps fallback on the host, and every R and U value converges there - so the flags
     the GPU test reads ("the whole wave fell back", "nobody fell back") do not rest on the code under test.
  3. The probe cross-compiles for gfx950 and lists the op shapes the twin has."""
import collections

import numpy as np
import pytest

import field_probe_lib as L


@pytest.fixture(scope="module")
def twin():
    return L.Twin()


def test_a_pack_unpack(twin):
    vals, arr = L.pack_words()
    assert len(vals) >= 512 + 5
    L.check_pack(vals, twin.run("pack_unpack", arr)[0], twin.run("unpack", arr)[0])


def test_b_multiplications(twin):
    for inp in (L.mul_tuples(), L.mul_random()):
        out, _ = twin.run("mul_forms", inp)
        L.check_mul(inp, out)
    assert len(L.mul_tuples()) == 46656 and len(L.mul_random()) == 8192


def test_c_small_ops(twin):
    for op, (inp, exp) in L.small_inputs().items():
        out, flags = twin.run(op, inp)
        L.check_small(op, inp, exp, out, flags)


@pytest.mark.parametrize("op", L.GROUP_OPS)
def test_d_group_law(twin, op):
    inp, exp = L.group_inputs(op)
    assert len(inp) % 64 != 0 and len(inp) > 128  # more than one wave, the last one partial
    out, flags = twin.run(op, inp)
    items, exceptional = L.check_group(op, exp, out, flags)
    assert exceptional == (0 if op.startswith("jac") else 32)


@pytest.mark.parametrize("family", sorted(L.INV_FAMILIES))
def test_e_inversions(twin, family):
    ops, bezout, m, kw = L.INV_FAMILIES[family]
    for which in L.LAYOUTS:
        got = L.inv_input(family, which)
        if got is None:
            continue
        inp, vals, cls = got
        for op in ops:
            L.check_inv(op, vals, twin.run(op, inp)[0])
        out, flags = twin.run(bezout, inp)
        L.check_bezout(bezout, vals, out, flags)
        # the twin runs one value at a time: flag 0 is the value's own answer.  S asks for the fallback; R, U and Z
        # converge - the seed of class R (field_probe_lib.SEED_R) is chosen so that this holds for every value.
        for c, ok in zip(cls, flags[:, 0]):
            assert ok == (0 if c == "S" else 1), (family, which, c)


def test_wave_composition():
    s, z = L.class_s(), L.class_z()
    assert set(range(1, 65)) <= set(s) and {L.P - 1, L.P - 2, (L.P + 1) // 2, (L.P - 1) // 2} <= set(s)
    assert {1 << k for i in range(9) for k in (29 * i - 1, 29 * i, 29 * i + 1) if 0 <= k < 251} <= set(s)
    assert any(v < 1 << 224 and v > 1 << 200 for v in s)
    assert len(z) == 31 and all(v % L.P == 0 for v in z)
    for group in (1, 4):
        per = 64 // group
        for which in L.LAYOUTS:
            vals, cls = L.layout(which, group=group)
            assert len(vals) == len(cls) and len(vals) % per == -(-L.PARTIAL // group) and len(vals) > per
            waves = [cls[i:i + per] for i in range(0, len(cls), per)]
            count = collections.Counter(cls)
            if which == 1:
                assert set(cls) == {"R"} and all(0 < v < L.P for v in vals)
            if which == 2:  # exactly one S lane in every wave, the partial one included; every S value is used
                assert all(w.count("S") == 1 and w.count("R") == len(w) - 1 for w in waves)
                assert {v for v, c in zip(vals, cls) if c == "S"} == set(s)
            if which == 3:
                assert set(cls) == {"S", "Z"} and {v for v, c in zip(vals, cls) if c == "Z"} == set(z)
                assert {v for v, c in zip(vals, cls) if c == "S"} == set(s)
                assert all("S" in w for w in waves)  # a wave of Z alone would converge
            if which == 4:
                assert set(cls) == {"U"}
                assert {v // L.P for v in vals} == {-2, -1, 0, 1, 2, 3} and all(v % L.P for v in vals)
            assert sum(count.values()) == len(vals)
    # the canonical-only forms: no layout 4, and Z is the single value 0
    vals, cls = L.layout(3, unreduced=False)
    assert [v for v, c in zip(vals, cls) if c == "Z"].count(0) >= 1 and all(0 <= v < L.P for v in vals)
    assert L.inv_input("plain", 4) is None and L.quad_inv_input("inv_plain_quad_divsteps", 4) is None
    # every quad input repeats its value on the four lanes
    inp, vals, cls = L.quad_inv_input("inv_plain_quad", 2)
    assert len(inp) == 4 * len(vals) and (inp.reshape(-1, 4, 9) == inp.reshape(-1, 4, 9)[:, :1]).all()


def test_quad_inputs_against_the_lane_private_twin(twin):
    """The quad ops cannot run on the host; their inputs and expectations can.  Quad inversions: the lane-private
    inversion of the same limbs gives the value the check expects, and S / R / U / Z fall back or converge as claimed.
    Quad additions: the serial xyzz_add / xyzz_mmadd of the same limbs gives the point the check expects."""
    for op in L.QUAD_INV:
        for which in L.LAYOUTS:
            got = L.quad_inv_input(op, which)
            if got is None:
                continue
            inp, vals, cls = got
            lane = inp[::4]
            plain, _ = twin.run("fe_inv_plain_lehmer", L.elems([[L.nform(v % L.P)] for v in vals]))
            fake = np.repeat(plain, 4, axis=0)
            if L.QUAD_INV[op][1] == "plain":
                L.check_quad_inv(op, vals, fake)
            _, flags = twin.run("lehmer_bezout", lane)
            assert flags[:, 0].tolist() == [0 if c == "S" else 1 for c in cls], (op, which)
    for op, serial in (("qadd", "xyzz_add"), ("qadd_x_only", "xyzz_add_x_only"), ("qmmadd", "xyzz_mmadd")):
        inp, exp = L.quad_add_input(op)
        assert len(inp) % 64 != 0 and len(inp) % 4 == 0 and len(inp) > 64
        q = inp.reshape(len(exp), 4, -1, 9)
        if op == "qmmadd":
            assert (q[:, 0] == q[:, 1]).all() and (q[:, 2] == q[:, 3]).all()
            for half in (0, 2):
                out, flags = twin.run(serial, q[:, half])
                L.check_group(serial, [e[half >> 1] for e in exp], out, flags)
        else:  # lanes 0,1: X | Y and ZZ | ZZZ of P1, lanes 2,3: of P2
            rec = np.stack([q[:, 0, 0], q[:, 1, 0], q[:, 0, 1], q[:, 1, 1], q[:, 2, 0], q[:, 3, 0], q[:, 2, 1], q[:, 3, 1]], axis=1)
            out, flags = twin.run(serial, rec)
            L.check_group(serial, [e[0] for e in exp], out, flags)
        assert len({tuple(r.reshape(-1)) for r in q[:, 0]}) == len(exp)  # a different pair in every quad
    for log_distinct in (1, 2):
        inp, vals = L.shared_quad_input(log_distinct)
        assert len(inp) == 4 * 41 and all(v % L.P for v in vals)
        quads = [vals[i:i + 4] for i in range(0, len(vals), 4)]
        assert all(len(set(q)) == 2 * log_distinct for q in quads)
        assert any(set(q) == {q[0], L.P - q[0], 1, L.P - 1} for q in quads) or log_distinct == 1
        out, _ = twin.run("fe_inv", inp)  # the lane-private inversion returns what the check expects of every lane
        L.check_shared_quad(False, vals, out)


def test_probe_cross_compiles_for_gfx950(twin, tmp_path):
    if L.hipcc() is None:
        pytest.skip("no hipcc on this box")
    import subprocess
    out = str(tmp_path / "field_probe")
    r = subprocess.run(L.probe_build_cmd(out), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    shapes = L.probe_shapes(out)
    lane = {op: s[:3] for op, s in shapes.items() if not s[3]}
    assert lane and all(twin.shape(op) == s for op, s in lane.items())
    quad = {op for op, s in shapes.items() if s[3]}
    assert quad == set(L.QUAD_INV) | {"inv_shared_quad_1", "inv_shared_quad_1_plain", "inv_shared_quad_2",
                                      "inv_shared_quad_2_plain", "qadd", "qadd_x_only", "qmmadd"}
    # a quad op refuses an n that would leave a quad with lanes off, before it touches the GPU
    np.zeros((6, 1, 9), dtype=np.int32).tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([out, "inv_quad", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "6"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "quad" in r.stderr
