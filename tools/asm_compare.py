#!/usr/bin/env python3
"""Compare two directories of device assembly kernel by kernel (profiles/air_bodies_asm.txt).

    for f in stark builtins ...; do hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only -S csrc/$f.hip -o DIR/$f.s; done
    tools/asm_compare.py PARENT_DIR NEW_DIR

Per kernel: whether the instruction stream is identical once labels, comments and directives are dropped, and if not
the opcode counts that differ; and the registers, scratch and occupancy attribute of both builds.  Needs no GPU.

    ... -S -emit-llvm ... -o DIR/$f.ll ;  tools/asm_compare.py --ir PARENT_DIR NEW_DIR

The same question one level up, where the scheduler has not yet reordered anything: per kernel the counts of optimised
LLVM IR instructions, by opcode and type, that differ.  Field arithmetic is mul / and / ashr / lshr / trunc / sext and
i64 add; address arithmetic is getelementptr, shl i64 and the i64 add beside them."""
import collections
import os
import re
import sys

ATTRS = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size")


def kernels(path):
    """{kernel: (instruction lines, {attribute: value})} of one .s file."""
    out, occ = {}, {}
    for chunk in open(path).read().split("; -- Begin function ")[1:]:
        name = chunk.split()[0]
        if ".amdhsa_kernel " + name not in chunk:
            continue  # a device function, not a kernel
        code = chunk[chunk.index("\n" + name + ":"):chunk.index(".Lfunc_end")]
        body = []
        for line in code.splitlines()[2:]:
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", s))
        out[name] = (body, {a: int(re.search(re.escape(a) + r" (\d+)", chunk).group(1)) for a in ATTRS})
        occ[name] = re.search(r"; Occupancy: (\d+)", chunk).group(1)
    return out, occ


def ir_kernels(path):
    """{kernel: Counter of (opcode, type)} of one .ll file."""
    out = {}
    for m in re.finditer(r"^define [^\n]*amdgpu_kernel [^\n]*@(\w+)\([^\n]*\{\n(.*?)^\}", open(path).read(), re.S | re.M):
        c = collections.Counter()
        for line in m.group(2).splitlines():
            t = re.match(r"\s+(?:%[\w.]+ = )?(?:tail )?(\w+)((?: nuw| nsw| exact| disjoint| inbounds)*) ?(\S+)?", line)
            if t:
                c[(t.group(1), t.group(3) if t.group(1) not in ("call", "br", "ret", "store") else "")] += 1
        out[m.group(1)] = c
    return out


def main_ir(parent, new):
    for f in sorted(os.listdir(parent)):
        if not f.endswith(".ll"):
            continue
        kp, kn = ir_kernels(os.path.join(parent, f)), ir_kernels(os.path.join(new, f))
        print("== %s: %d kernels" % (f, len(kp)))
        for k in sorted(set(kp) & set(kn)):
            diff = ", ".join("%s %s %d->%d" % (o[0], o[1], kp[k][o], kn[k][o])
                             for o in sorted(set(kp[k]) | set(kn[k])) if kp[k][o] != kn[k][o])
            print("  %-48s %s" % (k, "IR counts differ: " + diff if diff else "same IR instruction counts"))
    return 0


def main():
    if sys.argv[1] == "--ir":
        return main_ir(sys.argv[2], sys.argv[3])
    parent, new = sys.argv[1], sys.argv[2]
    worse = 0
    for f in sorted(os.listdir(parent)):
        if not f.endswith(".s"):
            continue
        kp, op = kernels(os.path.join(parent, f))
        kn, on = kernels(os.path.join(new, f))
        print("== %s: %d kernels" % (f, len(kp)))
        if set(kp) != set(kn):
            print("  KERNEL SETS DIFFER: only parent %s, only new %s" % (sorted(set(kp) - set(kn)), sorted(set(kn) - set(kp))))
            worse += 1
        for k in sorted(set(kp) & set(kn)):
            (bp, ap), (bn, an) = kp[k], kn[k]
            regs = " ".join("%s %d->%d" % (a.replace(".amdhsa_", ""), ap[a], an[a]) for a in ATTRS)
            occ = "occupancy %s->%s" % (op.get(k, "?"), on.get(k, "?"))
            bad = any(an[a] > ap[a] for a in ATTRS if a != ".amdhsa_accum_offset") or op.get(k) != on.get(k)
            # AGPRs = next_free_vgpr - accum_offset
            bad = bad or max(0, an[ATTRS[0]] - an[ATTRS[1]]) > max(0, ap[ATTRS[0]] - ap[ATTRS[1]])
            worse += bad
            if bp == bn:
                print("  %-48s identical (%d instructions)%s" % (k, len(bp), "" if ap == an else "  " + regs))
                continue
            cp, cn = collections.Counter(l.split()[0] for l in bp), collections.Counter(l.split()[0] for l in bn)
            diff = ", ".join("%s %d->%d" % (o, cp[o], cn[o]) for o in sorted(set(cp) | set(cn)) if cp[o] != cn[o])
            print("  %-48s DIFFERS %d->%d instructions%s\n      %s; %s\n      opcodes: %s"
                  % (k, len(bp), len(bn), "  MORE REGISTERS/SCRATCH OR OTHER OCCUPANCY" if bad else "", regs, occ,
                     diff or "same counts, other order or operands"))
    print("kernels with more registers, more scratch or another occupancy than the parent: %d" % worse)
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
