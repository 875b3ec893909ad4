"""Python-int restatement of the builtins proof bound to its statement (sp_boundary_combine_dev,
sp_builtins_boundary_dev, sp_builtins_boundary_points_dev, stark.prove_builtin_usage / verify_builtin_usage;
DESIGN.md 6.6), built on oracle/stark_ref.py and tests/boundary_ref.py: the flat transcript list, B on the coset and
at a point, the composition of a bound proof and the verifier - the twin of S.verify_builtins_proof with the extra
alphas and the extra term.

The combined trace lays the present segments side by side; every segment brings the groups and terms of its
descriptor, columns relative to its first column, periods 512, 1024 and 8:
    B(x) = sum over segments s, groups d of s: ( sum_{t in d} a_t col_{c0_s + c_t}(x) - C_d(x g^-o_d) ) / (x^k_s - w_{p_s}^o_d)
which is the sum of boundary_ref's B per segment.  Test infrastructure, written for clarity at small sizes."""
from oracle import ref_py as R
from oracle import stark_ref as S

import boundary_ref as B

P = S.P
AIR = "builtins_io"
SEG_NAMES = ("pedersen", "ecdsa", "rc16")
# acc (column 1 of the segment) at row 8 i + 7, the last limb of value i, is the padded value i
RC16_IO = {"air": "rc16", "period": 8, "n_cols": 3, "rows": (7,), "terms": ((1, 0),)}
SEG_DESC = {"pedersen": B.DESCRIPTORS["pedersen_io"], "ecdsa": B.DESCRIPTORS["ecdsa_io"], "rc16": RC16_IO}


def layout(segments):
    """[(segment, descriptor, first column, first boundary alpha)] of the present segments, in trace order."""
    out, col, al = [], 0, 0
    for seg in SEG_NAMES:
        if seg in segments:
            out.append((seg, SEG_DESC[seg], col, al))
            col += SEG_DESC[seg]["n_cols"]
            al += len(SEG_DESC[seg]["terms"])
    return out


def n_boundary_alphas(segments):
    return sum(len(SEG_DESC[s]["terms"]) for s in segments)


def flat_public(segments, pub):
    """What the transcript absorbs as the statement."""
    flat = [len(segments)] + [SEG_NAMES.index(s) for s in segments]
    if "rc16" in segments:
        flat += [pub["rc_min"], pub["rc_max"], len(pub["rc_values"])] + list(pub["rc_values"])
    if "ecdsa" in segments:
        flat += [v for sig in pub["signatures"] for v in sig]
    if "pedersen" in segments:
        flat += [v for triple in pub["hashes"] for v in triple]
    return flat


def term_values(seg, pub, n):
    """The public list v_t of every term of a segment from a proof's public inputs."""
    if seg == "pedersen":
        return [[t[c] for t in pub["hashes"]] for c in range(3)]
    if seg == "ecdsa":
        return B.term_values("ecdsa_io", [v for sig in pub["signatures"] for v in sig])
    return [S.rc16_fill(list(pub["rc_values"]), n // 8)[0]]


def boundary_on_coset(segments, trace_lde, values, n, alphas, shift=S.GEN, pub_lde=None):
    """B at every LDE index: trace_lde the columns of the present segments, values / pub_lde: segment -> term lists /
    the groups' columns C_d at x_j g^-o_d (made from the values when absent), alphas the boundary challenges."""
    out = [0] * (4 * n)
    for seg, desc, c0, a0 in layout(segments):
        al = alphas[a0: a0 + len(desc["terms"])]
        cols = trace_lde[c0: c0 + desc["n_cols"]]
        pl = pub_lde[seg] if pub_lde is not None else B.public_columns_lde(desc, values[seg], n, al, shift)
        out = [(a + b) % P for a, b in zip(out, B.boundary_on_coset(desc, cols, pl, n, al, shift))]
    return out


def coefficients(segments, values, n, alphas):
    """segment -> per group the coefficients of C_d."""
    return {seg: B.public_coefficients(desc, values[seg], n, alphas[a0: a0 + len(desc["terms"])])
            for seg, desc, _, a0 in layout(segments)}


def flat_coefficients(segments, coeffs):
    """The groups' coefficient arrays back to back, as the points call takes them."""
    return [c for seg, *_ in layout(segments) for group in coeffs[seg] for c in group]


def boundary_at(segments, n, coeffs, alphas, shift, pos, cur):
    """B at LDE index pos from the whole opened phase-1 row."""
    return sum(B.boundary_at(desc, n, coeffs[seg], alphas[a0: a0 + len(desc["terms"])], shift, pos,
                             cur[c0: c0 + desc["n_cols"]]) for seg, desc, c0, a0 in layout(segments)) % P


def composition_bound_on_coset(segments, trace_lde, p_lde, values, n, alphas, z, rc_min, rc_max, shift=S.GEN):
    """The composition of a bound proof: the segments' own compositions (alphas: the AIRs' first) plus B."""
    out = [0] * (4 * n)
    for air, c0, nc, a0, na in S.builtin_layout(list(segments)):
        al = alphas[a0: a0 + na]
        part = (S.rc16_composition_on_coset(trace_lde[c0: c0 + nc], p_lde, n, al, z, rc_min, rc_max, shift) if air == "rc16"
                else S.composition_on_coset(trace_lde[c0: c0 + nc], S.periodic_lde(n, shift, air), n, al, shift, air))
        out = [(a + b) % P for a, b in zip(out, part)]
    n_air = sum(na for *_, na in S.builtin_layout(list(segments)))
    extra = boundary_on_coset(segments, trace_lde, values, n, alphas[n_air:], shift)
    return [(a + b) % P for a, b in zip(out, extra)]


def public_inputs_ok(segments, pub, n):
    """The statement rules beyond S.verify_builtins_proof's own."""
    if "pedersen" in segments:
        if len(pub["hashes"]) != n // 512 or not all(0 <= v < P for t in pub["hashes"] for v in t):
            return False
    if "rc16" in segments:
        values = list(pub["rc_values"])
        if not values or not all(0 <= v < 1 << 128 for v in values):
            return False
        limbs = {(v >> (16 * k)) & 0xFFFF for v in values for k in range(8)}
        holes = max(limbs) - min(limbs) + 1 - len(limbs)
        if len(values) + -(-holes // 8) > n // 8:
            return False
        if (min(limbs), max(limbs)) != (pub["rc_min"], pub["rc_max"]):
            return False
    return True


def verify_builtins_proof_bound(proof, hash2=R.pedersen_hash, final_log=6):
    """S.verify_builtins_proof for air == "builtins_io": the same checks, order and reasons, with the statement's
    rules, its transcript list, the extra alphas and B added to the expected composition value."""
    if proof.get("air") != AIR:
        return False, "malformed"
    n, seed, shift = proof["n"], proof["seed"], proof["shift"]
    segments = proof["segments"]
    lay = S.builtin_layout(segments)
    if [s for s, *_ in lay] != list(segments) or not lay:
        return False, "segments"
    n_cols = sum(c for _, _, c, _, _ in lay)
    n_alphas = sum(a for *_, a in lay)
    has_rc = "rc16" in segments
    pub = proof["public_inputs"]
    rc_min = rc_max = 0
    if has_rc:
        rc_min, rc_max = pub["rc_min"], pub["rc_max"]
        if not (0 <= rc_min <= rc_max < 1 << S.RC16_BITS) or n % 8:
            return False, "public inputs"
    if "ecdsa" in segments:
        sigs = pub["signatures"]
        if n % 1024 or len(sigs) != n // 1024:
            return False, "public inputs"
        for z_, r_, s_, qx, qy in sigs:
            if not (1 <= s_ < R.EC_ORDER and 1 <= r_ < 2**251 and 0 < z_ < 2**251 and R.is_point_on_curve(qx, qy)):
                return False, "public inputs"
            if not 1 <= R.inv_mod_curve_size(s_) < 2**251:
                return False, "public inputs"
    if "pedersen" in segments and n % 512:
        return False, "public inputs"
    if not public_inputs_ok(segments, pub, n):
        return False, "public inputs"
    m = S.BLOWUP * n
    log_m = m.bit_length() - 1
    n_layers = log_m - final_log
    roots, final = proof["layer_roots"], proof["final_layer"]
    if len(roots) != n_layers or len(final) != 1 << final_log:
        return False, "shape"
    tr = S.Transcript(AIR, n, shift, seed, flat_public(segments, pub))
    tr.absorb("phase1_root", proof["phase1_root"])
    z = tr.challenge("rc16_z") if has_rc else 0
    if has_rc:
        tr.absorb("phase2_root", proof["phase2_root"])
    alphas = [tr.challenge("alpha", k) for k in range(n_alphas + n_boundary_alphas(segments))]
    betas = []
    for k in range(n_layers):
        tr.absorb("layer_root", roots[k])
        betas.append(tr.challenge("beta", k + 1))
    tr.absorb("final_layer", *final)
    w = S.root_of_unity(log_m)
    g_last = pow(S.root_of_unity(n.bit_length() - 1), n - 1, P)
    zinv = [pow((pow(shift, n, P) * pow(w, n * k, P) - 1) % P, -1, P) for k in range(S.BLOWUP)]
    pers = {}
    for air, *_ in lay:
        pers[air] = ([S.lde(c, S.BLOWUP, pow(shift, n // 8, P)) for c in S.rc16_periodic_columns()] if air == "rc16"
                     else B._periodic_lde(n, shift, air))
    fshift = shift
    for _ in range(n_layers):
        fshift = fshift * fshift % P
    if not S.poly_degree_bound_check(final, fshift, (3 * n >> n_layers) - 1):
        return False, "final layer degree"
    coeffs = None
    for qi, q in enumerate(proof["queries"]):
        j = tr.challenge("query", qi, modulus=m // 2)
        if q["index"] != j:
            return False, "query index"
        want_rows = [j, (j + S.BLOWUP) % m, j + m // 2, (j + m // 2 + S.BLOWUP) % m]
        if [t["row"] for t in q["phase1"]] != want_rows or (has_rc and [t["row"] for t in q["phase2"]] != want_rows):
            return False, "opened rows"
        for t in q["phase1"]:
            if len(t["values"]) != n_cols:
                return False, "opened rows"
            leaf = t["values"][0]
            for v in t["values"][1:]:
                leaf = hash2(leaf, v)
            if S._root_from_path(leaf, t["row"], t["path"], hash2) != proof["phase1_root"]:
                return False, "phase 1 path"
        if has_rc:
            for t in q["phase2"]:
                if S._root_from_path(t["value"], t["row"], t["path"], hash2) != proof["phase2_root"]:
                    return False, "phase 2 path"
        if coeffs is None:
            coeffs = coefficients(segments, {s: term_values(s, pub, n) for s in segments}, n, alphas[n_alphas:])
        for side, pos in enumerate((j, j + m // 2)):
            cur, nxt = q["phase1"][2 * side]["values"], q["phase1"][2 * side + 1]["values"]
            x = shift * pow(w, pos, P) % P
            expect = boundary_at(segments, n, coeffs, alphas[n_alphas:], shift, pos, cur)
            for air, c0, nc, a0, na in lay:
                al = alphas[a0: a0 + na]
                if air == "rc16":
                    pv = [tab[pos % 32] for tab in pers[air]]
                    cv = S.rc16_constraint_values(cur[c0: c0 + nc], nxt[c0: c0 + nc], pv, q["phase2"][2 * side]["value"],
                                                  q["phase2"][2 * side + 1]["value"], z, rc_min, rc_max)
                    expect += S.rc16_composition_value(al, cv, x, zinv[pos % S.BLOWUP], g_last)
                else:
                    spec = S.AIRS[air]
                    pv = [tab[pos % (S.BLOWUP * spec["period"])] for tab in pers[air]]
                    cv = spec["constraints"](cur[c0: c0 + nc], nxt[c0: c0 + nc], pv)
                    expect += sum(a * c for a, c in zip(al, cv)) % P * zinv[pos % S.BLOWUP]
            if q["layers"][0][side]["value"] != expect % P:
                return False, "composition value"
        jk, s, mk = j, shift, m
        for k in range(n_layers):
            jk %= mk // 2
            a, b = q["layers"][k]
            if (a["pos"], b["pos"]) != (jk, jk + mk // 2):
                return False, "layer positions"
            for o in (a, b):
                if S._root_from_path(o["value"], o["pos"], o["path"], hash2) != roots[k]:
                    return False, "layer path"
            wk = S.root_of_unity(mk.bit_length() - 1)
            xk = s * pow(wk, jk, P) % P
            folded = ((a["value"] + b["value"]) * pow(2, -1, P)
                      + betas[k] * (a["value"] - b["value"]) % P * pow(2 * xk, -1, P)) % P
            if k + 1 < n_layers:
                nxt_pair = q["layers"][k + 1]
                nxt_val = nxt_pair[0]["value"] if jk < mk // 4 else nxt_pair[1]["value"]
            else:
                nxt_val = final[jk]
            if folded != nxt_val:
                return False, "fold consistency at layer %d" % k
            s = s * s % P
            mk //= 2
    return True, "ok"
