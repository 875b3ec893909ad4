"""Python-int restatement of boundary constraints from a descriptor (sp_boundary_dev / sp_boundary_points_dev,
stark.prove_signatures / verify_signatures, prove_ranges / verify_ranges), built on
oracle/stark_ref.py: the combined public columns on the LDE coset, the boundary quotients, the composition they join
and the verifier - the twin of S.verify_proof with the extra alphas and the extra term.

An AIR of period p, n = p k rows, g = w_n, omega = g^p of order k.  A descriptor names boundary groups (a row o_d < p
each) and terms (column c_t, group): "column c_t at row p i + o_d is v_t[i]".  With one challenge a_t per term and C_d
the polynomial of degree < k through sum_{t in d} a_t v_t[i] at omega^i,
    B(x) = sum_d ( sum_{t in d} a_t col_{c_t}(x) - C_d(x g^-o_d) ) / (x^k - w_p^o_d).
Test infrastructure, written for clarity at small sizes."""
import functools

from oracle import ref_py as R
from oracle import stark_ref as S

P = S.P

# name -> base AIR, period, columns of a row, the groups' rows, the terms as (column, group)
DESCRIPTORS = {
    "ecdsa_io": {"air": "ecdsa", "period": 1024, "n_cols": 10, "rows": (0, 256, 512),
                 "terms": ((0, 0), (0, 1), (3, 1), (4, 1), (0, 2))},  # m = z | m = r, qx = Qx, qy = Qy | m = w
    "range_check_io": {"air": "range_check", "period": 128, "n_cols": 1, "rows": (0,), "terms": ((0, 0),)},
    "pedersen_io": {"air": "pedersen", "period": 512, "n_cols": 4, "rows": (0, 256, 511),
                    "terms": ((0, 0), (0, 1), (1, 2))},  # s = x | s = y | px = h: the statement of tests/hash_io_ref.py
}


def n_alphas(name):
    d = DESCRIPTORS[name]
    return S.AIRS[d["air"]]["n_constraints"] + len(d["terms"])


def term_values(name, pub):
    """The public list v_t of every term from a proof's public inputs."""
    if name == "ecdsa_io":  # [z, r, s, Qx, Qy] per signature; the third ladder's scalar is w = s^-1 mod N
        ws = [R.inv_mod_curve_size(s) for s in pub[2::5]]
        return [pub[0::5], pub[1::5], pub[3::5], pub[4::5], ws]
    if name == "range_check_io":
        return [list(pub)]
    return [pub[0::3], pub[1::3], pub[2::3]]


def combined_values(desc, values, alphas):
    """Per group the k values sum_{t in d} a_t v_t[i]."""
    k = len(values[0])
    out = [[0] * k for _ in desc["rows"]]
    for (_, d), v, a in zip(desc["terms"], values, alphas):
        out[d] = [(acc + a * x) % P for acc, x in zip(out[d], v)]
    return out


def public_columns_lde(desc, values, n, alphas, shift=S.GEN):
    """C_d at x_j g^-o_d for every j < 4 n: k combined values extended 4p-fold with the shifted shift."""
    g = S.root_of_unity(n.bit_length() - 1)
    return [S.lde(col, 4 * desc["period"], shift * pow(g, -o, P) % P)
            for col, o in zip(combined_values(desc, values, alphas), desc["rows"])]


def boundary_denominators(desc, n, shift=S.GEN):
    """Per group the denominator at x^k = shift^k w_4p^t, t < 4p - all the values it takes on the coset."""
    p = desc["period"]
    k = n // p
    wp, w = S.root_of_unity(p.bit_length() - 1), S.root_of_unity(p.bit_length() + 1)
    xk, out = pow(shift, k, P), []
    for _ in range(4 * p):
        out.append([(xk - pow(wp, o, P)) % P for o in desc["rows"]])
        xk = xk * w % P
    return out


def boundary_on_coset(desc, trace_lde, pub_lde, n, alphas, shift=S.GEN):
    """B at every LDE index; alphas = the boundary challenges in term order."""
    period = 4 * desc["period"]
    inv = [[pow(d, -1, P) for d in den] for den in boundary_denominators(desc, n, shift)]
    out = []
    for j in range(4 * n):
        num = [-col[j] for col in pub_lde]
        for (c, d), a in zip(desc["terms"], alphas):
            num[d] += a * trace_lde[c][j]
        out.append(sum(u * i for u, i in zip(num, inv[j % period])) % P)
    return out


def public_coefficients(desc, values, n, alphas):
    k = n // desc["period"]
    return [S.intt(col, S.root_of_unity(k.bit_length() - 1)) for col in combined_values(desc, values, alphas)]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def boundary_at(desc, n, coeffs, alphas, shift, pos, cur):
    """B at LDE index pos from the opened row `cur` and the coefficients of the C_d."""
    p = desc["period"]
    k = n // p
    g, wp = S.root_of_unity(n.bit_length() - 1), S.root_of_unity(p.bit_length() - 1)
    x = shift * pow(S.root_of_unity(n.bit_length() + 1), pos, P) % P
    xk = pow(x, k, P)
    num = [-horner(coeffs[d], x * pow(g, -o, P) % P) for d, o in enumerate(desc["rows"])]
    for (c, d), a in zip(desc["terms"], alphas):
        num[d] += a * cur[c]
    return sum(u * pow((xk - pow(wp, o, P)) % P, -1, P) for u, o in zip(num, desc["rows"])) % P


def composition_bound_on_coset(name, trace_lde, per_lde, values, n, alphas, shift=S.GEN):
    """The AIR's composition + B; alphas = all of them, the AIR's own first."""
    desc = DESCRIPTORS[name]
    nc = S.AIRS[desc["air"]]["n_constraints"]
    base = S.composition_on_coset(trace_lde, per_lde, n, alphas[:nc], shift, desc["air"])
    extra = boundary_on_coset(desc, trace_lde, public_columns_lde(desc, values, n, alphas[nc:], shift), n, alphas[nc:],
                              shift)
    return [(a + b) % P for a, b in zip(base, extra)]


@functools.lru_cache(maxsize=8)
def _periodic_lde(n, shift, air):
    """S.periodic_lde, kept: a test verifies many edited copies of one proof."""
    return S.periodic_lde(n, shift, air)


def verify_proof_bound(proof, hash2=R.pedersen_hash, final_log=6):
    """S.verify_proof for the airs of DESCRIPTORS: the same checks, order and reasons, with the extra alphas and B
    added to the expected composition value.  Returns (ok, reason)."""
    name = proof.get("air")
    if name not in ("ecdsa_io", "range_check_io"):
        return False, "malformed"
    desc = DESCRIPTORS[name]
    n, seed, shift = proof["n"], proof["seed"], proof["shift"]
    spec = S.AIRS[desc["air"]]
    pub = proof.get("public_inputs", [])
    if desc["air"] == "ecdsa":
        if len(pub) != 5 * (n // 1024):
            return False, "public inputs"
        for k in range(n // 1024):
            z, r, sig_s, qx, qy = pub[5 * k: 5 * k + 5]
            if not (1 <= sig_s < R.EC_ORDER and 1 <= r < 2**251 and 0 < z < 2**251 and R.is_point_on_curve(qx, qy)):
                return False, "public inputs"
            if not 1 <= R.inv_mod_curve_size(sig_s) < 2**251:
                return False, "public inputs"
    else:
        if len(pub) != n // S.RANGE_CHECK_BITS or not all(0 <= v < 2**S.RANGE_CHECK_BITS for v in pub):
            return False, "public inputs"
    m = S.BLOWUP * n
    log_m = m.bit_length() - 1
    root_t, roots, final = proof["trace_root"], proof["layer_roots"], proof["final_layer"]
    n_layers = log_m - final_log
    if len(roots) != n_layers or len(final) != 1 << final_log:
        return False, "shape"
    tr = S.Transcript(name, n, shift, seed, pub)
    tr.absorb("trace_root", root_t)
    alphas = [tr.challenge("alpha", k) for k in range(n_alphas(name))]
    betas = []
    for k in range(n_layers):
        tr.absorb("layer_root", roots[k])
        betas.append(tr.challenge("beta", k + 1))
    tr.absorb("final_layer", *final)
    per = _periodic_lde(n, shift, desc["air"])
    nc = spec["n_constraints"]
    coeffs = public_coefficients(desc, term_values(name, pub), n, alphas[nc:])
    w = S.root_of_unity(log_m)
    zinv = [pow((pow(shift, n, P) * pow(w, n * k, P) - 1) % P, -1, P) for k in range(S.BLOWUP)]
    fshift = shift
    for _ in range(n_layers):
        fshift = fshift * fshift % P
    if not S.poly_degree_bound_check(final, fshift, (3 * n >> n_layers) - 1):
        return False, "final layer degree"
    for qi, q in enumerate(proof["queries"]):
        j = tr.challenge("query", qi, modulus=m // 2)
        if q["index"] != j:
            return False, "query index"
        want_rows = [j, (j + S.BLOWUP) % m, j + m // 2, (j + m // 2 + S.BLOWUP) % m]
        if [t["row"] for t in q["trace"]] != want_rows:
            return False, "trace rows"
        for t in q["trace"]:
            leaf = t["values"][0]
            for v in t["values"][1:]:
                leaf = hash2(leaf, v)
            if S._root_from_path(leaf, t["row"], t["path"], hash2) != root_t:
                return False, "trace path"
        for side, pos in enumerate((j, j + m // 2)):
            cur, nxt = q["trace"][2 * side]["values"], q["trace"][2 * side + 1]["values"]
            pv = [tab[pos % (S.BLOWUP * spec["period"])] for tab in per]
            cv = spec["constraints"](cur, nxt, pv)
            expect = sum(a * c for a, c in zip(alphas, cv)) % P * zinv[pos % S.BLOWUP] % P
            expect = (expect + boundary_at(desc, n, coeffs, alphas[nc:], shift, pos, cur)) % P
            if q["layers"][0][side]["value"] != expect:
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
            x = s * pow(wk, jk, P) % P
            folded = ((a["value"] + b["value"]) * pow(2, -1, P)
                      + betas[k] * (a["value"] - b["value"]) % P * pow(2 * x, -1, P)) % P
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
