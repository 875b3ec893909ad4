"""Python-int restatement of the statement-binding Pedersen proof (stark.prove_hashes / verify_hashes),
built on oracle/stark_ref.py: the public columns on the LDE coset, the three boundary quotients, the composition they
join and the verifier - the twin of S.verify_proof with the 14-alpha transcript and the extra term.

n = 512 k rows, g = w_n, omega = g^512 of order k; X, Y, H are the polynomials of degree < k with X(omega^i) = x_i,
Y(omega^i) = y_i, H(omega^i) = h_i for public_inputs = [x_0, y_0, h_0, x_1, ...]:
    B(x) = a11 (s(x) - X(x)) / (x^k - 1) + a12 (s(x) - Y(x g^-256)) / (x^k + 1) + a13 (px(x) - H(x g^-511)) / (x^k - g^-k)
Test infrastructure, written for clarity at small sizes."""
from oracle import ref_py as R
from oracle import stark_ref as S

P = S.P
AIR = "pedersen_io"
N_ALPHAS = S.N_CONSTRAINTS + 3
ROWS = (0, 256, 511)  # where x_i, y_i, h_i stand in a hash's 512 rows (columns s, s, px)


def hash_outputs(trace):
    """h_i as the trace holds it: px at row 512 i + 511 (the accumulator is held through the padding rows)."""
    return [trace[1][r] for r in range(511, len(trace[1]), 512)]


def public_inputs(inputs, outs=None):
    outs = outs if outs is not None else [R.pedersen_hash(x, y) for x, y in inputs]
    return [v for (x, y), h in zip(inputs, outs) for v in (x, y, h)]


def public_columns_lde(pub, n, shift=S.GEN):
    """X, Y, H at x_j, x_j g^-256, x_j g^-511 for every j < 4 n: k values extended 2048-fold with the shifted shift."""
    g = S.root_of_unity(n.bit_length() - 1)
    return [S.lde(pub[c::3], 2048, shift * pow(g, -r, P) % P) for c, r in enumerate(ROWS)]


def boundary_denominators(n, shift=S.GEN):
    """The three denominators at x^k = shift^k w_2048^t, t < 2048 - all the values they take on the coset."""
    k = n // 512
    g = S.root_of_unity(n.bit_length() - 1)
    w = S.root_of_unity(11)
    gk_inv = pow(g, -k, P)
    xk, out = pow(shift, k, P), []
    for _ in range(2048):
        out.append(((xk - 1) % P, (xk + 1) % P, (xk - gk_inv) % P))
        xk = xk * w % P
    return out


def boundary_on_coset(trace_lde, pub_lde, n, alphas, shift=S.GEN):
    """B at every LDE index; alphas = the three boundary challenges."""
    inv = [[pow(d, -1, P) for d in den] for den in boundary_denominators(n, shift)]
    s, px = trace_lde[0], trace_lde[1]
    X, Y, H = pub_lde
    return [(alphas[0] * (s[j] - X[j]) * inv[j % 2048][0] + alphas[1] * (s[j] - Y[j]) * inv[j % 2048][1]
             + alphas[2] * (px[j] - H[j]) * inv[j % 2048][2]) % P for j in range(4 * n)]


def composition_io_on_coset(trace_lde, per_lde, pub_lde, n, alphas, shift=S.GEN):
    """comp_pedersen + B; alphas = all 14."""
    base = S.composition_on_coset(trace_lde, per_lde, n, alphas[:S.N_CONSTRAINTS], shift, "pedersen")
    extra = boundary_on_coset(trace_lde, pub_lde, n, alphas[S.N_CONSTRAINTS:], shift)
    return [(a + b) % P for a, b in zip(base, extra)]


def public_coefficients(pub, n):
    k = n // 512
    return [S.intt(pub[c::3], S.root_of_unity(k.bit_length() - 1)) for c in range(3)]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def boundary_at(n, coeffs, alphas, shift, pos, cur):
    """B at LDE index pos from the opened row `cur` and the public polynomials' coefficients."""
    k = n // 512
    g = S.root_of_unity(n.bit_length() - 1)
    x = shift * pow(S.root_of_unity(n.bit_length() + 1), pos, P) % P
    xk = pow(x, k, P)
    dens = ((xk - 1) % P, (xk + 1) % P, (xk - pow(g, -k, P)) % P)
    vals = [horner(coeffs[c], x * pow(g, -r, P) % P) for c, r in enumerate(ROWS)]
    nums = (cur[0] - vals[0], cur[0] - vals[1], cur[1] - vals[2])
    return sum(a * u * pow(d, -1, P) for a, u, d in zip(alphas, nums, dens)) % P


def verify_proof_io(proof, hash2=R.pedersen_hash, final_log=6):
    """S.verify_proof for air "pedersen_io": the same checks, order and reasons, with 14 alphas and B added to the
    expected composition value.  Returns (ok, reason)."""
    n, seed, shift = proof["n"], proof["seed"], proof["shift"]
    if proof.get("air") != AIR:
        return False, "malformed"
    spec = S.AIRS["pedersen"]
    pub = proof.get("public_inputs", [])
    if len(pub) != 3 * (n // 512) or not all(type(v) is int and 0 <= v < P for v in pub):
        return False, "public inputs"
    m = S.BLOWUP * n
    log_m = m.bit_length() - 1
    root_t, roots, final = proof["trace_root"], proof["layer_roots"], proof["final_layer"]
    n_layers = log_m - final_log
    if len(roots) != n_layers or len(final) != 1 << final_log:
        return False, "shape"
    tr = S.Transcript(AIR, n, shift, seed, pub)
    tr.absorb("trace_root", root_t)
    alphas = [tr.challenge("alpha", k) for k in range(N_ALPHAS)]
    betas = []
    for k in range(n_layers):
        tr.absorb("layer_root", roots[k])
        betas.append(tr.challenge("beta", k + 1))
    tr.absorb("final_layer", *final)
    per = S.periodic_lde(n, shift, "pedersen")
    coeffs = public_coefficients(pub, n)
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
            expect = (expect + boundary_at(n, coeffs, alphas[S.N_CONSTRAINTS:], shift, pos, cur)) % P
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
