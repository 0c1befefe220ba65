"""Big-int model of the two-element multiproof (kzg_multiopen_* in kzg_amd/csrc/capi.hip, multiopen.hip, multiopen_plan.h) and of its
verifier (kzg_verify_multiopen, kzg_amd/csrc/verify_eval_batch.hip).  N claims k: polynomial m(k), point z_k, value y_k = p_{m(k)}(z_k);
challenges r and t:
    g = sum_k r^k (p_{m(k)} - y_k)/(X - z_k) = sum_u (F_u - Y_u)/(X - z_u),  F_u = sum_{k in u} r^k p_{m(k)},  Y_u = sum_{k in u} r^k y_k
    D = [g(tau)]    w_k = r^k/(t - z_k)    W_m = sum_{m(k) = m} w_k    v = sum_m W_m p_m - g    g2 = sum_k w_k y_k = v(t)
    pi = [(v - v(t))/(X - t)]    E = sum_m W_m C_m    ok = [ e(pi, hs[1]) e(-(t pi + E - D - [g2] gs[0]), hs[0]) == 1 ].
Points are carried as their discrete logs where tau is known (verdict); the scalars need no tau.  Polynomials are coefficient lists or,
for the *_eval functions, lists of values on the size-d domain of compute_omega."""
from oracle import kzg_model as M
from tests import open_eval_model as OE

R = M.R
MONT = M.FR_MONT_R


def poly_eval(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def div_linear(coeffs, z):
    """the n - 1 coefficients of (p - p(z))/(X - z)"""
    q, acc = [0] * (len(coeffs) - 1), 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (acc * z + coeffs[i]) % R
        q[i - 1] = acc
    return q


def lincomb(vecs, idx, weights, carry=None):
    """out[j] (+ carry[j]) = sum_k weights[k] vecs[idx[k]][j]; any integers count as residues (k_fr_lincomb)"""
    d = len(vecs[0]) if vecs else len(carry)
    out = [c % R for c in carry] if carry is not None else [0] * d
    for m, wt in zip(idx, weights):
        out = [(o + wt * x) % R for o, x in zip(out, vecs[m])]
    return out


def plan(zs, cap=None, on=None):
    """(order, pstart, points, chunks): the claims sorted by point -- by the Montgomery representation, the order of multiopen_plan.h;
    claims of one point keep their order -- the claim ranges of the distinct points, and the points cut into chunks of at most cap.
    on(z) true: the point goes behind the others (the evaluation-form driver's points of the domain) and is no part of a chunk."""
    order = sorted(range(len(zs)), key=lambda k: zs[k] % R * MONT % R)
    points, pstart = [], []
    for s, k in enumerate(order):
        if s == 0 or zs[k] % R != zs[order[s - 1]] % R:
            points.append(zs[k] % R)
            pstart.append(s)
    pstart.append(len(zs))
    if on is not None:
        parts = [[u for u in range(len(points)) if bool(on(points[u])) == flag] for flag in (False, True)]
        src = parts[0] + parts[1]
        order2, pstart2 = [], []
        for u in src:
            pstart2.append(len(order2))
            order2 += order[pstart[u]:pstart[u + 1]]
        pstart2.append(len(order2))
        order, pstart, points, n_off = order2, pstart2, [points[u] for u in src], len(parts[0])
    else:
        n_off = len(points)
    cap = cap or max(n_off, 1)
    chunks = [(u0, min(u0 + cap, n_off)) for u0 in range(0, n_off, cap)]
    return order, pstart, points, chunks


def weights(zs, r, t, first=0, count=None):
    """w_k = r^k/(t - z_k) for k = first .. first + count - 1 (a chunk continues the call's powers of r)"""
    count = len(zs) - first if count is None else count
    return [pow(r, k, R) * M.fr_inv((t - zs[k]) % R) % R for k in range(first, first + count)]


def poly_weights(zs, idx, n_polys, r, t, chunk=None):
    """(w, W): W_m = sum_{m(k) = m} w_k; with `chunk` the claims are worked in chunks of that many, as the library does"""
    idx = list(range(len(zs))) if idx is None else idx
    chunk = chunk or max(len(zs), 1)
    w, W = [], [0] * n_polys
    for k0 in range(0, len(zs), chunk):
        part = weights(zs, r, t, k0, min(chunk, len(zs) - k0))
        for k, x in zip(range(k0, k0 + len(part)), part):
            W[idx[k]] = (W[idx[k]] + x) % R
        w += part
    return w, W


# ---- coefficient form -------------------------------------------------------------------------------------------------------------
def commit_coeff(polys, idx, zs, r):
    """(ys, g): the per-claim sum"""
    idx = list(range(len(zs))) if idx is None else idx
    n = len(polys[0])
    ys, g = [], [0] * (n - 1)
    for k, (m, z) in enumerate(zip(idx, zs)):
        ys.append(poly_eval(polys[m], z))
        rk = pow(r, k, R)
        g = [(a + rk * b) % R for a, b in zip(g, div_linear(polys[m], z))]
    return ys, g


def commit_coeff_regrouped(polys, idx, zs, r, cap=None):
    """g by distinct points: sum_u (F_u - Y_u)/(X - z_u), chunk by chunk"""
    idx = list(range(len(zs))) if idx is None else idx
    order, pstart, points, chunks = plan(zs, cap)
    n = len(polys[0])
    g = [0] * (n - 1)
    for u0, u1 in chunks:
        for u in range(u0, u1):
            ks = order[pstart[u]:pstart[u + 1]]
            F = lincomb(polys, [idx[k] for k in ks], [pow(r, k, R) for k in ks])
            Y = sum(pow(r, k, R) * poly_eval(polys[idx[k]], points[u]) for k in ks) % R
            assert poly_eval(F, points[u]) == Y
            g = [(a + b) % R for a, b in zip(g, div_linear(F, points[u]))]
    return g


def finish_coeff(polys, idx, zs, r, t, g):
    """(v(t), the n - 1 coefficients of (v - v(t))/(X - t))"""
    w, W = poly_weights(zs, idx, len(polys), r, t)
    v = lincomb(polys, range(len(polys)), W)
    v = [(a - b) % R for a, b in zip(v, list(g) + [0])]
    return poly_eval(v, t), div_linear(v, t)


# ---- evaluation form ----------------------------------------------------------------------------------------------------------------
def commit_eval(evals, idx, zs, r):
    """(ys, g on the domain): per claim the quotient of kzg_open_eval, weighted by r^k"""
    idx = list(range(len(zs))) if idx is None else idx
    d = len(evals[0])
    ys, g = [], [0] * d
    for k, (m, z) in enumerate(zip(idx, zs)):
        y, q = OE.quotient_at([f % R for f in evals[m]], z)
        ys.append(y)
        rk = pow(r, k, R)
        g = [(a + rk * b) % R for a, b in zip(g, q)]
    return ys, g


def finish_eval(evals, idx, zs, r, t, g):
    """(v, v(t), the values of (v - v(t))/(X - t) on the domain)"""
    w, W = poly_weights(zs, idx, len(evals), r, t)
    v = lincomb(evals, range(len(evals)), W, carry=[(R - x) % R for x in g])
    y, q = OE.quotient_at(v, t)
    return v, y, q


def interpolate(evals):
    """the coefficients of the polynomial with these values on the domain"""
    d = len(evals)
    w = M.compute_omega(d)[2]
    wi, di = M.fr_inv(w), M.fr_inv(d % R)
    return [sum(f * pow(wi, i * j, R) for j, f in enumerate(evals)) % R * di % R for i in range(d)]


# ---- the proof and its verifier, points as discrete logs -------------------------------------------------------------------------------
def prove(polys, idx, zs, r, t, tau):
    """(ys, D, pi) of the honest prover for coefficient lists; tau != t"""
    ys, g = commit_coeff(polys, idx, zs, r)
    vt, q = finish_coeff(polys, idx, zs, r, t, g)
    return ys, poly_eval(g, tau), poly_eval(q, tau)


def verdict(tau, commitments, idx, zs, ys, r, t, D, pi, chunk=None):
    """the pairing equation with known tau: commitments[m] = p_m(tau), D = g(tau), pi = q(tau) as scalars"""
    w, W = poly_weights(zs, idx, len(commitments), r, t, chunk)
    E = sum(a * b for a, b in zip(W, commitments)) % R
    g2 = sum(a * b for a, b in zip(w, ys)) % R
    return pi * tau % R == (t * pi + E - D - g2) % R


def forge(C, z, y_wrong, t):
    """(D, pi) that pass for the ONE wrong claim (C, z, y') when t was known before D was chosen; r^0 = 1; no tau needed: as scalars
    this is a linear map of C and gs[0], i.e. group operations on public points"""
    return (C - y_wrong) * M.fr_inv((t - z) % R) % R, 0
