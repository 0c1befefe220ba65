"""Big-int model of the folded opening (kzg_fr_fold, kzg_open_fold_eval / kzg_open_fold_coeff in kzg_amd/csrc/capi.hip and fold.hip)
and of its verifier (kzg_verify_fold, kzg_amd/csrc/verify_eval_batch.hip).  Group g opens t polynomials at one point z_g with ONE
witness: with the challenge gamma_g
    F_g = sum_i gamma_g^i p_{g,i}    y_F = sum_i gamma_g^i y_{g,i}    pi_g = [(F_g - y_F) / (X - z_g)]_1
and the verifier, with rho_{g,i} = r^g gamma_g^i and m(g,i) = idx[g t + i] (idx None: m = g t + i),
    c_m = sum_{m(g,i) = m} rho_{g,i}    Cagg = sum_m c_m C_m    yagg = sum rho_{g,i} y_{g,i}    P1 = sum_g r^g pi_g    P2 = sum_g r^g z_g pi_g
    ok = [ e(P1, hs[1]) e(-(P2 + Cagg - [yagg] gs[0]), hs[0]) == 1 ].
Points are carried as their discrete logs where tau is known (verdict); the scalars need no tau."""
from oracle import kzg_model as M

R = M.R


def fold(vecs, gamma):
    """sum_i gamma^i vecs[i], element by element (Horner from the last vector down, as the kernel); any integers count as residues"""
    acc = [0] * len(vecs[0])
    for v in reversed(vecs):
        acc = [(a * gamma + x) % R for a, x in zip(acc, v)]
    return acc


def fold_pieces(vecs, gamma, piece):
    """fold() with the vectors taken in pieces of at most `piece`, the last piece first and the running sum carried: the staging of
    host inputs"""
    acc, i1 = [0] * len(vecs[0]), len(vecs)
    while i1 > 0:
        i0 = max(0, i1 - piece)
        for v in reversed(vecs[i0:i1]):
            acc = [(a * gamma + x) % R for a, x in zip(acc, v)]
        i1 = i0
    return acc


def poly_eval(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def open_fold(polys, z, gamma, tau):
    """(ys, pi) of the honest folded opening of coefficient lists of one length at z: pi = q(tau) as a scalar; tau != z"""
    ys = [poly_eval(p, z) for p in polys]
    F = fold(polys, gamma)
    yF = poly_eval(F, z)
    assert yF == fold([[y] for y in ys], gamma)[0]
    return ys, (poly_eval(F, tau) - yF) * pow((tau - z) % R, R - 2, R) % R


def weights(r, gammas, t, first=0, count=None):
    """rho_{g,i} = r^g gammas[g]^i in the order k = g t + i, for k = first .. first + count - 1: a chunk that starts inside a group
    continues the call's sequence"""
    total = len(gammas) * t
    count = total - first if count is None else count
    out = []
    g, i = divmod(first, t)
    rg = pow(r, g, R)
    w = rg * pow(gammas[g], i, R) % R if count else 0
    for _ in range(count):
        out.append(w)
        i += 1
        if i == t:
            g, i = g + 1, 0
            rg = rg * r % R
            w = rg
        else:
            w = w * gammas[g] % R
    return out


def scalars(r, gammas, t, zs, ys, idx, n_commitments, chunk=None):
    """(rg, rg_z, c, yagg) of one call: the witness weights r^g and r^g z_g, the commitment weights and the value sum; with `chunk`
    the witnesses and then the values are worked in chunks of that many, as the library does"""
    groups, count = len(gammas), len(gammas) * t
    idx = list(range(count)) if idx is None else idx
    chunk = max(count, 1) if not chunk else chunk
    rg = [pow(r, g, R) for g in range(groups)]
    rg_z = [a * z % R for a, z in zip(rg, zs)]
    c, yagg = [0] * n_commitments, 0
    for k0 in range(0, count, chunk):
        B = min(chunk, count - k0)
        for k, p in zip(range(k0, k0 + B), weights(r, gammas, t, k0, B)):
            c[idx[k]] = (c[idx[k]] + p) % R
            yagg = (yagg + p * ys[k]) % R
    return rg, rg_z, c, yagg


def verdict(tau, r, gammas, t, zs, ys, commitments, idx, witnesses, chunk=None):
    """the combined check with known tau: commitments[m] = p_m(tau), witnesses[g] = q_g(tau) as scalars; ys flat, k = g t + i"""
    rg, rg_z, c, yagg = scalars(r, gammas, t, zs, ys, idx, len(commitments), chunk)
    P1 = sum(p * q for p, q in zip(rg, witnesses)) % R
    P2 = sum(p * q for p, q in zip(rg_z, witnesses)) % R
    Cagg = sum(a * b for a, b in zip(c, commitments)) % R
    return P1 * tau % R == (P2 + Cagg - yagg) % R
