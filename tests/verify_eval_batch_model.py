"""Big-int model of kzg_verify_eval_batch (kzg_amd/csrc/verify_eval_batch.hip).  Opening k claims p_{m_k}(x_k) = y_k with the witness
pi_k, m_k = idx[k] (idx None: m_k = k, one commitment per opening); with the challenge r the weights are rho_k = r^k over the whole
call and
    P1 = sum_k rho_k pi_k    P2 = sum_k (rho_k x_k) pi_k    c_m = sum_{k: m_k = m} rho_k    Cagg = sum_m c_m C_m    yagg = sum_k rho_k y_k
    ok = [ e(P1, hs[1]) e(-(P2 + Cagg - [yagg] gs[0]), hs[0]) == 1 ].
Points are carried as their discrete logs where tau is known (verdict, opening_ok); the scalars need no tau."""
from oracle import kzg_model as M

R = M.R


def weights(r, count, first=0):
    """rho_k = r^k for k = first .. first + count - 1: a chunk that starts at opening `first` continues the call's sequence"""
    out, rho = [], pow(r, first, R)
    for _ in range(count):
        out.append(rho)
        rho = rho * r % R
    return out


def scalars(r, xs, ys, idx, n_commitments, chunk=None):
    """(rho, rho_x, c, yagg) of one call; with `chunk` the openings are worked in chunks of that many, as the library does"""
    count = len(xs)
    idx = list(range(count)) if idx is None else idx
    chunk = count if not chunk else chunk
    rho, rho_x, c, yagg = [], [], [0] * n_commitments, 0
    for k0 in range(0, count, chunk):
        B = min(chunk, count - k0)
        for k, p in zip(range(k0, k0 + B), weights(r, B, k0)):
            rho.append(p)
            rho_x.append(p * xs[k] % R)
            c[idx[k]] = (c[idx[k]] + p) % R
            yagg = (yagg + p * ys[k]) % R
    return rho, rho_x, c, yagg


def poly_eval(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def witness_at(coeffs, x, tau):
    """(y, q(tau)) of the honest opening of the polynomial at x: q = (p - y) / (X - x); tau != x"""
    y = poly_eval(coeffs, x)
    return y, (poly_eval(coeffs, tau) - y) * pow((tau - x) % R, R - 2, R) % R


def opening_ok(tau, x, y, commitment, witness):
    """the check of kzg_verify_eval for one opening: e(pi, hs[1] - [x] hs[0]) == e(C - [y] gs[0], hs[0])"""
    return witness * (tau - x) % R == (commitment - y) % R


def verdict(tau, r, xs, ys, commitments, idx, witnesses, chunk=None):
    """the combined check with known tau: commitments[m] = p_m(tau) and witnesses[k] = q_k(tau) as scalars"""
    rho, rho_x, c, yagg = scalars(r, xs, ys, idx, len(commitments), chunk)
    P1 = sum(p * q for p, q in zip(rho, witnesses)) % R
    P2 = sum(p * q for p, q in zip(rho_x, witnesses)) % R
    Cagg = sum(a * b for a, b in zip(c, commitments)) % R
    return P1 * tau % R == (P2 + Cagg - yagg) % R
