"""Big-int model of kzg_verify_cosets_batch (kzg_amd/csrc/verify_cosets_batch.hip) on top of tests/verify_cosets_model.py.  Cell k has
commitment index m_k, coset i_k, values v_k and proof pi_k; with the challenge r the weights are rho_k = r^k over the whole call and
    a_j = sum_k rho_k r_{k,j}    c_m = sum_{k: m_k = m} rho_k    P1 = sum_k rho_k pi_k    P2 = sum_k (rho_k w^(i_k l)) pi_k
    ok  = [ e(P1, hs[l]) e(-(P2 + Cagg - Ragg), hs[0]) == 1 ],  Ragg = sum_j a_j gs[j],  Cagg = sum_m c_m C_m.
Points are carried as their discrete logs where tau is known (verdict); the scalars (weights, a, c, rho h) need no tau."""
from tests import verify_cosets_model as V

R = V.R


def weights(r, count, first=0):
    """rho_k = r^k for k = first .. first + count - 1: a chunk that starts at cell `first` continues the call's sequence"""
    out, rho = [], pow(r, first, R)
    for _ in range(count):
        out.append(rho)
        rho = rho * r % R
    return out


def scalars(r, idx, ids, cells, n_commitments, log_n, log_l, chunk=None):
    """(a, c, rho, rho_h) of one call; with `chunk` the cells are worked in chunks of that many, as the library does"""
    l, w = 1 << log_l, V.omega(log_n)
    count = len(ids)
    chunk = count if not chunk else chunk
    a, c, rho, rho_h = [0] * l, [0] * n_commitments, [], []
    for k0 in range(0, count, chunk):
        B = min(chunk, count - k0)
        for k, p in zip(range(k0, k0 + B), weights(r, B, k0)):
            rk = V.interpolant(cells[k], ids[k], log_n, log_l)
            for j in range(l):
                a[j] = (a[j] + p * rk[j]) % R
            c[idx[k]] = (c[idx[k]] + p) % R
            rho.append(p)
            rho_h.append(p * pow(w, ids[k] << log_l, R) % R)
    return a, c, rho, rho_h


def verdict(tau, r, commitments, idx, ids, cells, proofs, log_n, log_l, chunk=None):
    """the combined check with known tau: commitments[m] = p_m(tau) and proofs[k] = q_k(tau) as scalars"""
    a, c, rho, rho_h = scalars(r, idx, ids, cells, len(commitments), log_n, log_l, chunk)
    P1 = sum(p * q for p, q in zip(rho, proofs)) % R
    P2 = sum(p * q for p, q in zip(rho_h, proofs)) % R
    Cagg = sum(x * y for x, y in zip(c, commitments)) % R
    Ragg = V.poly_eval(a, tau)
    return P1 * pow(tau, 1 << log_l, R) % R == (P2 + Cagg - Ragg) % R
