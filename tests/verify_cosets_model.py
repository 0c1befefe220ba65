"""Big-int model of kzg_verify_cosets (kzg_amd/csrc/verify_cosets.hip).  Coset i of the size-N domain is {w^(i + tK) : t < l}, K = N / l,
nu = w^K; a cell is the l values v_t = p(w^(i + tK)).  Points are carried as their discrete logs (tau is known here), so the pairing
check e(pi, [tau^l - w^(il)]H) == e(C - R, H) is the Fr identity q (tau^l - w^(il)) == p(tau) - r(tau)."""
from oracle import kzg_model as M

R = M.R
WINDOW = 8  # VC_C


def omega(log_n):
    return M.compute_omega(1 << log_n)[2]


def coset_points(i, log_n, log_l):
    w, K = omega(log_n), 1 << (log_n - log_l)
    return [pow(w, i + t * K, R) for t in range(1 << log_l)]


def interpolant(values, i, log_n, log_l):
    """step 1: u = iNTT_l(values) over nu, r_j = u_j w^(-ij): the l coefficients of the polynomial through the cell"""
    l, w = 1 << log_l, omega(log_n)
    assert len(values) == l
    nu_inv, w_inv, l_inv = pow(w, -(1 << (log_n - log_l)), R), pow(w, -1, R), pow(l, -1, R)
    u = [l_inv * sum(v * pow(nu_inv, j * t, R) for t, v in enumerate(values)) % R for j in range(l)]
    return [u[j] * pow(w_inv, i * j, R) % R for j in range(l)]


def digits(s, c=WINDOW):
    """step 2's recoding (vc_digit): digit `win` from bits [c win - 1, c win + c) alone, |d| <= 2^(c-1), sum d 2^(c win) = s < 2^256"""
    W = (256 + c - 1) // c
    x = s << 1
    out = []
    for win in range(W):
        b = (x >> (c * win)) & ((2 << c) - 1)
        d = (b >> 1) + (b & 1)
        out.append(d - (1 << c) if b >> c else d)
    return out


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def verdict(tau, commitment, proof, values, i, log_n, log_l):
    """step 3 with known tau: commitment = p(tau) and proof = q_i(tau) as scalars"""
    r = interpolant(values, i, log_n, log_l)
    z = (pow(tau, 1 << log_l, R) - pow(omega(log_n), i << log_l, R)) % R
    return (commitment - poly_eval(r, tau)) % R == proof * z % R


def quotient_at(coeffs, r, i, log_n, log_l, tau):
    """q_i(tau) for (p - r_i) / (X^l - w^(il)) by long division (None if it leaves a remainder)"""
    l = 1 << log_l
    c = pow(omega(log_n), i << log_l, R)
    num = [(a - (r[k] if k < l else 0)) % R for k, a in enumerate(list(coeffs) + [0] * max(0, l - len(coeffs)))]
    q = [0] * max(0, len(num) - l)
    for k in range(len(num) - 1, l - 1, -1):  # X^k = X^(k-l) (X^l - c) + c X^(k-l)
        q[k - l] = num[k]
        num[k - l] = (num[k - l] + c * num[k]) % R
        num[k] = 0
    if any(num[:l]):
        return None
    return poly_eval(q, tau)
