"""Big-int model of kzg_open_eval's Fr stage (kzg_amd/csrc/open_eval.hip): an evaluation-form polynomial opened at any point of Fr.
evals[i] = p(w^i), i < d = 2^k, w = compute_omega(d).omega; returns y = p(z) and the values q_i of (p - y)/(X - z) on the domain."""
from oracle import kzg_model as M

R = M.R


def domain_index(d, z):
    """m with z = w^m, or None when z is not on the size-d domain.  z^d == 1 decides; the bits of m are read one per squaring
    level, lowest first: z^(d / 2^(j+1)) is rho^(m mod 2^j) or minus that, rho = w^(d / 2^(j+1))."""
    w = M.compute_omega(d)[2]
    z %= R
    if pow(z, d, R) != 1:
        return None
    m, j = 0, 0
    while (1 << j) < d:
        e = d >> (j + 1)
        v, low = pow(z, e, R), pow(w, e * m, R)
        if v != low:
            assert v == (R - low) % R
            m |= 1 << j
        j += 1
    assert pow(w, m, R) == z
    return m


def eval_at(evals, z):
    """y = (z^d - 1)/d sum_i f_i w^i / (z - w^i) off the domain, f_m at z = w^m"""
    d = len(evals)
    m = domain_index(d, z)
    if m is not None:
        return evals[m] % R
    w = M.compute_omega(d)[2]
    acc, wi = 0, 1
    for f in evals:
        acc = (acc + f * wi % R * M.fr_inv((z - wi) % R)) % R
        wi = wi * w % R
    return (pow(z, d, R) - 1) * M.fr_inv(d % R) % R * acc % R


def quotient_at(evals, z):
    """(y, q): q_i = (f_i - y)/(w^i - z) off the domain; on it q_j = (f_j - f_m)/(w^j - w^m) for j != m and
    q_m = -sum_{j != m} q_j w^(j - m) (the closed form of div_by_omega_i)"""
    d = len(evals)
    w = M.compute_omega(d)[2]
    y = eval_at(evals, z)
    m = domain_index(d, z)
    pw = [pow(w, i, R) for i in range(d)]
    if m is None:
        return y, [(f - y) * M.fr_inv((pw[i] - z) % R) % R for i, f in enumerate(evals)]
    q = [0] * d
    for j in range(d):
        if j != m:
            q[j] = (evals[j] - y) * M.fr_inv((pw[j] - pw[m]) % R) % R
            q[m] = (q[m] - q[j] * pw[(j - m) % d]) % R
    return y, q
