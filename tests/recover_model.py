"""Big-int model of kzg_recover_cosets (kzg_amd/csrc/recover.hip): a polynomial of at most n coefficients from any `known` of the
K = N / l cosets C_i = { w^(i + tK) : t < l } of its size-N domain with known * l >= n.  The six steps of the call in Fr, and the
zero polynomial through the layout of the GPU's product tree: roots padded with zeros to LEAF * 2^k, a monic polynomial kept as
its low coefficients (the leading 1 implicit), pairs multiplied by a decimation-in-frequency transform forward, a pointwise
product and a decimation-in-time transform back (bit-reversed in between, no permutation), with the inverse twiddles taken from
the forward table as w^-j = -w^(h - j)."""
from oracle import kzg_model as M

R = M.R
LEAF = 256      # roots per leaf workgroup: REC_LEAF in recover.hip (tests/test_recover_model.py compares the two)
SHIFT = 7       # Scalar::multiplicative_generator(), the coset of the division


def ntt(a, inverse=False):
    """natural order in and out over compute_omega(len(a)); the inverse scales by 1 / len(a)"""
    n = len(a)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    w = M.compute_omega(n)[2]
    out = [v % R for v in a]
    M.serial_fft(out, pow(w, R - 2, R) if inverse else w, log_n)
    if inverse:
        ninv = pow(n, R - 2, R)
        out = [v * ninv % R for v in out]
    return out


def chunk_size(N):
    """polynomials per chunk of kzg_recover_cosets: the rule of fk20_run, max(1, min(4096, 2^21 / 2N))"""
    return max(1, min(4096, (1 << 21) // (2 * N)))


def padded_roots(m, leaf=LEAF):
    """Mpad: the root count of the padded tree"""
    mpad = leaf
    while mpad < m:
        mpad *= 2
    return mpad


def tree_launches(m, leaf=LEAF):
    """kernel launches of the zero polynomial's tree in recover.hip (roots, leaves, the twiddle table, the levels)"""
    log_t = padded_roots(m, leaf).bit_length() - 1
    count = 2 + (1 if log_t > leaf.bit_length() - 1 else 0)
    for s in range(leaf.bit_length(), log_t + 1):
        count += 1 if s <= 10 else 5 + 2 * (s - 11)
    return count


# ---- the transforms of the tree, butterfly by butterfly as the kernels do them ---------------------------------------------
def _tw(table, j, log_h, log_t, inverse):
    sh = log_t - 1 - log_h
    if not inverse:
        return table[j << sh]
    return 1 if j == 0 else (-table[((1 << log_h) - j) << sh]) % R


def _stage(x, log_h, table, log_t, inverse):
    h = 1 << log_h
    for p in range(len(x) // 2):
        j = p & (h - 1)
        i0 = ((p >> log_h) << (log_h + 1)) | j
        i1 = i0 + h
        w = _tw(table, j, log_h, log_t, inverse)
        if not inverse:
            u, v = x[i0], x[i1]
            x[i0], x[i1] = (u + v) % R, (u - v) * w % R
        else:
            u, v = x[i0], x[i1] * w % R
            x[i0], x[i1] = (u + v) % R, (u - v) % R


def tree_dif(x, s, table, log_t):
    """arrays of 2^s points, contiguous in x: natural in, bit-reversed out"""
    for log_h in range(s - 1, -1, -1):
        _stage(x, log_h, table, log_t, False)


def tree_dit(x, s, table, log_t):
    """bit-reversed in, natural out, times 2^s"""
    for log_h in range(s):
        _stage(x, log_h, table, log_t, True)


def leaf_product(roots):
    """low coefficients of prod (Y - r): c_j <- c_{j-1} - r c_j with the implicit c_i = 1"""
    c = [0] * len(roots)
    for i, r in enumerate(roots):
        old = list(c)
        for j in range(i + 1):
            cj = old[j] if j < i else 1
            cm = old[j - 1] if j >= 1 else 0
            c[j] = (cm - r * cj) % R
    return c


def zero_poly_tree(roots, leaf=LEAF):
    """The m + 1 coefficients of prod (Y - r) through the padded tree: (Y^d + a')(Y^d + b') = Y^2d + Y^d (a' + b') + a' b', and
    a' b' is a cyclic product of 2d points that does not wrap."""
    m = len(roots)
    mpad = padded_roots(m, leaf)
    log_t = mpad.bit_length() - 1
    padded = [r % R for r in roots] + [0] * (mpad - m)
    cur = []
    for b in range(mpad // leaf):
        cur += leaf_product(padded[b * leaf:(b + 1) * leaf])
    table = []
    if mpad > leaf:
        w, v = M.compute_omega(mpad)[2], 1
        for _ in range(mpad // 2):
            table.append(v)
            v = v * w % R
    for s in range(leaf.bit_length(), log_t + 1):
        S, d = 1 << s, 1 << (s - 1)
        f = []
        for i in range(mpad // d):
            f += cur[i * d:(i + 1) * d] + [0] * d
        tree_dif(f, s, table, log_t)
        g = []
        for q in range(mpad // S):
            g += [f[2 * q * S + k] * f[(2 * q + 1) * S + k] % R for k in range(S)]
        tree_dit(g, s, table, log_t)
        sinv = pow(S, R - 2, R)
        nxt = [v * sinv % R for v in g]
        for e in range(mpad):
            if e & (S - 1) >= d:
                nxt[e] = (nxt[e] + cur[e - d] + cur[e]) % R
        cur = nxt
    pad = mpad - m
    assert not any(cur[:pad]), "the padded product is Y^pad Zs(Y)"
    return cur[pad:] + [1]


def zero_poly_plain(roots):
    z = [1]
    for r in roots:
        z = [((z[j - 1] if j else 0) - r * (z[j] if j < len(z) else 0)) % R for j in range(len(z) + 1)]
    return z


# ---- the call ----------------------------------------------------------------------------------------------------------------
def coset_cells(coeffs, N, l, ids, evals=None):
    """the cells of `ids`: cell j = [p(w^(id_j + tK)) for t < l]"""
    K = N // l
    ev = evals if evals is not None else ntt(list(coeffs) + [0] * (N - len(coeffs)))
    return [[ev[i + t * K] for t in range(l)] for i in ids]


def recover_with_tree(N, l, n, ids, cells):
    """recover() with the zero polynomial built the way the GPU builds it (zero_poly_tree over the missing ids in ascending order)"""
    K = N // l
    nu = pow(M.compute_omega(N)[2], l, R)
    known = set(ids)
    return recover(N, l, n, ids, cells, zs=zero_poly_tree([pow(nu, i, R) for i in range(K) if i not in known]))


def recover(N, l, n, ids, cells, zs=None):
    """(coefficients [0, n), the N evaluations, consistent) by the six steps of the call.  zs: the zero polynomial's coefficients
    if the caller has them (else the plain product)."""
    K = N // l
    known = len(ids)
    assert N % l == 0 and 1 <= n <= N and 1 <= known <= K and known * l >= n and len(set(ids)) == known and max(ids) < K
    known_ids = set(ids)
    missing = [i for i in range(K) if i not in known_ids]
    m = len(missing)
    w = M.compute_omega(N)[2]
    nu = pow(w, l, R)
    if zs is None:
        zs = zero_poly_plain([pow(nu, i, R) for i in missing])
    assert len(zs) == m + 1
    zpad = list(zs) + [0] * (K - m - 1)
    zv = ntt(zpad) if K > 1 else list(zpad)                                  # Zs(nu^j)
    g = pow(SHIFT, l, R)
    zc = [c * pow(g, j, R) % R for j, c in enumerate(zpad)]
    zc = ntt(zc) if K > 1 else zc                                            # Zs(7^l nu^j)
    zinv = [pow(v, R - 2, R) for v in zc]
    ez = [0] * N
    for j, i in enumerate(ids):
        for t in range(l):
            ez[i + t * K] = cells[j][t] * zv[i] % R
    pz = ntt(ez, inverse=True) if N > 1 else ez                              # p Z, exactly
    consistent = not any(pz[n + m * l:])
    on = [c * pow(SHIFT, j, R) % R for j, c in enumerate(pz)]
    on = ntt(on) if N > 1 else on
    on = [v * zinv[j % K] % R for j, v in enumerate(on)]
    p = ntt(on, inverse=True) if N > 1 else on
    sinv = pow(SHIFT, R - 2, R)
    p = [c * pow(sinv, j, R) % R for j, c in enumerate(p)]
    coeffs = p[:n]
    evals = ntt(coeffs + [0] * (N - n)) if N > 1 else list(coeffs)
    return coeffs, evals, consistent
