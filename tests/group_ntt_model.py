"""Python-integer model of the group DFTs (kzg_ntt_g1 / kzg_ntt_g2, kzg_amd/csrc/g1ntt.hip and g2ntt.hip) and of the G2 twiddle
multiplier: the untwist-Frobenius-twist endomorphism psi, the base-u split of a scalar, the signed 4-bit recoding and the joint
double-and-add chain, on the primitives of oracle.pairing_model / oracle.kzg_model."""
from oracle import kzg_model as M
from oracle import pairing_model as PM

Q, R = M.Q, M.R
U = PM.BLS_Z_ABS          # |z|; the curve parameter is z = -U and r = U^4 - U^2 + 1
Z_MOD_R = (-U) % R
assert R == U ** 4 - U ** 2 + 1


def psi_candidates():
    """the two (c_x, c_y) pairs the twist convention leaves open: (xi^((q-1)/3), xi^((q-1)/2)) and the inverses"""
    cx, cy = PM.f2_pow(PM.XI, (Q - 1) // 3), PM.f2_pow(PM.XI, (Q - 1) // 2)
    return [(cx, cy), (PM.f2_inv(cx), PM.f2_inv(cy))]


def psi_with(P, cx, cy):
    if P is None:
        return None
    return (PM.f2_mul(cx, PM.f2_conj(P[0])), PM.f2_mul(cy, PM.f2_conj(P[1])))


def derive_psi_consts():
    """the pair with psi(H) = [z mod r] H"""
    want = PM.g2_mul(PM.G2, Z_MOD_R)
    for cx, cy in psi_candidates():
        if psi_with(PM.G2, cx, cy) == want:
            return cx, cy
    raise AssertionError("no psi constants")


def psi(P, consts, times=1):
    for _ in range(times):
        P = psi_with(P, consts[0], consts[1])
    return P


def split_u(k):
    """k < r as k0 + k1 u + k2 u^2 + k3 u^3, every k_i < u: three divisions by the 64-bit constant"""
    out = []
    for _ in range(3):
        k, rem = divmod(k, U)
        out.append(rem)
    out.append(k)
    return out


def recode64(v):
    """v < 2^64 -> 17 signed digits in [-8, 7], least significant first: sum d_i 16^i = v (the 17th is the carry out of bit 63)"""
    t = v + 0x8888888888888888
    return [((t >> (4 * i)) & 15) - 8 for i in range(16)] + [t >> 64]


def recode256(v):
    """v < r -> 64 signed digits (no carry out: r + 0x88..8 < 2^256)"""
    t = v + int("8" * 64, 16)
    assert t < 1 << 256
    return [((t >> (4 * i)) & 15) - 8 for i in range(64)]


def _table(P):
    tab, acc = [], None
    for _ in range(8):
        acc = PM.g2_add(acc, P)
        tab.append(acc)
    return tab


def gls_mul(P, k, consts):
    """[k]P by the joint chain over (P, -psi P, psi^2 P, -psi^3 P): the order of operations of the kernel"""
    k %= R
    digs = [recode64(v) for v in split_u(k)]
    tab = _table(P)

    def term(i, d):
        T = psi(tab[abs(d) - 1], consts, i)
        return PM.g2_neg(T) if (d < 0) != (i & 1 == 1) else T

    acc = None
    for i in range(4):
        if digs[i][16]:
            acc = PM.g2_add(acc, term(i, 1))
    for nib in range(15, -1, -1):
        for _ in range(4):
            acc = PM.g2_add(acc, acc)
        for i in range(4):
            if digs[i][nib]:
                acc = PM.g2_add(acc, term(i, digs[i][nib]))
    return acc


def plain_mul(P, k):
    """the comparison route: signed 4-bit digits over the whole scalar"""
    digs = recode256(k % R)
    tab = _table(P)
    acc = None
    for nib in range(63, -1, -1):
        for _ in range(4):
            acc = PM.g2_add(acc, acc)
        d = digs[nib]
        if d:
            T = tab[abs(d) - 1]
            acc = PM.g2_add(acc, PM.g2_neg(T) if d < 0 else T)
    return acc


class Group:
    def __init__(self, add, mul, neg):
        self.add, self.mul, self.neg = add, mul, neg


G1 = Group(M.g1_add, M.g1_mul, M.g1_neg)
G2 = Group(PM.g2_add, PM.g2_mul, PM.g2_neg)


def omega(d):
    return M.compute_omega(d)[2]


def dft_naive(grp, pts, inverse=False):
    """forward: out[m] = sum_j [w^(jm)] P[j]; inverse: out[j] = [1/d] sum_m [w^(-jm)] P[m]"""
    d = len(pts)
    w = omega(d) if d > 1 else 1
    if inverse:
        w = pow(w, -1, R)
    out = []
    for m in range(d):
        acc = None
        for j, P in enumerate(pts):
            acc = grp.add(acc, grp.mul(P, pow(w, j * m, R)))
        out.append(grp.mul(acc, pow(d, -1, R)) if inverse else acc)
    return out


def _brev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def dft(grp, pts, inverse=False):
    """the shape of the kernels: forward = DIF (natural in, bit-reversed out, read out reversed); inverse = DIT on the bit-reversed
    input with the inverse twiddles, then the 1/d product"""
    d = len(pts)
    bits = d.bit_length() - 1
    assert 1 << bits == d
    if d == 1:
        return list(pts)
    w = omega(d)
    if inverse:
        w = pow(w, -1, R)
    tw = [pow(w, e, R) for e in range(d // 2)]
    if not inverse:
        A = list(pts)
        m = d // 2
        while m >= 1:
            for j in range(d // (2 * m)):
                for i in range(m):
                    i0, i1 = j * 2 * m + i, j * 2 * m + i + m
                    x, y = A[i0], A[i1]
                    A[i0] = grp.add(x, y)
                    D = grp.add(x, grp.neg(y))
                    A[i1] = D if m == 1 else grp.mul(D, tw[i * (d // (2 * m))])
            m //= 2
        return [A[_brev(i, bits)] for i in range(d)]
    A = [pts[_brev(i, bits)] for i in range(d)]
    m = 1
    while m <= d // 2:
        for j in range(d // (2 * m)):
            for i in range(m):
                i0, i1 = j * 2 * m + i, j * 2 * m + i + m
                x = A[i0]
                T = A[i1] if m == 1 else grp.mul(A[i1], tw[i * (d // (2 * m))])
                A[i0] = grp.add(x, T)
                A[i1] = grp.add(x, grp.neg(T))
        m *= 2
    dinv = pow(d, -1, R)
    return [grp.mul(P, dinv) for P in A]


# the multiplier's edge scalars (digit and carry boundaries, the powers of u, word boundaries, maximal carry chains)
EDGE_SCALARS = [0, 1, 7, 8, 9, 15, 16, U - 1, U, U + 1, U ** 2, U ** 3, U ** 4 - U ** 2, R - 2, 2 ** 64 - 1, 2 ** 64, 2 ** 128,
                int("7" * 64, 16) % R, int("8" * 64, 16) % R, int("7" * 16, 16), int("8" * 16, 16),
                sum(int("7" * 16, 16) * U ** i for i in range(4)) % R, sum(int("8" * 16, 16) * U ** i for i in range(4)) % R]
