"""Fr-only model of the FK20 layout of kzg_amd/csrc/g1ntt.hip (every opening of one polynomial over its size-N domain), and the
GLV split of its twiddles.  The group is replaced by Fr itself (s_i = tau^i), so the model checks the index bookkeeping -- the
reversed SRS, the length-2N convolution, the folded 1/2N, the bit-reversed orders -- against direct quotients."""
from oracle import kzg_model as M

R = M.R
GLV_LAMBDA = 0xac45a4010001a40200000000ffffffff  # z^2 - 1; r = lambda^2 + lambda + 1
GLV_BETA = 0x1a0111ea397fe699ec02408663d4de85aa0d857d89759ad4897d29650fb85f9b409427eb4f49fffd8bfd00000000aaac


def glv_split(k):
    """k = k2 lambda + k1 by plain division (k < r): k1 < lambda, k2 <= lambda + 1."""
    k2, k1 = divmod(k, GLV_LAMBDA)
    return k1, k2


def signed_digits(v, ndig):
    """v + 0x88..8 read as nibbles minus 8 (least significant first), plus the carry out as the top digit."""
    t = v + int("8" * ndig, 16)
    return [((t >> (4 * i)) & 15) - 8 for i in range(ndig)], t >> (4 * ndig)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def dft(a, w):
    n = len(a)
    return [sum(a[j] * pow(w, j * m, R) for j in range(n)) % R for m in range(n)]


def fk20_model(coeffs, N, tau, srs_len=None):
    """All N witnesses q_m(tau) through the layout of g1ntt.hip, with s_i = tau^i for i < srs_len (else 0 = the identity)."""
    n = len(coeffs)
    assert 1 <= n <= N
    if N == 1:
        return [0]
    srs_len = N if srs_len is None else srs_len
    c = list(coeffs) + [0] * (N - n)
    s = [pow(tau, i, R) if i < srs_len else 0 for i in range(N)]
    two = 2 * N
    k = (two - 1).bit_length()
    w2 = M.compute_omega(two)[2]
    x = [s[N - 2 - j] if j <= N - 2 else 0 for j in range(two)]
    y = [c[N - 1]] + [0] * N + c[:N - 1]
    xh = dft(x, w2)
    xh_rev = [xh[bitrev(j, k)] for j in range(two)]               # the plan: DIF output, bit-reversed
    inv2n = pow(two, R - 2, R)
    yh = dft(y, w2)
    yh_rev = [yh[bitrev(j, k)] * inv2n % R for j in range(two)]   # folded scale, permuted in Fr
    hh_rev = [a * b % R for a, b in zip(xh_rev, yh_rev)]
    hh = [0] * two
    for j in range(two):
        hh[bitrev(j, k)] = hh_rev[j]
    H = dft(hh, pow(w2, R - 2, R))[:N]                              # DIT: bit-reversed in, natural out, first half
    return dft(H, M.compute_omega(N)[2])                            # DIF + bit-reversed read-out = natural order


def chunk_size(N):
    """Polynomials per chunk of fk20_run in g1ntt.hip (single-point and coset calls alike):
    max(1, min(FK20_MAX_CHUNK, FK20_CHUNK_POINTS / 2N))."""
    return max(1, min(4096, (1 << 21) // (2 * N)))


def coset_slices(l, two, batch):
    """Residue slices of a coset combination over `batch` x two frequencies (g1ntt.hip coset_slices, COSET_TARGET_THREADS
    = 2^17).  fk20_run takes S from its first chunk and keeps it for the ragged last one."""
    S = 1
    while S < l and batch * S * two < (1 << 17):
        S *= 2
    return S


def direct_witnesses(coeffs, N, tau):
    """q_m(tau) = (p(tau) - p(w^m)) / (tau - w^m) by synthetic division at every w^m."""
    w = M.compute_omega(N)[2]
    out = []
    for m in range(N):
        x = pow(w, m, R)
        # quotient coefficients of (p - p(x)) / (X - x)
        q = [0] * max(len(coeffs) - 1, 0)
        acc = 0
        for i in range(len(coeffs) - 1, 0, -1):
            acc = (acc * x + coeffs[i]) % R
            q[i - 1] = acc
        out.append(sum(qi * pow(tau, i, R) for i, qi in enumerate(q)) % R)
    return out
