"""CPU checks of the multi-point FK20 layout of kzg_amd/csrc/g1ntt.hip (every coset opening of a polynomial over its size-N
domain).  The group is replaced by Fr itself (s_v = tau^v), so the model checks the index bookkeeping -- the residue split, the
per-residue reversed SRS, the l-term combination in the frequency domain, the folded 1/2K, the bit-reversed orders -- against
direct long division by X^l - w^(il); the interpolants' DFT formula is checked against the oracle's lagrange_interpolation."""
import ctypes
import random

import pytest

from oracle import kzg_model as M
from tests import fk20_model as F

R = M.R


def cosets_model(coeffs, N, l, tau, srs_len=None):
    """All K = N / l coset witnesses q_i(tau) through the layout of g1ntt.hip, s_v = tau^v for v < srs_len (else 0 = the
    identity)."""
    n = len(coeffs)
    assert 1 <= n <= N and N % l == 0
    K = N // l
    srs_len = N if srs_len is None else srs_len
    c = list(coeffs) + [0] * (N - n)
    s = [pow(tau, v, R) if v < srs_len else 0 for v in range(N)]
    two = 2 * K
    k = (two - 1).bit_length()
    w2 = M.compute_omega(two)[2]
    inv2k = pow(two, R - 2, R)
    hh_rev = [0] * two
    for r in range(l):
        x = [s[r + (K - 2 - j) * l] if j <= K - 2 else 0 for j in range(two)]
        cr = [c[r + t * l] for t in range(K)]
        y = [cr[K - 1]] + [0] * K + cr[:K - 1]
        xh, yh = F.dft(x, w2), F.dft(y, w2)
        for j in range(two):                                   # the plan's Xh^(r) and yh^(r) are both bit-reversed
            hh_rev[j] = (hh_rev[j] + xh[F.bitrev(j, k)] * yh[F.bitrev(j, k)] * inv2k) % R
    hh = [0] * two
    for j in range(two):
        hh[F.bitrev(j, k)] = hh_rev[j]
    h = F.dft(hh, pow(w2, R - 2, R))[:K]                       # DIT, first half
    return F.dft(h, M.compute_omega(K)[2]) if K > 1 else h     # DIF + bit-reversed read-out = natural coset order


def cosets_interpolants(coeffs, N, l):
    """coefficient r of I_i = sum_t c^(r)_t w_K^(it) = DFT_K(c^(r))_i -> K lists of l coefficients"""
    K = N // l
    c = list(coeffs) + [0] * (N - len(coeffs))
    wk = M.compute_omega(K)[2] if K > 1 else 1
    cols = [F.dft([c[r + t * l] for t in range(K)], wk) for r in range(l)]
    return [[cols[r][i] for r in range(l)] for i in range(K)]


def direct_cosets(coeffs, N, l, tau):
    """(q_i(tau), I_i) by long division of p by X^l - w^(il)"""
    K = N // l
    w = M.compute_omega(N)[2]
    out = []
    for i in range(K):
        z = pow(w, i * l, R)
        rem = list(coeffs) + [0] * max(0, l - len(coeffs))
        q = [0] * max(0, len(coeffs) - l)
        for d in range(len(coeffs) - 1, l - 1, -1):           # X^d = X^(d-l) (X^l - z) + z X^(d-l)
            a = rem[d]
            rem[d] = 0
            q[d - l] = a
            rem[d - l] = (rem[d - l] + a * z) % R
        out.append((sum(qv * pow(tau, v, R) for v, qv in enumerate(q)) % R, rem[:l]))
    return out


CASES = [(N, l) for N in (2, 4, 8, 16, 32, 64) for l in (2, 4, 8, 16, 32, 64) if l <= N]


@pytest.mark.parametrize("N,l", CASES)
def test_layout_matches_long_division(N, l):
    rng = random.Random(31 * N + l)
    tau = rng.randrange(1, R)
    for n in sorted({1, max(1, l - 1), l, min(N, l + 1), max(1, N - 3), N}):
        coeffs = [rng.randrange(R) for _ in range(n)]
        direct = direct_cosets(coeffs, N, l, tau)
        assert cosets_model(coeffs, N, l, tau) == [q for q, _ in direct], (N, l, n)
        assert cosets_interpolants(coeffs, N, l) == [r for _, r in direct], (N, l, n)


@pytest.mark.parametrize("N,l", [(8, 2), (16, 4), (32, 8), (16, 16), (64, 4)])
def test_short_srs_is_exact(N, l):
    # SRS points past len(srs) count as the identity: exact whenever n <= l or n - l <= len(srs) (whole residue classes of the
    # plan's bases are then the identity)
    rng = random.Random(77 + N + l)
    tau = rng.randrange(1, R)
    for n in range(1, N + 1):
        coeffs = [rng.randrange(R) for _ in range(n)]
        srs_len = max(0, n - l)
        assert cosets_model(coeffs, N, l, tau, srs_len=srs_len) == [q for q, _ in direct_cosets(coeffs, N, l, tau)], (N, l, n)


def test_coset_roots_and_interpolants_match_oracle():
    # w_N^l = w_K, so the coset points are the roots of X^l - w^(il); the DFT interpolant equals the reference's
    rng = random.Random(3)
    for N, l in [(16, 4), (32, 2), (8, 8), (64, 16)]:
        K = N // l
        w = M.compute_omega(N)[2]
        assert pow(w, l, R) == (M.compute_omega(K)[2] if K > 1 else 1)
        n = rng.randrange(min(l + 1, N), N + 1)
        coeffs = [rng.randrange(R) for _ in range(n)]
        p = M.Polynomial(coeffs, n - 1)
        interp = cosets_interpolants(coeffs, N, l)
        for i in range(K):
            xs = [pow(w, i + t * K, R) for t in range(l)]
            assert all(pow(x, l, R) == pow(w, i * l, R) for x in xs)
            ys = [p.eval(x) for x in xs]
            ref = M.Polynomial.lagrange_interpolation(xs, ys)
            assert ref.slice_coeffs() + [0] * (l - ref.num_coeffs()) == interp[i], (N, l, i)


SYMBOLS = ["kzg_fk20_cosets_setup", "kzg_fk20_cosets_free", "kzg_fk20_cosets_shape", "kzg_witness_cosets_coeff",
           "kzg_witness_cosets_eval"]


def test_library_exports_coset_calls():
    import kzg_amd
    from kzg_amd import _lib
    assert hasattr(kzg_amd, "FK20CosetPlan")
    for m in ("domain", "coset_size", "num_cosets", "coset_points", "free"):
        assert callable(getattr(kzg_amd.FK20CosetPlan, m))
    for cls, m in ((kzg_amd.KZGProver, "create_witness_all_cosets"), (kzg_amd.KZGProver, "create_witness_all_cosets_batch"),
                   (kzg_amd.KZGProverEvalForm, "create_witness_all_cosets")):
        assert callable(getattr(cls, m)), m
    lib = ctypes.CDLL(_lib.SO_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
