"""CPU checks of the model of kzg_verify_cosets (tests/verify_cosets_model.py): the values -> interpolant map against the `r` of the
oracle's create_witness_batched, the signed-digit recoding of the fixed-base sum, and the known-tau verdict."""
import random

import pytest

from oracle import kzg_model as M
from tests import verify_cosets_model as V

SHAPES = [(1, 0), (2, 1), (3, 3), (4, 2), (6, 3)]
TAU = 0x7A05EED


def cells_of(coeffs, log_n, log_l):
    ev = list(coeffs) + [0] * ((1 << log_n) - len(coeffs))
    M.best_fft(ev, V.omega(log_n), log_n)  # in place
    K = 1 << (log_n - log_l)
    return [[ev[i + t * K] for t in range(1 << log_l)] for i in range(K)]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_interpolant_is_the_r_of_create_witness_batched(log_n, log_l):
    rng = random.Random(10 * log_n + log_l)
    N, l = 1 << log_n, 1 << log_l
    coeffs = [rng.randrange(M.R) for _ in range(N)]
    prover = M.KZGProver(M.setup(TAU, N))
    poly = M.Polynomial(coeffs, N - 1)
    cells = cells_of(coeffs, log_n, log_l)
    for i in sorted({0, 1 % (N // l), N // l - 1}):
        xs = V.coset_points(i, log_n, log_l)
        r = V.interpolant(cells[i], i, log_n, log_l)
        want, _w = prover.create_witness_batched(poly, xs, cells[i])
        # at the coset's points: for one point the reference's interpolation returns X + (y - x), which agrees there only
        assert [V.poly_eval(r, x) for x in xs] == [want.eval(x) for x in xs] == cells[i]
        if l > 1:
            assert r == (want.slice_coeffs() + [0] * l)[:l]


def test_digits_recompose_and_stay_in_range():
    rng = random.Random(3)
    for s in [0, 1, M.R - 1, (1 << 255) - 1, int("7f" * 32, 16), int("80" * 32, 16) % M.R, int("ff" * 31, 16)] + [rng.randrange(M.R) for _ in range(50)]:
        d = V.digits(s)
        assert len(d) == 32 and all(abs(x) <= 128 for x in d)
        assert sum(x << (8 * k) for k, x in enumerate(d)) == s


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_verdict_true_for_honest_cells_false_after_tampering(log_n, log_l):
    rng = random.Random(77 + log_n)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    coeffs = [rng.randrange(M.R) for _ in range(N)]
    other = [rng.randrange(M.R) for _ in range(N)]
    cells = cells_of(coeffs, log_n, log_l)
    C = V.poly_eval(coeffs, TAU)
    proofs = []
    for i in range(K):
        q = V.quotient_at(coeffs, V.interpolant(cells[i], i, log_n, log_l), i, log_n, log_l, TAU)
        assert q is not None
        proofs.append(q)
        assert V.verdict(TAU, C, q, cells[i], i, log_n, log_l)
    i = K - 1
    bad = list(cells[i])
    bad[rng.randrange(l)] = (bad[0] + 1) % M.R
    assert not V.verdict(TAU, C, proofs[i], bad, i, log_n, log_l)                                 # one value
    assert not V.verdict(TAU, C, (proofs[i] + 1) % M.R, cells[i], i, log_n, log_l)               # the proof
    assert not V.verdict(TAU, V.poly_eval(other, TAU), proofs[i], cells[i], i, log_n, log_l)      # the commitment
    if K > 1:
        assert not V.verdict(TAU, C, proofs[i], cells[i], 0, log_n, log_l)                        # the id
        if K >= 4:  # (with fewer than three chunks of l coefficients the quotient does not depend on the coset)
            assert not V.verdict(TAU, C, proofs[0], cells[i], i, log_n, log_l)                    # another cell's proof
    # a polynomial of at most l coefficients: the quotient is zero (the identity proof) and r = p
    short = coeffs[:l]
    sc = cells_of(short, log_n, log_l)
    assert V.interpolant(sc[0], 0, log_n, log_l) == short
    assert V.verdict(TAU, V.poly_eval(short, TAU), 0, sc[i], i, log_n, log_l)


def test_bindings_exist():
    import kzg_amd
    lib = kzg_amd.load()
    for s in ("kzg_cosets_verifier_setup", "kzg_cosets_verifier_free", "kzg_cosets_verifier_shape", "kzg_verify_cosets"):
        assert hasattr(lib, s)
    assert hasattr(kzg_amd.CosetVerifier, "verify") and hasattr(kzg_amd.KZGVerifier, "verify_cosets")
