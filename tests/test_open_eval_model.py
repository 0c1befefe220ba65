"""tests/open_eval_model.py against the oracle (oracle/kzg_model.py): the barycentric value is the polynomial's value after an
inverse transform, the quotient's values are the long division by X - z transformed back, and on the domain they are
div_by_omega_i of (evals - evals[m])."""
import random

import pytest

from oracle import kzg_model as M
from tests import open_eval_model as OM

R = M.R
SIZES = [1, 2, 4, 8, 64]


def coeffs_of(evals):
    e = M.EvaluationDomain.from_coeffs(list(evals))
    e.ifft()
    return e.coeffs


def evals_of(coeffs, d):
    e = M.EvaluationDomain.from_coeffs(list(coeffs) + [0] * (d - len(coeffs)))
    e.fft()
    return e.coeffs


def points(d, rng):
    w = M.compute_omega(d)[2]
    w2 = M.compute_omega(2 * d)[2]          # a primitive 2d-th root: off the domain, z^d = -1
    on = sorted({0, 1 % d, d // 2, d - 1})
    return [(pow(w, m, R), m) for m in on] + [(z, None) for z in (rng.randrange(R), 0, w2, 7) if pow(z, d, R) != 1]


@pytest.mark.parametrize("d", SIZES)
def test_model_matches_the_oracle(d):
    rng = random.Random(900 + d)
    for evals in ([rng.randrange(R) for _ in range(d)], [0] * d, [5] * d, [R - 1] * d, evals_of([rng.randrange(R) for _ in range(d - 1)] + [1], d)):
        coeffs = coeffs_of(evals)
        assert evals_of(coeffs, d) == [v % R for v in evals]
        for z, m in points(d, rng):
            assert OM.domain_index(d, z) == m
            y, q = OM.quotient_at(evals, z)
            assert y == OM.eval_at(evals, z) == M.Polynomial(coeffs, d - 1).eval(z)
            # (p - y) / (X - z) by long division, transformed back to the domain
            dividend = M.Polynomial(list(coeffs), d - 1)
            dividend.coeffs[0] = (dividend.coeffs[0] - y) % R
            if d == 1:
                assert q == [0]
                continue
            psi, rem = dividend.long_division(M.Polynomial([M.fr_neg(z), 1], 1))
            assert rem is None
            assert q == evals_of(psi.coeffs[:d - 1], d), (d, z)
            if m is not None:
                shifted = M.EvaluationDomain.from_coeffs([(f - evals[m]) % R for f in evals])
                assert q == M.div_by_omega_i(shifted, m).coeffs


def test_degree_and_constant_vectors():
    rng = random.Random(7)
    d = 8
    top = evals_of([rng.randrange(R) for _ in range(d - 1)] + [1], d)
    assert coeffs_of(top)[d - 1] == 1                       # degree exactly d - 1
    y, q = OM.quotient_at([5] * d, 12345)
    assert y == 5 and q == [0] * d                          # a constant: q = 0, the witness is the identity
