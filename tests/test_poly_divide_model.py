"""The algorithm of kzg_poly_divide (tests/poly_divide_model.py: base recurrence, Newton doubling with a truncated last level, the
reversed quotient, the remainder folded modulo X^N - 1) against oracle.kzg_model.Polynomial.long_division, before a GPU sees it."""
import random

import pytest

from oracle import kzg_model as M
from tests import poly_divide_model as PD

R = M.R
SHAPES = [(1, 1), (5, 1), (1, 2), (2, 2), (3, 2), (9, 2), (4, 5), (8, 8), (9, 8), (10, 8), (17, 9), (33, 17), (40, 33), (300, 200),
          (257, 2), (256, 129), (520, 257), (521, 258), (1000, 3)]
B0 = PD.DEFAULT_BASE
# m = na - nb + 1 one below, at and one above the default base precision; nb - 1 one below, at and one above a power of two
SHAPES += [(B0 + 1, 3), (B0 + 2, 3), (B0 + 3, 3), (2 * B0 + 9, 10), (40, 16), (40, 17), (40, 18), (90, 64), (90, 65), (90, 66)]
BASES = [1, 4, B0]


def oracle_divide(a, b):
    """the reference's quotient and remainder zero-padded to na - nb + 1 and nb - 1 coefficients (b[-1] != 0)"""
    na, nb = len(a), len(b)
    q, r = M.Polynomial(a).long_division(M.Polynomial(b))
    if na < nb:
        return [], [x % R for x in a] + [0] * (nb - 1 - na)
    qc = q.coeffs[: q.degree + 1]
    rc = [] if r is None else r.coeffs[: r.degree + 1]
    return qc + [0] * (na - nb + 1 - len(qc)), rc + [0] * (nb - 1 - len(rc))


def case(na, nb, seed=0):
    rng = random.Random(1000 * na + nb + seed)
    a = [rng.randrange(R) for _ in range(na)]
    b = [rng.randrange(R) for _ in range(nb - 1)] + [rng.randrange(1, R)]
    return a, b


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_model_equals_long_division(na, nb, base):
    a, b = case(na, nb)
    assert PD.divide(a, b, base) == oracle_divide(a, b)


def test_m_nine_runs_four_and_two_levels_with_a_truncated_last_one():
    a, b = case(10, 2)
    for base, want in ((1, [(1, 2), (2, 4), (4, 8), (8, 9)]), (4, [(4, 8), (8, 9)]), (B0, [])):
        levels = []
        PD.divide(a, b, base, levels)
        assert [(k, hi) for k, hi, _ in levels] == want


def test_newton_sizes_short_divisors_stay_at_two_k():
    assert PD.newton_size(1024, 2048, 2) == 2048       # a short divisor: one wrap-free transform of 2k
    assert PD.newton_size(1024, 2048, 1026) == 2048
    assert PD.newton_size(1024, 2048, 1027) == 4096
    assert PD.newton_size(1024, 2048, 2048) == 4096
    assert PD.newton_size(1024, 1500, 1500) == 4096
    assert PD.newton_size(8, 9, 2) == 16


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("na,nb", [(40, 9), (20, 14)])   # m > nb and nb > m
def test_patterns(na, nb, base):
    rng = random.Random(na * nb)
    a, b = case(na, nb, 7)
    divisors = {
        "b0_zero": [0] + b[1:],
        "sparse": [(-5) % R] + [0] * (nb - 2) + [1],            # X^k - c
        "monic": b[:-1] + [1],
        "non_monic": b[:-1] + [R - 2],
    }
    dividends = {
        "random": a,
        "top_two_zero": a[:-2] + [0, 0],
        "zero": [0] * na,
        "above_r": [x + R if x + R < 1 << 256 else x for x in a],
        "tiny": [rng.randrange(3) for _ in range(na)],
    }
    for dn, d in divisors.items():
        for an, x in dividends.items():
            assert PD.divide(x, d, base) == oracle_divide(x, d), (dn, an)


@pytest.mark.parametrize("base", BASES)
def test_exact_divisions_have_a_zero_remainder(base):
    q0, b = case(23, 12, 3)
    a = M.Polynomial(q0).mul_naive(M.Polynomial(b)).coeffs
    q, r = PD.divide(a, b, base)
    assert q == q0 + [0] * (len(q) - len(q0)) and r == [0] * 11
    a[5] = (a[5] + 1) % R
    q, r = PD.divide(a, b, base)
    assert (q, r) == oracle_divide(a, b) and any(r)
