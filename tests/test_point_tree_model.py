"""CPU checks of the point-tree model (tests/point_tree_model.py) against oracle.kzg_model's SubProductTree / Polynomial: product,
values, linear_mod_combination and interpolation for every k from 1 to 40 at forced small leaves and at the kernels' own leaf, around
the leaf and the in-LDS transform bound, with 0, 1 and r - 1 among the points, repeated points and coefficients >= r."""
import random

import pytest

from oracle import kzg_model as M
from tests import point_tree_model as PT

R = M.R


def points(rng, k):
    xs = [rng.randrange(R) for _ in range(k)]
    for pos, v in ((1, 0), (2, 1), (3, R - 1)):
        if k > pos + 1:
            xs[pos] = v
    return xs


def ns_for(k, K):
    return sorted({v for v in (1, k - 1, k, k + 1, K - 1, K, K + 1, 2 * K + 1, 3 * K + 5) if v >= 1})


def horner(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def test_constants_are_read_from_the_kernel_source():
    assert PT.LEAF == 16 and PT.SMALL == 1024 and PT.CHUNK_ELEMS == 1 << 21
    assert PT.constant("PT_T") == 256


@pytest.mark.parametrize("leaf", [1, 4, PT.LEAF])
@pytest.mark.parametrize("k", list(range(1, 41)) + [63, 64, 65])
def test_model_against_the_oracle(k, leaf):
    rng = random.Random(100 * k + leaf)
    xs = points(rng, k)
    t = PT.Tree(xs, leaf)
    ot = M.SubProductTree.new_from_points(xs)
    assert t.M == ot.product.coeffs[: k + 1] and t.K == PT.next_pow2(k) and t.distinct
    for n in ns_for(k, t.K):
        p = [rng.randrange(R) for _ in range(n)]
        if n > 1:
            p[n // 2] += R  # a coefficient >= r counts as its residue
        assert t.eval(p) == [M.Polynomial(p).eval(x) for x in xs], (k, n)
    cs = [rng.randrange(R) + (R if i == 0 else 0) for i in range(k)]
    ys = [rng.randrange(R) for _ in range(k)]
    if k == 1:
        assert t.combine(cs) == [cs[0] % R] and t.interpolate(ys) == ys  # the constant; the X + (y - x) quirk stays in the mirrors
        return
    want = ot.linear_mod_combination([c % R for c in cs])
    assert t.combine(cs) == (want.coeffs + [0] * k)[:k]
    want = M.Polynomial.lagrange_interpolation(xs, ys)
    assert t.interpolate(ys) == (want.coeffs + [0] * k)[:k]
    assert t.den == [horner([t.M[i] * i % R for i in range(1, k + 1)], x) for x in xs]


@pytest.mark.parametrize("leaf", [1, PT.LEAF])
def test_repeated_points(leaf):
    xs = [5, 9, 5, 0, 0, R - 1, 7]
    t = PT.Tree(xs, leaf)
    rng = random.Random(3)
    p = [rng.randrange(R) for _ in range(19)]
    assert t.eval(p) == [M.Polynomial(p).eval(x) for x in xs]
    assert not t.distinct and [bool(v) for v in t.den] == [False, True, False, False, False, True, True]
    assert t.M == M.SubProductTree.new_from_points(xs).product.coeffs[:8]
    cs = [rng.randrange(R) for _ in xs]
    assert t.combine(cs) == (M.SubProductTree.new_from_points(xs).linear_mod_combination(cs).coeffs + [0] * 7)[:7]


def test_a_real_point_zero_beside_the_dummy_points():
    """the derivative is the true M's: the padded root's vanishes at x = 0"""
    xs = [0, 3, 4]
    t = PT.Tree(xs, 1)
    assert t.distinct and t.den[0] == 12 and t.interpolate([1, 1, 1]) == [1, 0, 0]


@pytest.mark.parametrize("k", [PT.LEAF - 1, PT.LEAF, PT.LEAF + 1, 2 * PT.LEAF + 1, PT.SMALL - 1, PT.SMALL, PT.SMALL + 1])
def test_around_the_kernels_boundaries_at_the_default_leaf(k):
    rng = random.Random(k)
    xs = points(rng, k)
    t = PT.Tree(xs)
    prod = [1]
    for x in xs:  # the plain product, factor by factor
        prod = [((prod[i - 1] if i else 0) - x * (prod[i] if i < len(prod) else 0)) % R for i in range(len(prod) + 1)]
    assert t.M == prod and t.distinct
    for n in (1, k, t.K + 1):
        p = [rng.randrange(R) for _ in range(n)]
        got = t.eval(p)
        for i in rng.sample(range(k), 8) + [1, 2, 3]:
            assert got[i] == horner(p, xs[i]), (k, n, i)
    ys = [rng.randrange(R) for _ in range(k)]
    f = t.interpolate(ys)
    for i in rng.sample(range(k), 8) + [1, 2, 3]:
        assert horner(f, xs[i]) == ys[i]
    cs = [0] * k
    cs[k // 3], cs[k - 1] = 5, 7  # two terms of the combination: 5 M / (X - x_a) + 7 M / (X - x_b), checked at a few points
    comb = t.combine(cs)
    for z in (2, R - 3):
        mz = horner(t.M, z)
        assert horner(comb, z) == (5 * mz * pow(z - xs[k // 3], -1, R) + 7 * mz * pow(z - xs[k - 1], -1, R)) % R


def test_plan_bytes():
    assert PT.Tree([1, 2, 3], 1).plan_bytes() == 32 * (3 * 4 + 2 * 8 + 8 + 8 + 8 + 3 + 4)
    assert PT.Tree([7], 16).plan_bytes() == 32 * (1 + 0 + 2 + 2 + 2 + 1 + 2)
    assert PT.Tree(list(range(40)), 16).plan_bytes() == 32 * (7 * 64 + 2 * 128 + 6 * 64 + 40 + 41)
    assert PT.chunk_units(1 << 13) == 256 and PT.chunk_units(1 << 22) == 1
