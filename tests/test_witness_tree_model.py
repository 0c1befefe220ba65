"""The big-int model of kzg_msm_g2_bucket (tests/witness_tree_model.py) against the oracle's G2 arithmetic: the digits recompose to
the scalar, no digit leaves [-128, 128], and the slice / slot / window / bucket sum is G2Projective::multi_exp."""
import random

import pytest

from oracle import kzg_model as M
from oracle import pairing_model as P
from tests import witness_tree_model as WT

X80 = int.from_bytes(b"\x80" * 32, "little")
X7F = int.from_bytes(b"\x7f" * 32, "little")


def test_digits_recompose_to_the_scalar():
    rng = random.Random(11)
    for k in [0, 1, M.R - 1, X80 % M.R, X7F % M.R, X7F, 127, 128, 129, 255, 256, (1 << 255) - 1] + [rng.randrange(M.R) for _ in range(200)]:
        ds = WT.digits(k)
        assert len(ds) == WT.W and all(-WT.D <= d <= WT.D for d in ds), hex(k)
        assert WT.recompose(ds) == k, hex(k)


def test_the_top_window_keeps_its_carry_for_every_reduced_scalar():
    # r < 2^255: the top byte of a reduced scalar is at most 0x73, so its digit is at most 0x73 + 1 and nothing leaves window 31
    assert M.R >> 248 == 0x73
    assert WT.digit(M.R - 1, WT.W - 1) <= 0x74
    # an unreduced value of 0x80 bytes would not fit: its top digit is negative and the sum is short of 2^256
    assert WT.recompose(WT.digits(X80)) == X80 - (1 << 256)


@pytest.mark.parametrize("S,slots,n", [(4, 2, 0), (4, 2, 1), (4, 2, 3), (4, 2, 4), (4, 2, 5), (4, 2, 8), (4, 2, 9), (4, 2, 19), (2, 3, 13), (2048, 16, 6)])
def test_bucket_sum_is_the_multi_exp(S, slots, n):
    rng = random.Random(1000 * S + 10 * slots + n)
    hs = P.setup_g2(rng.getrandbits(64), max(n, 1))[:n]
    sc = [rng.randrange(M.R) for _ in range(n)]
    if n > 2:
        sc[0], sc[1] = M.R - 1, X80 % M.R
    if n > 4:
        sc[3], sc[4] = 0, 1
    assert WT.msm_g2_bucket(hs, sc, S, slots) == P.g2_multi_exp(hs, sc)


@pytest.mark.parametrize("k,n", [(1, 4), (3, 8), (4, 8), (5, 8), (5, 5), (5, 3), (7, 8)])
def test_division_by_the_product_leaves_the_interpolant(k, n):
    rng = random.Random(10 * k + n)
    xs = rng.sample(range(1, 1 << 30), k)
    p = [rng.randrange(M.R) for _ in range(n)]
    m = WT.product(xs)
    assert len(m) == k + 1 and m[k] == 1 and all(WT.poly_eval(m, x) == 0 for x in xs)
    assert M.Polynomial(list(m)).slice_coeffs() == M.SubProductTree.new_from_points(xs).product.slice_coeffs()
    q, r = WT.divide(p, m)
    assert len(r) == k and len(q) == max(n - k, 0)
    z = rng.randrange(M.R)  # p = q M + r as polynomials: equal at a random point, degrees bounded
    assert WT.poly_eval(p, z) == (WT.poly_eval(q, z) * WT.poly_eval(m, z) + WT.poly_eval(r, z)) % M.R
    ys = [WT.poly_eval(p, x) for x in xs]
    assert r == WT.interpolate(xs, ys)  # r is the interpolant through (x_i, p(x_i)), zero-padded to k
    if n <= k:
        assert q == [] and r == p + [0] * (k - n)
    if k >= 2:
        ref = M.Polynomial.lagrange_interpolation(xs, ys)
        assert r == (ref.slice_coeffs() + [0] * k)[:k]


@pytest.fixture(scope="module")
def params8():
    return P.setup(0x1234567, 8)


@pytest.mark.parametrize("k", [3, 4, 5])
def test_verifier_equation_against_the_oracle_models(params8, k):
    n = 8
    rng = random.Random(k)
    xs = rng.sample(range(1, 1 << 30), k)
    coeffs = [rng.randrange(M.R) for _ in range(n)]
    poly = M.Polynomial(list(coeffs))
    ys = [poly.eval(x) for x in xs]
    ref_r, ref_w = M.KZGProver(params8).create_witness_batched(poly, xs, ys)
    commitment = M.KZGProver(params8).commit(poly)
    # the model's opening is the reference's: the same remainder, the same witness
    q, r = WT.divide(coeffs, WT.product(xs))
    assert r == (ref_r.slice_coeffs() + [0] * k)[:k]
    assert M.g1_multi_exp(params8.gs[:len(q)], q) == ref_w
    ver = P.KZGVerifier(params8)
    assert WT.verify_eval_tree(params8.gs, params8.hs, xs, r, commitment, ref_w, 4, 1) is True
    assert ver.verify_eval_batched(xs, commitment, ref_w, ref_r) is True
    if k == 4:  # a tampered remainder, a tampered witness, a shifted point set: both verifiers say no
        bent = [(r[0] + 1) % M.R] + r[1:]
        assert WT.verify_eval_tree(params8.gs, params8.hs, xs, bent, commitment, ref_w, 4, 1) is False
        assert ver.verify_eval_batched(xs, commitment, ref_w, M.Polynomial(list(bent))) is False
        assert WT.verify_eval_tree(params8.gs, params8.hs, xs, r, commitment, M.g1_add(ref_w, params8.gs[0]), 2, 2) is False
        assert WT.verify_eval_tree(params8.gs, params8.hs, [x + 1 for x in xs], r, commitment, ref_w, 4, 1) is False


def test_equal_and_opposite_points_and_lifted_scalars():
    H = P.G2
    pts = [H, P.g2_neg(H), H, None, H, P.g2_neg(H), H]
    sc = [5, 5, 5, 9, M.R - 1, 1, 5 + M.R]  # one bucket holds H, -H, H and H again (5 + r counts as 5)
    want = P.g2_multi_exp(pts, [s % M.R for s in sc])
    assert WT.msm_g2_bucket(pts, sc, 4, 1) == want == P.g2_mul(H, (5 - 5 + 5 + (M.R - 1) - 1 + 5) % M.R)
