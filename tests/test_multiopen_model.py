"""The big-int model of the two-element multiproof (tests/multiopen_model.py) against itself: honest proofs pass for several r and t,
every single flip fails, the forgery a predictable t allows (the example of include/kzg_mi355x.h) passes with that t and fails with a
fresh one, the regrouped form equals the per-claim sum, chunked weights are the unchunked ones, and the evaluation-form g is the
transform of the coefficient-form g."""
import random

import pytest

from oracle import kzg_model as M
from tests import multiopen_model as MO
from tests import open_eval_model as OE
from tests import verify_eval_batch_model as V

R = MO.R


def make(rng, n_polys, n, count, n_points, identity=False):
    tau = rng.randrange(2, R)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_polys)]
    pts = [rng.randrange(R) for _ in range(n_points)]
    if identity:
        idx, count = None, n_polys
    else:
        idx = [rng.randrange(n_polys) for _ in range(count)]
    zs = [pts[rng.randrange(n_points)] for _ in range(count)]
    commitments = [MO.poly_eval(p, tau) for p in polys]
    return tau, polys, idx, zs, commitments


def fresh_t(rng, zs):
    t = rng.randrange(R)
    while t in zs:
        t = rng.randrange(R)
    return t


def test_honest_proofs_pass_for_several_r_and_t():
    rng = random.Random(1)
    for n_polys, n, count, n_points, identity in ((1, 5, 1, 1, False), (3, 6, 7, 3, False), (4, 4, 4, 2, True), (2, 8, 9, 9, False), (5, 1, 6, 2, False)):
        tau, polys, idx, zs, commitments = make(rng, n_polys, n, count, n_points, identity)
        for r in (1, 2, R - 1, rng.randrange(1, R)):
            for t in (fresh_t(rng, zs), fresh_t(rng, zs)):
                ys, D, pi = MO.prove(polys, idx, zs, r, t, tau)
                assert MO.verdict(tau, commitments, idx, zs, ys, r, t, D, pi)
                # v(t) = g2, and the proof is a plain opening of E - D at (t, g2)
                _, g = MO.commit_coeff(polys, idx, zs, r)
                vt, _ = MO.finish_coeff(polys, idx, zs, r, t, g)
                w, W = MO.poly_weights(zs, idx, n_polys, r, t)
                assert vt == sum(a * b for a, b in zip(w, ys)) % R
                E = sum(a * b for a, b in zip(W, commitments)) % R
                assert V.opening_ok(tau, t, vt, (E - D) % R, pi)


def test_every_single_flip_fails():
    rng = random.Random(2)
    tau, polys, idx, zs, commitments = make(rng, 3, 5, 6, 3)
    r, t = rng.randrange(1, R), fresh_t(rng, zs)
    ys, D, pi = MO.prove(polys, idx, zs, r, t, tau)
    assert MO.verdict(tau, commitments, idx, zs, ys, r, t, D, pi)
    for k in range(len(zs)):
        bad = list(ys)
        bad[k] = (bad[k] + 1) % R
        assert not MO.verdict(tau, commitments, idx, zs, bad, r, t, D, pi)
        bad = list(zs)
        bad[k] = (bad[k] + 1) % R
        assert not MO.verdict(tau, commitments, idx, bad, ys, r, t, D, pi)
        bad = list(idx)
        bad[k] = (bad[k] + 1) % 3
        assert not MO.verdict(tau, commitments, bad, zs, ys, r, t, D, pi)
    for m in range(3):
        bad = list(commitments)
        bad[m] = (bad[m] + 1) % R
        assert not MO.verdict(tau, bad, idx, zs, ys, r, t, D, pi)
    assert not MO.verdict(tau, commitments, idx, zs, ys, r, t, (D + 1) % R, pi)
    assert not MO.verdict(tau, commitments, idx, zs, ys, r, t, D, (pi + 1) % R)
    assert not MO.verdict(tau, commitments, idx, zs, ys, (r + 1) % R or 1, t, D, pi)
    other = (t + 1) % R
    while other in zs:
        other = (other + 1) % R
    assert not MO.verdict(tau, commitments, idx, zs, ys, r, other, D, pi)


def test_predictable_t_lets_one_wrong_claim_pass():
    """the header's example: pi = identity, D = (C - [y'] gs[0])/(t - z)"""
    rng = random.Random(3)
    tau, polys, idx, zs, commitments = make(rng, 1, 6, 1, 1, identity=True)
    z, C = zs[0], commitments[0]
    y_true = MO.poly_eval(polys[0], z)
    y_wrong = (y_true + rng.randrange(1, R)) % R
    for r in (1, rng.randrange(1, R)):
        t = fresh_t(rng, zs)
        D, pi = MO.forge(C, z, y_wrong, t)
        assert MO.verdict(tau, [C], None, [z], [y_wrong], r, t, D, pi)  # the forger knew t
        t2 = fresh_t(rng, zs + [t])
        assert not MO.verdict(tau, [C], None, [z], [y_wrong], r, t2, D, pi)  # t drawn after D
        # and the honest prover has no better answer for the wrong value: its own proof is for the true one
        ys, D2, pi2 = MO.prove(polys, None, [z], r, t2, tau)
        assert ys == [y_true] and MO.verdict(tau, [C], None, [z], ys, r, t2, D2, pi2)
        assert not MO.verdict(tau, [C], None, [z], [y_wrong], r, t2, D2, pi2)


def test_regrouped_form_equals_the_per_claim_sum():
    rng = random.Random(4)
    for n_polys, n, count, n_points in ((3, 6, 10, 3), (2, 5, 7, 7), (4, 3, 9, 1), (2, 1, 4, 2)):
        tau, polys, idx, zs, commitments = make(rng, n_polys, n, count, n_points)
        r = rng.randrange(1, R)
        ys, g = MO.commit_coeff(polys, idx, zs, r)
        for cap in (None, 1, 2, 3, 16):
            assert MO.commit_coeff_regrouped(polys, idx, zs, r, cap) == g
        order, pstart, points, chunks = MO.plan(zs, 2)
        assert sorted(order) == list(range(count)) and len(points) == len(set(zs)) and pstart[-1] == count
        assert all(zs[k] == points[u] for u in range(len(points)) for k in order[pstart[u]:pstart[u + 1]])
        assert [c for u0, u1 in chunks for c in range(u0, u1)] == list(range(len(points))) and all(u1 - u0 <= 2 for u0, u1 in chunks)


def test_chunked_weights_equal_the_unchunked_ones():
    rng = random.Random(5)
    tau, polys, idx, zs, commitments = make(rng, 4, 4, 15, 5)
    r, t = rng.randrange(1, R), fresh_t(rng, zs)
    whole = MO.poly_weights(zs, idx, 4, r, t)
    assert whole[0] == [pow(r, k, R) * pow((t - zs[k]) % R, R - 2, R) % R for k in range(15)]
    ys, D, pi = MO.prove(polys, idx, zs, r, t, tau)
    for chunk in (1, 2, 4, 7, 14, 15, 16):
        assert MO.poly_weights(zs, idx, 4, r, t, chunk) == whole
        assert MO.verdict(tau, commitments, idx, zs, ys, r, t, D, pi, chunk)


@pytest.mark.parametrize("d", [1, 2, 4, 8, 64])
def test_evaluation_form_g_is_the_transform_of_coefficient_form_g(d):
    rng = random.Random(60 + d)
    n_polys = 3
    w = M.compute_omega(d)[2]
    polys = [[rng.randrange(R) for _ in range(d)] for _ in range(n_polys)]
    evals = [[MO.poly_eval(p, pow(w, i, R)) for i in range(d)] for p in polys]
    on = [pow(w, rng.randrange(d), R) for _ in range(2)]
    pts = [rng.randrange(R), rng.randrange(R)] + on
    zs = [pts[k % len(pts)] for k in range(9)]
    idx = [rng.randrange(n_polys) for _ in range(9)]
    r = rng.randrange(1, R)
    ys_c, g_c = MO.commit_coeff(polys, idx, zs, r)
    ys_e, g_e = MO.commit_eval(evals, idx, zs, r)
    assert ys_c == ys_e
    assert g_e == [MO.poly_eval(g_c, pow(w, i, R)) for i in range(d)]
    assert MO.interpolate(g_e) == g_c + [0]
    for t in (fresh_t(rng, zs), pow(w, 1, R) if pow(w, 1, R) not in zs else fresh_t(rng, zs)):  # off the domain, on it
        vt_c, q_c = MO.finish_coeff(polys, idx, zs, r, t, g_c)
        v, vt_e, q_e = MO.finish_eval(evals, idx, zs, r, t, g_e)
        assert vt_c == vt_e
        assert q_e == [MO.poly_eval(q_c, pow(w, i, R)) for i in range(d)]
    # the plan puts the points of the domain behind the others, and only the others into chunks
    order, pstart, points, chunks = MO.plan(zs, 1, on=lambda z: OE.domain_index(d, z) is not None)
    n_off = len(chunks)
    assert all(OE.domain_index(d, z) is None for z in points[:n_off]) and all(OE.domain_index(d, z) is not None for z in points[n_off:])
