"""The big-int model of the folded opening and its verifier (tests/open_fold_model.py) against itself and against the per-opening
check: honest folded openings pass for every gamma and r, one wrong value fails, the cancellation a predictable gamma allows (the
example of include/kzg_mi355x.h) passes with that gamma and fails with a random one, and the chunked weights are the unchunked ones."""
import random

from tests import open_fold_model as F
from tests import verify_eval_batch_model as V

R = F.R


def make(rng, groups, t, n, shared=False):
    """groups x t random polynomials of n coefficients, points and challenges; with `shared` every group opens the SAME t polynomials
    (at its own point) and names them through indices"""
    tau = rng.randrange(2, R)
    base = [[rng.randrange(R) for _ in range(n)] for _ in range(t)]
    polys = [base if shared else [[rng.randrange(R) for _ in range(n)] for _ in range(t)] for _ in range(groups)]
    zs = [rng.randrange(R) for _ in range(groups)]
    gammas = [rng.randrange(1, R) for _ in range(groups)]
    ys, pis = [], []
    for g in range(groups):
        y, pi = F.open_fold(polys[g], zs[g], gammas[g], tau)
        ys += y
        pis.append(pi)
    if shared:
        commitments, idx = [F.poly_eval(p, tau) for p in base], [i for _ in range(groups) for i in range(t)]
    else:
        commitments, idx = [F.poly_eval(p, tau) for grp in polys for p in grp], None
    return tau, polys, zs, gammas, ys, pis, commitments, idx


def test_fold_is_the_weighted_sum_and_pieces_do_not_change_it():
    rng = random.Random(1)
    for t in (1, 2, 3, 17, 33):
        vecs = [[rng.randrange(R) for _ in range(5)] for _ in range(t)]
        for gamma in (1, 2, R - 1, rng.randrange(1, R)):
            want = [sum(pow(gamma, i, R) * vecs[i][j] for i in range(t)) % R for j in range(5)]
            assert F.fold(vecs, gamma) == want
            for piece in (1, 2, 16):
                assert F.fold_pieces(vecs, gamma, piece) == want
    # values beyond the modulus count as their residue
    assert F.fold([[R + 5], [(1 << 256) - 1]], 3) == [(5 + 3 * (((1 << 256) - 1) % R)) % R]


def test_honest_folded_openings_pass_for_several_gamma_and_r():
    rng = random.Random(2)
    for groups, t, shared in ((1, 1, False), (1, 4, False), (3, 3, False), (5, 2, True)):
        tau, polys, zs, gammas, ys, pis, commitments, idx = make(rng, groups, t, 6, shared)
        for r in (1, 2, R - 1, rng.randrange(1, R)):
            assert F.verdict(tau, r, gammas, t, zs, ys, commitments, idx, pis)
        # the folded witness is a plain opening of the folded commitment: the per-opening check of kzg_verify_eval
        for g in range(groups):
            cs = commitments[:t] if shared else commitments[g * t:(g + 1) * t]
            CF = F.fold([[c] for c in cs], gammas[g])[0]
            yF = F.fold([[y] for y in ys[g * t:(g + 1) * t]], gammas[g])[0]
            assert V.opening_ok(tau, zs[g], yF, CF, pis[g])
    # another gamma at the verifier than at the prover fails
    tau, polys, zs, gammas, ys, pis, commitments, idx = make(rng, 2, 3, 6)
    assert not F.verdict(tau, 7, [gammas[0], (gammas[1] + 1) % R or 1], 3, zs, ys, commitments, idx, pis)


def test_a_single_wrong_value_commitment_witness_or_point_fails():
    rng = random.Random(3)
    tau, polys, zs, gammas, ys, pis, commitments, idx = make(rng, 3, 4, 5)
    r = rng.randrange(1, R)
    for k in range(len(ys)):
        bad = list(ys)
        bad[k] = (bad[k] + 1) % R
        assert not F.verdict(tau, r, gammas, 4, zs, bad, commitments, idx, pis)
    bad = list(commitments)
    bad[5] = (bad[5] + 1) % R
    assert not F.verdict(tau, r, gammas, 4, zs, ys, bad, idx, pis)
    bad = list(pis)
    bad[1] = (bad[1] + 1) % R
    assert not F.verdict(tau, r, gammas, 4, zs, ys, commitments, idx, bad)
    bad = list(zs)
    bad[2] = (bad[2] + 1) % R
    assert not F.verdict(tau, r, gammas, 4, bad, ys, commitments, idx, pis)


def test_predictable_gamma_lets_wrong_values_cancel():
    """the header's example: y_0 + D and y_1 - D / gamma have the fold of the true values"""
    rng = random.Random(4)
    tau, polys, zs, gammas, ys, pis, commitments, idx = make(rng, 1, 2, 8)
    for gamma in (1, rng.randrange(2, R)):
        true_ys, pi = F.open_fold(polys[0], zs[0], gamma, tau)
        D = rng.randrange(1, R)
        forged = [(true_ys[0] + D) % R, (true_ys[1] - D * pow(gamma, R - 2, R)) % R]
        assert forged[0] != true_ys[0] and forged[1] != true_ys[1]
        # the forger knew gamma: the honest witness passes with two wrong values
        assert F.verdict(tau, 1, [gamma], 2, zs, forged, commitments, None, [pi])
        # a gamma drawn after the values were claimed: the prover's best witness for it does not pass
        fresh = rng.randrange(2, R)
        while fresh == gamma:
            fresh = rng.randrange(2, R)
        _, pi2 = F.open_fold(polys[0], zs[0], fresh, tau)
        assert not F.verdict(tau, 1, [fresh], 2, zs, forged, commitments, None, [pi2])
        assert F.verdict(tau, 1, [fresh], 2, zs, true_ys, commitments, None, [pi2])


def test_chunked_weights_equal_the_unchunked_ones():
    rng = random.Random(5)
    groups, t = 5, 3
    gammas = [rng.randrange(1, R) for _ in range(groups)]
    r = rng.randrange(1, R)
    whole = F.weights(r, gammas, t)
    assert whole == [pow(r, g, R) * pow(gammas[g], i, R) % R for g in range(groups) for i in range(t)]
    for chunk in (1, 2, 4, 7, 15, 16):
        parts = []
        for k0 in range(0, groups * t, chunk):
            parts += F.weights(r, gammas, t, k0, min(chunk, groups * t - k0))
        assert parts == whole
    tau, polys, zs, gammas, ys, pis, commitments, idx = make(rng, groups, t, 4, shared=True)
    ref = F.scalars(r, gammas, t, zs, ys, idx, len(commitments))
    for chunk in (1, 4, 7):
        assert F.scalars(r, gammas, t, zs, ys, idx, len(commitments), chunk) == ref
        assert F.verdict(tau, r, gammas, t, zs, ys, commitments, idx, pis, chunk)
