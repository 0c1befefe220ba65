"""CPU checks of the model of kzg_verify_eval_batch (tests/verify_eval_batch_model.py): the combined equation accepts honest openings
and rejects every single tampering, the weights matter (a compensating pair passes at r = 1 only), the weights continue across chunk
boundaries, the verdict is all(per-opening check) on mixes of good and bad openings -- and the call exists in the header and the
binding."""
import os
import random

from tests import verify_eval_batch_model as E

R = E.R
TAU = 0x7A05EED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def polys_of(rng):
    return [[rng.randrange(R) for _ in range(n)] for n in (7, 2, 4)]


def call_of(seed=0, count=7):
    """(xs, ys, commitments, idx, witnesses) as scalars: three polynomials of fewer than 8 coefficients opened at `count` points; every
    commitment is named, opening count - 1 repeats opening 0"""
    rng = random.Random(seed)
    polys = polys_of(rng)
    xs, ys, idx, ws = [], [], [], []
    for k in range(count):
        m, x = (idx[0], xs[0]) if k == count - 1 else (k % 3 if k < 3 else rng.randrange(3), rng.randrange(R))
        y, q = E.witness_at(polys[m], x, TAU)
        xs.append(x)
        ys.append(y)
        idx.append(m)
        ws.append(q)
    return xs, ys, [E.poly_eval(p, TAU) for p in polys], idx, ws


def test_honest_openings_pass_for_several_r():
    xs, ys, C, idx, ws = call_of()
    assert all(E.opening_ok(TAU, x, y, C[m], q) for x, y, m, q in zip(xs, ys, idx, ws))
    rng = random.Random(1)
    for r in [1, 2, R - 1] + [rng.randrange(1, R) for _ in range(4)]:
        assert E.verdict(TAU, r, xs, ys, C, idx, ws), r
    # one commitment per opening: idx None
    assert E.verdict(TAU, 5, xs, ys, [C[m] for m in idx], None, ws)


def test_every_single_tampering_fails():
    xs, ys, C, idx, ws = call_of()
    r = random.Random(2).randrange(2, R)
    for k in range(len(xs)):
        for which in range(3):
            a = [list(xs), list(ys), list(ws)]
            a[which][k] = (a[which][k] + 1) % R
            assert not E.verdict(TAU, r, a[0], a[1], C, idx, a[2]), (which, k)
        bad = list(idx)
        bad[k] = (bad[k] + 1) % 3
        assert not E.verdict(TAU, r, xs, ys, C, bad, ws), ("index", k)
    for m in range(3):
        bad = list(C)
        bad[m] = (bad[m] + 1) % R
        assert not E.verdict(TAU, r, xs, ys, bad, idx, ws), ("commitment", m)


def test_compensating_pair_at_a_common_x_passes_at_r_1_only():
    xs, ys, C, idx, ws = call_of()
    ka, kb = 1, 4
    xs[kb] = xs[ka]  # openings of two polynomials at one point
    ys[kb], ws[kb] = E.witness_at(polys_of(random.Random(0))[idx[kb]], xs[kb], TAU)  # call_of's polynomials
    assert E.verdict(TAU, 2, xs, ys, C, idx, ws)
    D = 0xD1FF
    ws[ka], ws[kb] = (ws[ka] + D) % R, (ws[kb] - D) % R
    assert not E.opening_ok(TAU, xs[ka], ys[ka], C[idx[ka]], ws[ka]) and not E.opening_ok(TAU, xs[kb], ys[kb], C[idx[kb]], ws[kb])
    assert E.verdict(TAU, 1, xs, ys, C, idx, ws)  # the weights are all 1: the errors cancel
    assert not E.verdict(TAU, 2, xs, ys, C, idx, ws)


def test_chunked_runs_equal_the_unchunked_run():
    xs, ys, C, idx, ws = call_of()
    r = random.Random(3).randrange(2, R)
    whole = E.scalars(r, xs, ys, idx, 3)
    assert whole[0] == [pow(r, k, R) for k in range(7)]
    assert whole[3] == sum(pow(r, k, R) * y for k, y in enumerate(ys)) % R
    for chunk in (1, 3):
        assert E.scalars(r, xs, ys, idx, 3, chunk) == whole
        assert E.verdict(TAU, r, xs, ys, C, idx, ws, chunk)
        assert E.scalars(r, xs, ys, None, 7, chunk) == E.scalars(r, xs, ys, None, 7)
    assert E.scalars(r, xs, ys, None, 7)[2] == whole[0]  # without indices c_k = rho_k


def test_verdict_is_all_of_the_per_opening_checks_on_random_mixes():
    # fixed seeds; a false accept of the combination has probability about count / |Fr|
    seen = set()
    for seed in range(40):
        rng = random.Random(1000 + seed)
        xs, ys, C, idx, ws = call_of(seed, count=3 + seed % 6)
        for k in range(len(xs)):
            if rng.random() < 0.2:
                [xs, ys, ws][rng.randrange(3)][k] += 1
        each = [E.opening_ok(TAU, x, y, C[m], q) for x, y, m, q in zip(xs, ys, idx, ws)]
        r = rng.randrange(1, R)
        assert E.verdict(TAU, r, xs, ys, C, idx, ws) == all(each), seed
        assert E.verdict(TAU, r, xs, ys, C, idx, ws, chunk=2) == all(each), seed
        seen.add(all(each))
    assert seen == {True, False}


def test_the_call_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    binding = open(os.path.join(ROOT, "kzg_amd", "_lib.py")).read()
    assert "int kzg_verify_eval_batch(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs," in header
    assert '"kzg_verify_eval_batch":' in binding
