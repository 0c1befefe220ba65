"""CPU checks of the model of kzg_verify_cosets_batch (tests/verify_cosets_batch_model.py): the combined equation accepts honest cells
and rejects every single tampering, the weights matter (a compensating pair passes at r = 1 only), `a` is the weighted sum of the
interpolants, and the weights continue across chunk boundaries."""
import random

import pytest

from oracle import kzg_model as M
from tests import verify_cosets_batch_model as B
from tests import verify_cosets_model as V

R = M.R
SHAPES = [(6, 2), (4, 4), (5, 0)]
TAU = 0x7A05EED


def call_of(log_n, log_l, count=40, seed=0):
    """(commitments, idx, ids, cells, proofs) as scalars: `count` honest cells of three polynomials of different lengths, in random
    order, with duplicate (commitment, coset) pairs"""
    rng = random.Random(100 * log_n + log_l + seed)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    polys = [[rng.randrange(R) for _ in range(max(1, N - 3 * m))] for m in range(3)]
    idx, ids, cells, proofs = [], [], [], []
    for k in range(count):
        m, i = (idx[0], ids[0]) if k == count - 1 else (rng.randrange(3), rng.randrange(K))  # at least one duplicate pair
        vals = [V.poly_eval(polys[m], x) for x in V.coset_points(i, log_n, log_l)]
        q = V.quotient_at(polys[m], V.interpolant(vals, i, log_n, log_l), i, log_n, log_l, TAU)
        assert q is not None
        idx.append(m)
        ids.append(i)
        cells.append(vals)
        proofs.append(q)
    return [V.poly_eval(p, TAU) for p in polys], idx, ids, cells, proofs


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_honest_cells_are_accepted_and_every_single_tampering_is_rejected(log_n, log_l):
    C, idx, ids, cells, proofs = call_of(log_n, log_l)
    rng = random.Random(5)
    r = rng.randrange(2, R)
    assert len(set(zip(idx, ids))) < len(ids)
    assert all(V.verdict(TAU, C[m], q, v, i, log_n, log_l) for m, i, v, q in zip(idx, ids, cells, proofs))
    assert B.verdict(TAU, r, C, idx, ids, cells, proofs, log_n, log_l)
    assert B.verdict(TAU, 1, C, idx, ids, cells, proofs, log_n, log_l)
    for k in range(len(ids)):
        p = list(proofs)
        p[k] = (p[k] + 1) % R
        assert not B.verdict(TAU, r, C, idx, ids, cells, p, log_n, log_l), ("proof", k)
        c = [list(v) for v in cells]
        c[k][rng.randrange(1 << log_l)] = (c[k][0] + 1) % R
        assert not B.verdict(TAU, r, C, idx, ids, c, proofs, log_n, log_l), ("value", k)
    for m in set(idx):
        bad = list(C)
        bad[m] = (bad[m] + 1) % R
        assert not B.verdict(TAU, r, bad, idx, ids, cells, proofs, log_n, log_l), ("commitment", m)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_compensating_pair_passes_at_r_1_only(log_n, log_l):
    C, idx, ids, cells, proofs = call_of(log_n, log_l)
    rng = random.Random(6)
    r = rng.randrange(2, R)
    by = {}
    for k, i in enumerate(ids):
        by.setdefault(i, []).append(k)
    ka, kb = next(v for v in by.values() if len(v) >= 2)[:2]
    D = rng.randrange(1, R)
    p = list(proofs)
    p[ka], p[kb] = (p[ka] + D) % R, (p[kb] - D) % R  # pi_a + D and pi_b - D in one coset: P1 and P2 of r = 1 do not move
    assert B.verdict(TAU, 1, C, idx, ids, cells, p, log_n, log_l)
    assert not B.verdict(TAU, r, C, idx, ids, cells, p, log_n, log_l)
    assert not V.verdict(TAU, C[idx[ka]], p[ka], cells[ka], ids[ka], log_n, log_l)
    assert not V.verdict(TAU, C[idx[kb]], p[kb], cells[kb], ids[kb], log_n, log_l)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_a_is_the_weighted_sum_of_the_interpolants_and_chunks_continue_the_weights(log_n, log_l):
    C, idx, ids, cells, proofs = call_of(log_n, log_l, count=17, seed=1)
    r = random.Random(7).randrange(2, R)
    l = 1 << log_l
    a, c, rho, rho_h = B.scalars(r, idx, ids, cells, len(C), log_n, log_l)
    assert rho == [pow(r, k, R) for k in range(17)] == B.weights(r, 17)
    inter = [V.interpolant(v, i, log_n, log_l) for v, i in zip(cells, ids)]
    assert a == [sum(p * rk[j] for p, rk in zip(rho, inter)) % R for j in range(l)]
    assert c == [sum(p for p, m in zip(rho, idx) if m == mm) % R for mm in range(len(C))]
    w = V.omega(log_n)
    assert rho_h == [p * pow(w, i * l, R) % R for p, i in zip(rho, ids)]
    # chunks of 5 (17 = 5 + 5 + 5 + 2) and of 1: the same scalars, the same verdict
    assert B.weights(r, 5, 10) == rho[10:15]
    for chunk in (5, 1):
        assert B.scalars(r, idx, ids, cells, len(C), log_n, log_l, chunk) == (a, c, rho, rho_h)
        assert B.verdict(TAU, r, C, idx, ids, cells, proofs, log_n, log_l, chunk)
    # weights that restarted in every chunk would be another (and unsound) combination
    restarted = [x for k0 in range(0, 17, 5) for x in B.weights(r, min(5, 17 - k0))]
    assert restarted != rho


def test_bindings_exist():
    import kzg_amd
    lib = kzg_amd.load()
    assert hasattr(lib, "kzg_verify_cosets_batch")
    assert lib.kzg_verify_cosets_batch.restype is not None and len(lib.kzg_verify_cosets_batch.argtypes) == 14
    for name in ("verify_batch", "verify_with_fallback"):
        assert hasattr(kzg_amd.CosetVerifier, name)
    assert hasattr(kzg_amd.KZGVerifier, "verify_cosets_batch")
