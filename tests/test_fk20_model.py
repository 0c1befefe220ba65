"""CPU checks of the FK20 layout (tests/fk20_model.py) and of the GLV constants of kzg_amd/csrc/g1ntt.hip."""
import os
import random
import re

import pytest

from oracle import kzg_model as M
from tests import fk20_model as F


@pytest.mark.parametrize("N", [1, 2, 4, 8, 16, 32, 64])
def test_layout_matches_direct_quotients(N):
    rng = random.Random(1000 + N)
    tau = rng.randrange(1, M.R)
    for n in sorted({1, max(1, N // 2 - 1), max(1, N - 1), N}):
        coeffs = [rng.randrange(M.R) for _ in range(n)]
        assert F.fk20_model(coeffs, N, tau) == F.direct_witnesses(coeffs, N, tau), (N, n)


@pytest.mark.parametrize("N", [4, 16])
def test_short_srs_is_exact(N):
    # points past len(srs) count as the identity: exact whenever n - 1 <= len(srs)
    rng = random.Random(7 + N)
    tau = rng.randrange(1, M.R)
    for n in range(1, N + 1):
        coeffs = [rng.randrange(M.R) for _ in range(n)]
        assert F.fk20_model(coeffs, N, tau, srs_len=n - 1) == F.direct_witnesses(coeffs, N, tau), (N, n)


def test_chunk_rules_match_the_source():
    # the GPU chunk tests pick their shapes (a second chunk, a ragged last one, several residue slices) with F.chunk_size and
    # F.coset_slices; if g1ntt.hip changes either rule, this fails instead of those tests quietly covering less
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "kzg_amd", "csrc", "g1ntt.hip")) as f:
        src = f.read()
    const = dict(re.findall(r"constexpr \w+ (\w+) = ([^;]+);", src))
    assert (const["FK20_CHUNK_POINTS"], const["FK20_MAX_CHUNK"]) == ("(size_t)1 << 21", "4096")
    assert const["COSET_TARGET_THREADS"] == "(size_t)1 << 17"
    # fk20_run, the one chunk loop behind kzg_witness_all_* and kzg_witness_cosets_*
    assert src.count("chunk = std::max<size_t>(1, std::min(FK20_MAX_CHUNK, FK20_CHUNK_POINTS / (2 * N)));") == 1
    assert "while (S < l && batch * S * two < COSET_TARGET_THREADS) S *= 2;" in src
    assert "const size_t S = coset_slices(l, two, B0);" in src
    assert [F.chunk_size(1 << k) for k in (0, 6, 12, 14, 16, 20, 22)] == [4096, 4096, 256, 64, 16, 1, 1]
    assert [F.coset_slices(64, 512, b) for b in (64, 2, 1)] == [4, 64, 64]
    assert F.coset_slices(64, 2 << 14, 1) == 4    # 2^20 / l = 64


def test_glv_constants():
    lam = F.GLV_LAMBDA
    assert lam * lam + lam + 1 == M.R
    assert (lam * lam + lam + 1) % M.R == 0
    assert pow(F.GLV_BETA, 3, M.Q) == 1 and F.GLV_BETA != 1


EDGE = [0, 1, F.GLV_LAMBDA - 1, F.GLV_LAMBDA, F.GLV_LAMBDA + 1, M.R - 1]


def test_glv_split_and_digits():
    rng = random.Random(5)
    for k in EDGE + [rng.randrange(M.R) for _ in range(200)]:
        k1, k2 = F.glv_split(k)
        assert k1 + k2 * F.GLV_LAMBDA == k
        assert 0 <= k1 < 1 << 128 and 0 <= k2 < 1 << 128
        for v in (k1, k2):
            digs, top = F.signed_digits(v, 32)
            assert all(-8 <= d <= 7 for d in digs) and top in (0, 1)
            assert sum(d << (4 * i) for i, d in enumerate(digs)) + (top << 128) == v
        digs, top = F.signed_digits(k, 64)  # the point-wise products: no carry out below r
        assert top == 0 and sum(d << (4 * i) for i, d in enumerate(digs)) == k


def test_endomorphism_is_lambda():
    G = M.setup_g1(1, 1)[0]
    rng = random.Random(9)
    for P in (G, M.g1_mul(G, rng.randrange(1, M.R))):
        phi = (P[0] * F.GLV_BETA % M.Q, P[1])
        assert M.g1_is_on_curve(phi)
        assert M.g1_mul(P, F.GLV_LAMBDA) == phi
        # the other non-trivial cube root of unity belongs to the other eigenvalue
        assert M.g1_mul(P, F.GLV_LAMBDA) != (P[0] * F.GLV_BETA * F.GLV_BETA % M.Q, P[1])
