"""CPU checks of the recovery model (tests/recover_model.py): the six steps of kzg_recover_cosets against the original polynomial,
the consistency criterion, and the padded product tree of kzg_amd/csrc/recover.hip against the plain product."""
import ctypes
import os
import random
import re

import pytest

from oracle import kzg_model as M
from tests import fk20_model as F
from tests import recover_model as RM

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = RM.LEAF

SHAPES = [(log_n, log_l) for log_n in range(0, 7) for log_l in range(0, log_n + 1)]


def ns_for(l, known):
    return sorted({v for v in (1, l - 1, l, l + 1, known * l) if 1 <= v <= known * l})


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_six_steps_recover_the_polynomial(log_n, log_l):
    rng = random.Random(1000 * log_n + log_l)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    for m in range(K):  # 0 .. the largest m the precondition allows (known >= 1)
        known = K - m
        for n in ns_for(l, known):
            ids = rng.sample(range(K), known)  # shuffled
            coeffs = [rng.randrange(R) for _ in range(n)]
            cells = RM.coset_cells(coeffs, N, l, ids)
            got, evals, ok = RM.recover(N, l, n, ids, cells)
            assert ok and got == coeffs, (N, l, n, m)
            assert evals == RM.ntt(coeffs + [0] * (N - n)), (N, l, n, m)
            assert RM.coset_cells(None, N, l, ids, evals=evals) == cells


@pytest.mark.parametrize("log_n,log_l", [(3, 0), (4, 2), (5, 1), (6, 3), (6, 0), (6, 6)])
def test_consistency_criterion(log_n, log_l):
    rng = random.Random(50 + 7 * log_n + log_l)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    for m in sorted({0, K // 2, K - 1}):
        known = K - m
        for n in ns_for(l, known):
            ids = rng.sample(range(K), known)
            cells = RM.coset_cells([rng.randrange(R) for _ in range(n)], N, l, ids)
            j, t = rng.randrange(known), rng.randrange(l)
            cells[j][t] = (cells[j][t] + 1 + rng.randrange(R - 1)) % R
            _, _, ok = RM.recover(N, l, n, ids, cells)
            # known * l > n: some coefficient in [n + m l, N) is non-zero; known * l == n: the range is empty, any values fit
            assert ok == (known * l == n), (N, l, n, m)


def test_zero_polynomial_vanishes_on_the_missing_cosets_only():
    N, l = 64, 4
    K = N // l
    w = M.compute_omega(N)[2]
    missing = [1, 5, 6, 15]
    zs = RM.zero_poly_plain([pow(w, l * i, R) for i in missing])
    for j in range(N):
        z = sum(c * pow(w, j * l * k, R) for k, c in enumerate(zs)) % R      # Z(w^j) = Zs(w^(jl))
        assert (z == 0) == (j % K in missing), j
        assert z == sum(c * pow(w, (j % K) * l * k, R) for k, c in enumerate(zs)) % R
    g = pow(RM.SHIFT, l, R)
    for j in range(K):
        assert sum(c * pow(g * pow(w, l * j, R), k, R) for k, c in enumerate(zs)) % R != 0


# the root counts at which the padded tree changes shape, for the leaf size the kernels use
TREE_COUNTS = [0, 1, L - 1, L, L + 1, 2 * L + 1, 3 * L, 4 * L, 4 * L + 1]


@pytest.mark.parametrize("m", TREE_COUNTS)
def test_padded_product_tree_matches_plain_product(m):
    rng = random.Random(900 + m)
    roots = [rng.randrange(R) for _ in range(m)]
    assert RM.zero_poly_tree(roots) == RM.zero_poly_plain(roots), m


@pytest.mark.parametrize("leaf", [2, 4, 16])
def test_padded_product_tree_small_leaves(leaf):
    # the same layout with small leaves: every root count up to 4 leaves and the powers of two around deeper trees
    rng = random.Random(leaf)
    for m in list(range(0, 4 * leaf + 2)) + [16 * leaf - 1, 16 * leaf, 16 * leaf + 1]:
        roots = [rng.randrange(R) for _ in range(m)]
        assert RM.zero_poly_tree(roots, leaf) == RM.zero_poly_plain(roots), (leaf, m)


@pytest.mark.parametrize("N,m,n", [(2048, 2 * L + 1, 300), (4096, L - 1, 1), (4096, L, 1), (4096, L + 1, 1), (4096, 2 * L + 1, 1)])
def test_recovery_through_the_tree(N, m, n):
    # the model with its zero polynomial from the padded tree, at the cheaper of the shapes tests/test_gpu_recover.py runs at the
    # tree's edges (that file runs RM.recover_with_tree at all of them, beside the GPU)
    rng = random.Random(4 + m)
    ids = rng.sample(range(N), N - m)
    coeffs = [rng.randrange(R) for _ in range(n)]
    got, evals, ok = RM.recover_with_tree(N, 1, n, ids, RM.coset_cells(coeffs, N, 1, ids))
    assert ok and got == coeffs and evals == RM.ntt(coeffs + [0] * (N - n))


def test_kernel_constants_match_the_model():
    # the GPU tests' tree shapes are built around RM.LEAF and their batch around RM.chunk_size: if recover.hip changes either,
    # this fails instead of those tests quietly covering less
    with open(os.path.join(ROOT, "kzg_amd", "csrc", "recover.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t REC_LEAF = (\d+);", src).group(1)) == RM.LEAF == 256
    assert int(re.search(r"constexpr uint32_t REC_SMALL_LOG = (\d+);", src).group(1)) == 10
    assert int(re.search(r"constexpr uint32_t REC_TILE_LOG = (\d+);", src).group(1)) == 11
    assert re.search(r"REC_MAX_CHUNK = 4096, REC_CHUNK_POINTS = \(size_t\)1 << 21;", src)
    for N in (1, 1 << 10, 1 << 14, 1 << 20, 1 << 22):
        assert RM.chunk_size(N) == F.chunk_size(N)
    assert RM.tree_launches(1 << 19) == 122     # 2^20 / l = 1 with half the points missing


def test_library_exports_recovery():
    import kzg_amd
    from kzg_amd import _lib
    for m in ("recover_cosets", "recover_cosets_batch"):
        assert callable(getattr(kzg_amd.Engine, m)), m
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "kzg_recover_cosets")
