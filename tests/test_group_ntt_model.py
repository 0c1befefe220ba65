"""The constants and the arithmetic behind the G2 DFT's twiddle products, without a GPU: the psi constants of tower_consts.inc against
the Python model, the base-u split and signed recoding, the joint chain against g2_mul, and the FFT-shaped group DFT of
tests/group_ntt_model.py against the naive double sum."""
import os
import random
import re

import pytest

from oracle import kzg_model as M
from oracle import pairing_model as PM
from tests import group_ntt_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, Q, U = M.R, M.Q, G.U
SCALARS = G.EDGE_SCALARS + [random.Random(0x6175).randrange(R) for _ in range(50)]


def inc_table(name):
    """the rows of a table function of tower_consts.inc as integers (Montgomery form undone)"""
    src = open(os.path.join(ROOT, "kzg_amd", "csrc", "tower_consts.inc")).read()
    m = re.search(r"KZG_HD Fq %s\(int i\) \{(.*?)\n\}" % name, src, flags=re.S)
    assert m, f"{name} is not in tower_consts.inc"
    rinv = pow(M.FQ_MONT_R, -1, Q)
    rows = []
    for row in re.findall(r"\{((?:0x[0-9a-f]{8}u,? ?){12})\}", m.group(1)):
        limbs = [int(x.rstrip("u"), 16) for x in row.replace(" ", "").rstrip(",").split(",")]
        rows.append(sum(v << (32 * i) for i, v in enumerate(limbs)) * rinv % Q)
    return rows


@pytest.fixture(scope="module")
def consts():
    t = inc_table("g2_psi_limb")
    assert len(t) == 7
    return {"cx": (t[0], t[1]), "cy": (t[2], t[3]), "cx2": t[4], "cx3": (t[5], t[6])}


def test_generated_constants_are_the_pair_with_psi_h_equal_z_h(consts):
    c = (consts["cx"], consts["cy"])
    assert c == G.derive_psi_consts()
    assert c in G.psi_candidates()
    assert G.psi(PM.G2, c) == PM.g2_mul(PM.G2, G.Z_MOD_R)
    other = [p for p in G.psi_candidates() if p != c][0]
    assert G.psi(PM.G2, other) != PM.g2_mul(PM.G2, G.Z_MOD_R)  # the choice is pinned, not free


def test_psi_is_multiplication_by_z_on_the_subgroup(consts):
    c = (consts["cx"], consts["cy"])
    rng = random.Random(11)
    for _ in range(4):
        a = rng.randrange(1, R)
        assert G.psi(PM.g2_mul(PM.G2, a), c) == PM.g2_mul(PM.G2, a * G.Z_MOD_R % R)
    assert G.psi(None, c) is None


def test_psi_powers_are_the_shortcuts_the_kernel_applies(consts):
    """psi^2: x times an Fq constant, y negated; psi^3: conj x times cx3, conj y times -cy"""
    c = (consts["cx"], consts["cy"])
    P = PM.g2_mul(PM.G2, 0xABCDEF)
    assert G.psi(P, c, 2) == (PM.f2_scale(P[0], consts["cx2"]), PM.f2_neg(P[1]))
    assert G.psi(P, c, 3) == (PM.f2_mul(consts["cx3"], PM.f2_conj(P[0])), PM.f2_neg(PM.f2_mul(consts["cy"], PM.f2_conj(P[1]))))
    assert G.psi(P, c, 2) == PM.g2_mul(P, U * U % R) and G.psi(P, c, 3) == PM.g2_mul(P, (-U ** 3) % R)


def test_split_recombines_with_every_word_below_u():
    for k in SCALARS:
        ks = G.split_u(k)
        assert len(ks) == 4 and all(0 <= v < U for v in ks), hex(k)
        assert sum(v * U ** i for i, v in enumerate(ks)) == k


def test_recoding_has_17_digits_in_range_and_the_value():
    for v in [0, 1, 7, 8, 2 ** 64 - 1, int("7" * 16, 16), int("8" * 16, 16), U - 1]:
        d = G.recode64(v)
        assert len(d) == 17 and all(-8 <= x <= 7 for x in d[:16]) and d[16] in (0, 1)
        assert sum(x * 16 ** i for i, x in enumerate(d)) == v
    assert G.recode64(int("8" * 16, 16))[16] == 1 and G.recode64(int("7" * 16, 16))[16] == 0  # the 17th digit on both sides
    for k in SCALARS:
        d = G.recode256(k)
        assert len(d) == 64 and all(-8 <= x <= 7 for x in d) and sum(x * 16 ** i for i, x in enumerate(d)) == k


def test_joint_chain_equals_g2_mul(consts):
    c = (consts["cx"], consts["cy"])
    P = PM.g2_mul(PM.G2, 0x1234567)
    for k in SCALARS:
        want = PM.g2_mul(P, k)
        assert G.gls_mul(P, k, c) == want, hex(k)
    for k in G.EDGE_SCALARS:
        assert G.plain_mul(P, k) == PM.g2_mul(P, k), hex(k)
        assert G.gls_mul(None, k, c) is None


def test_model_dft_of_size_8_equals_the_naive_double_sum():
    rng = random.Random(5)
    pts = [PM.g2_mul(PM.G2, rng.randrange(R)) for _ in range(8)]
    assert G.dft(G.G2, pts) == G.dft_naive(G.G2, pts)
    assert G.dft(G.G2, pts, inverse=True) == G.dft_naive(G.G2, pts, inverse=True)
    assert G.dft(G.G2, G.dft(G.G2, pts), inverse=True) == pts
    g1 = [M.g1_mul(M.G1, rng.randrange(R)) for _ in range(8)]
    assert G.dft(G.G1, g1) == G.dft_naive(G.G1, g1)
    assert G.dft(G.G1, g1, inverse=True) == G.dft_naive(G.G1, g1, inverse=True)
    structured = [pts[0], PM.g2_neg(pts[0]), None, pts[0], pts[0], pts[0], None, PM.g2_neg(pts[0])]
    assert G.dft(G.G2, structured) == G.dft_naive(G.G2, structured)
