"""The integer model of the sumcheck calls (tests/mle_model.py) against the identities it has to satisfy, and a complete prove / verify
in integers.  No GPU."""
import random

import pytest

from tests import fr_program_model as FM
from tests import mle_model as MM

R = MM.R


def rand(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def hypercube_sum(prog, cols, consts):
    words, n_cols, n_consts, n_out = prog
    return [sum(o) % R for o in FM.run(words, n_cols, n_consts, n_out, cols, consts, len(cols[0]))]


@pytest.mark.parametrize("m", range(0, 7))
def test_eq_dotted_with_a_table_is_its_evaluation(m):
    rng = random.Random(7100 + m)
    f, u = rand(rng, 1 << m), rand(rng, m)
    e = MM.eq(u)
    assert sum(e) % R == 1
    assert sum(a * b for a, b in zip(e, f)) % R == MM.evaluate(f, u)[0]
    # at a corner the table is an indicator and the evaluation a lookup
    corner = [rng.randrange(2) for _ in range(m)]
    idx = sum(b << j for j, b in enumerate(corner))
    assert MM.eq(corner) == [int(i == idx) for i in range(1 << m)] and MM.evaluate(f, corner)[0] == f[idx]


@pytest.mark.parametrize("m", range(1, 6))
def test_the_zeromorph_identity_at_random_points(m):
    """f(X) - f(u) = sum_k (X_k - u_k) q_k(X_0 .. X_{k-1})"""
    rng = random.Random(7200 + m)
    f, u = rand(rng, 1 << m), rand(rng, m)
    y, q = MM.evaluate(f, u)
    assert len(q) == (1 << m) - 1
    for _ in range(4):
        x = rand(rng, m)
        rhs = sum((x[k] - u[k]) * MM.evaluate(q[(1 << k) - 1:(2 << k) - 1], x[:k])[0] for k in range(m))
        assert (MM.evaluate(f, x)[0] - y) % R == rhs % R


def test_bind_is_evaluation_in_the_top_variable():
    rng = random.Random(7300)
    f, u = rand(rng, 32), rand(rng, 5)
    assert MM.evaluate(MM.bind(f, u[4]), u[:4])[0] == MM.evaluate(f, u)[0]
    assert MM.bind(f, 0) == f[:16] and MM.bind(f, 1) == f[16:]
    assert MM.bind([5, R + 9], 3) == [(5 + 3 * 4) % R]                     # any integer counts as its residue


def test_s0_plus_s1_is_the_hypercube_sum_and_the_degree_bound_is_tight():
    rng = random.Random(7400)
    for prog, exact in ((MM.product_program(), 2), (MM.eq_gate_program(), 4)):
        words, n_cols, n_consts, n_out = prog
        assert MM.degrees(*prog) == [exact]
        cols = [rand(rng, 16) for _ in range(n_cols)]
        s = MM.round_sums(words, n_cols, n_consts, n_out, cols, [], exact + 4)[0]
        assert (s[0] + s[1]) % R == hypercube_sum(prog, cols, [])[0]
        # degree + 1 points determine s; one point fewer does not
        for x in range(exact + 1, exact + 4):
            assert MM.interpolate(s[:exact + 1], x) == s[x]
            assert MM.interpolate(s[:exact], x) != s[x]


def test_degrees_of_consts_sums_and_temporaries():
    I, C, K, T, O = FM.insn, FM.COL, FM.CONST, FM.TEMP, FM.OUT
    words = (I(FM.ADD, O, 0, K, 0, K, 0) + I(FM.SUB, O, 1, C, 0, K, 0) + I(FM.MUL, T, 0, C, 0, C, 1) + I(FM.MUL, T, 0, T, 0, T, 0) +
             I(FM.ADD, O, 2, T, 0, C, 0) + I(FM.MUL, O, 3, T, 0, K, 0))
    assert MM.degrees(words, 2, 1, 4) == [0, 1, 4, 4]
    sq = I(FM.MUL, T, 0, C, 0, C, 0)
    for _ in range(40):
        sq += I(FM.MUL, T, 0, T, 0, T, 0)
    assert MM.degrees(sq + I(FM.ADD, O, 0, T, 0, T, 0), 1, 0, 1) == [(1 << 32) - 1]      # 2^41 saturates


def test_the_round_refuses_what_the_header_lists():
    words, n_cols, n_consts, n_out = MM.product_program()
    cols = [[1, 2, 3, 4], [5, 6, 7, 8]]
    for n_eval in (0, 17, 33):
        with pytest.raises(MM.ShapeError):
            MM.round_sums(words, 2, 0, 1, cols, [], n_eval)
    with pytest.raises(MM.ShapeError):
        MM.round_sums(FM.insn(FM.MUL, FM.OUT, 0, FM.COL, 0, FM.COL, 1, 1, 0), 2, 0, 1, cols, [], 3)       # a rotation
    with pytest.raises(MM.ShapeError):
        MM.round_sums(words, 2, 0, 1, [[1, 2, 3], [4, 5, 6]], [], 3)
    two = FM.insn(FM.MUL, FM.OUT, 0, FM.COL, 0, FM.COL, 1) + FM.insn(FM.ADD, FM.OUT, 1, FM.COL, 0, FM.COL, 1)
    assert len(MM.round_sums(two, 2, 0, 2, cols, [], 16)) == 2
    with pytest.raises(MM.ShapeError):
        MM.round_sums(two + FM.insn(FM.SUB, FM.OUT, 2, FM.COL, 0, FM.COL, 1), 2, 0, 3, cols, [], 11)      # 33 accumulators
    with pytest.raises(MM.ShapeError):
        MM.eq([R])
    with pytest.raises(MM.ShapeError):
        MM.bind([1, 2], R)


def gate_witness(rng, m):
    """nine columns of 2^m rows on which eq x gate sums to ... whatever it sums to: the claim is computed, not assumed zero"""
    n = 1 << m
    cols = [rand(rng, n) for _ in range(8)]
    return cols + [MM.eq(rand(rng, m))]


def test_a_complete_proof_of_eq_times_gate_is_accepted_and_a_changed_column_is_not():
    rng = random.Random(7500)
    m, prog = 6, MM.eq_gate_program()
    cols = gate_witness(rng, m)
    claim = hypercube_sum(prog, cols, [])
    chal = random.Random(7501)
    challenges = [chal.randrange(R) for _ in range(m)]
    rounds, point, finals = MM.prove(*prog, cols, [], lambda k, s: challenges[k])
    assert point == challenges[::-1] and len(rounds) == m and all(len(s[0]) == 5 for s in rounds)
    assert finals == [MM.evaluate(c, point)[0] for c in cols]
    ev = lambda v: [MM.eq_gate_value(v)]  # noqa: E731
    assert MM.verify(claim, rounds, point, finals, ev)
    # the kzg_amd verifier is the same check
    from kzg_amd import sumcheck
    assert sumcheck.verify(claim, rounds, point, finals, ev)
    assert not sumcheck.verify([(claim[0] + 1) % R], rounds, point, finals, ev)
    # one element changed, the old claim kept: the first round's s(0) + s(1) no longer matches
    cols[2][5] = (cols[2][5] + 1) % R
    rounds2, point2, finals2 = MM.prove(*prog, cols, [], lambda k, s: challenges[k])
    assert not MM.verify(claim, rounds2, point2, finals2, ev) and not sumcheck.verify(claim, rounds2, point2, finals2, ev)
    # the honest rounds with the changed column's final values fail at the end
    assert not MM.verify(claim, rounds, point, finals2, ev)
