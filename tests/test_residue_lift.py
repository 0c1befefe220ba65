"""The generator of tests/test_gpu_scalar_residues.py on its own (no GPU): every lifted word is congruent to its input, fits in
32 bytes, and is >= r exactly where the mode says so; the edge words are the ones the module promises."""
import random

import pytest

from tests import residue_lift as RL

R, TOP = RL.R, RL.TOP


@pytest.mark.parametrize("n", [1, 5, 6, 8, 33, 777])
@pytest.mark.parametrize("mode", RL.MODES)
def test_lift_is_congruent_in_range_and_lifted_where_promised(n, mode):
    v = RL.base(random.Random(n), n)
    assert all(0 <= x < R for x in v) and len(v) == n
    w = RL.lift(v, mode)
    assert len(w) == n
    moved = set(RL.lifted_positions(n, mode))
    for i, (a, b) in enumerate(zip(v, w)):
        assert b % R == a and 0 <= b < TOP, (i, mode)
        assert (b >= R) == (i in moved), (i, mode)
        if i not in moved:
            assert b == a
    if mode == "all":
        assert moved == set(range(n))
    if mode == "sparse":
        assert moved == set(range(0, n, 7))
    assert RL.pack(w) == RL.lift_bytes(RL.pack(v), mode)
    assert RL.lift(v, mode) == w and v == RL.base(random.Random(n), n)      # deterministic, inputs untouched


def test_base_and_edge_words():
    v = RL.base(random.Random(1), 777)
    assert tuple(v[:6]) == (0, 0, 1, 1, R - 1, (TOP - 1) % R) and v[-1] == R - 1
    assert all(0 < v[i] < TOP - 2 * R for i in (6, 7))
    e = RL.lift(v, "edges")
    assert tuple(e[:6]) == (R, 2 * R, R + 1, 2 * R + 1, 2 * R - 1, TOP - 1)
    assert e[7] == v[7] + 2 * R and e[6] == v[6]                            # a residue with two lifted representatives takes the larger
    a = RL.lift(v, "all")
    assert a[0] == 2 * R and a[4] == 2 * R - 1 and a[5] == TOP - 1 and a[7] == v[7] + 2 * R
    assert all(x == y + R or x == y + 2 * R for x, y in zip(a, v))
    assert all(x + R >= TOP for x in a)                                     # "all" takes the largest representative
    assert 2 * R < TOP < 3 * R                                              # why two conditional subtractions reach the residue
    with pytest.raises(AssertionError):
        RL.lift([R], "all")
    with pytest.raises(ValueError):
        RL.lift([1], "most")
