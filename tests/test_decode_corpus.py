"""The strict reference decoder (oracle/decode.py) over the corpus of tests/decode_corpus.py, and the two twelve-word constants of
the G1 wire decoder.  No GPU: tests/test_gpu_decode.py holds the engine's decoders against the same corpus and the same decoder."""
import os
import re

import pytest

from oracle import decode as D
from oracle import kzg_model as M
from oracle import pairing_model as PM
from tests import decode_corpus as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg_amd", "csrc")


def strict(e, level):
    """(accepted, point) of the strict decoder"""
    try:
        return True, D.decode_point(e.group, e.fmt, e.data, level)
    except D.BadPoint:
        return False, None


@pytest.mark.parametrize("group", DC.GROUPS)
@pytest.mark.parametrize("fmt", DC.FORMATS, ids=[DC.FMT_NAMES[f] for f in DC.FORMATS])
def test_strict_decoder_agrees_with_every_hand_label(group, fmt):
    es = DC.entries(group, fmt)
    need = {"ok", "ok-oncurve-only", "bad-range", "bad-sqrt" if fmt == D.COMPRESSED else "bad-curve"}
    assert {e.cls for e in es} >= need, "a class went missing from the corpus"
    for e in es:
        for level in (1, 2):
            got, P = strict(e, level)
            assert got == DC.accepted(e.cls, level), (e.name, e.cls, level)
            if got:
                assert P == e.point, (e.name, level)


def test_corpus_holds_what_the_decoders_can_get_wrong():
    """the classes per format, the branches no honest multiple of a generator reaches, and both signs of every kind of y"""
    for group in DC.GROUPS:
        for fmt in D.WIRE_FORMATS:
            assert {e.cls for e in DC.entries(group, fmt)} >= {"ok", "ok-oncurve-only", "bad-flags", "bad-range"}
            signs = {DC.y_is_larger(group, e.point) for e in DC.entries(group, fmt, DC.OK_CLASSES) if e.point is not None}
            assert signs == {True, False}
        assert "bad-sqrt" in {e.cls for e in DC.entries(group, D.COMPRESSED)}
        assert any(e.point is None for e in DC.entries(group, D.JACOBIAN_MONT, ("ok",)) if any(e.data))     # Z = 0 over a payload
    ys = [e.point[1] for e in DC.entries("g2", D.COMPRESSED, DC.OK_CLASSES) if e.point is not None]
    assert {y[1] > (M.Q - 1) // 2 for y in ys if y[0] == 0} == {True, False}     # purely imaginary y, both signs
    assert {y[0] > (M.Q - 1) // 2 for y in ys if y[1] == 0} == {True, False}     # y in Fq (c1 = 0), both signs
    assert any(e.point == (0, 2) for e in DC.entries("g1", D.AFFINE_MONT))


@pytest.mark.parametrize("group", DC.GROUPS)
def test_accepted_wire_encodings_are_canonical(group):
    """one byte string per group element: re-encoding what the strict decoder accepted gives the bytes back"""
    n = 0
    for fmt in D.WIRE_FORMATS:
        for e in DC.entries(group, fmt):
            got, P = strict(e, 1)
            if got:
                assert D.encode_point(group, fmt, P) == e.data, e.name
                n += 1
    assert n >= 20


def test_level_0_takes_montgomery_limbs_as_they_are():
    for e in DC.entries(fmt=D.AFFINE_MONT, classes=("bad-curve",)) + DC.entries(fmt=D.JACOBIAN_MONT, classes=("bad-range",)):
        D.decode_point(e.group, e.fmt, e.data, D.TRUSTED)
    for e in DC.entries(fmt=D.COMPRESSED, classes=DC.BAD_CLASSES) + DC.entries(fmt=D.UNCOMPRESSED, classes=DC.BAD_CLASSES):
        with pytest.raises(D.BadPoint):
            D.decode_point(e.group, e.fmt, e.data, D.TRUSTED)


def test_lax_helpers_are_strict_now():
    G, H = M.G1, PM.G2
    assert M.g1_from_compressed(M.g1_to_compressed(G)) == G and M.g1_from_uncompressed(M.g1_to_uncompressed(G)) == G
    assert PM.g2_from_compressed(PM.g2_to_compressed(H)) == H and PM.g2_from_uncompressed(PM.g2_to_uncompressed(H)) == H
    for f, blob in ((M.g1_from_compressed, b"\xc0" + b"\x01" * 47), (M.g1_from_uncompressed, b"\x40" + b"\x01" * 95),
                    (M.g1_from_uncompressed, DC.with_flags(M.g1_to_uncompressed(G), 1)), (M.g1_from_uncompressed, bytes(96)),
                    (PM.g2_from_compressed, b"\xe0" + bytes(95)), (PM.g2_from_uncompressed, bytes(192)),
                    (PM.g2_from_uncompressed, DC.with_flags(PM.g2_to_uncompressed(H), 1))):
        with pytest.raises(D.BadPoint):
            f(blob)


def _words(text, name):
    m = re.search(r"constexpr uint32_t %s\[12\] = \{([^}]*)\}" % name, text)
    assert m, name
    words = [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]
    assert len(words) == 12
    return sum(w << (32 * i) for i, w in enumerate(words))


def test_sign_and_square_root_constants_equal_the_integers():
    """H = (q-1)/2 decides the sign flag and E = (q+1)/4 is the square-root exponent.  No curve point sits at the sign boundary, so
    no decoding test pins the low words of H; they are read from the sources instead."""
    with open(os.path.join(CSRC, "srs.hip")) as f:
        srs = f.read()
    assert _words(srs, "H") == (M.Q - 1) // 2
    assert _words(srs, "E") == (M.Q + 1) // 4
    with open(os.path.join(CSRC, "emit.h")) as f:
        assert _words(f.read(), "H") == (M.Q - 1) // 2      # the encoder's copy
