"""The two point decoders -- k_decode_points (kzg_amd/csrc/srs.hip, G1) and k_g2_decode (kzg_amd/csrc/pairing.hip, G2) -- against
the strict reference decoder (oracle/decode.py) over the corpus of tests/decode_corpus.py: every flag bit, every bound, every
branch of the square roots and of the sign comparison, in all eight formats and at both validation levels; one encoding per call,
thousands per launch, one bad encoding anywhere in a launch, and the two decoders behind every verifier entry point.

Every input is well-formed memory of the right size with unusual contents.  This file sorts after the tests that release the
session's contexts (tests/conftest.py ORDER), so it opens and closes a module-scoped Engine of its own."""
import ctypes
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import decode as D
from tests import decode_corpus as DC

pytestmark = pytest.mark.gpu

VP, SZ, U32, I32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
FMT_IDS = [DC.FMT_NAMES[f] for f in DC.FORMATS]
BAD = L.KZG_ERR_BAD_POINT
TAU = 0xDEC0DE5EED
SENTINEL = 0xA5
assert (L.G1_AFFINE_MONT, L.G1_JACOBIAN_MONT, L.G1_ZCASH_UNCOMPRESSED, L.G1_ZCASH_COMPRESSED) == DC.FORMATS
assert (L.G2_AFFINE_MONT, L.G2_JACOBIAN_MONT, L.G2_UNCOMPRESSED, L.G2_COMPRESSED) == DC.FORMATS


@pytest.fixture(scope="module")
def eng():
    e = kzg_amd.Engine(0)
    yield e
    e.set_option("trusted_points", 0)
    e.close()


def want_bytes(group, P):
    """the oracle's point in the engine's resident form (affine Montgomery)"""
    return D.encode_point(group, D.AFFINE_MONT, P)


def reference(e, level):
    """(accepted, point) of the strict decoder, checked against the hand label on the way"""
    try:
        P = D.decode_point(e.group, e.fmt, e.data, level)
        ok = True
    except D.BadPoint:
        P, ok = None, False
    assert ok == DC.accepted(e.cls, level), e.name
    return ok, P


# ---- the three ways a G1 / G2 encoding reaches a decoder ---------------------------------------------------------------------------
def g1_sum(eng, blob, count, groups, pfmt, ofmt):
    """(rc, out): kzg_g1_sum_batch with `groups` sums of `count` points -- decodes at the on-curve level whatever the options say"""
    out = ctypes.create_string_buffer(groups * L.POINT_BYTES[ofmt])
    if groups == 1:
        rc = eng.lib.kzg_g1_sum(eng.ctx, blob, count, pfmt, 0, out, ofmt)
    else:
        rc = eng.lib.kzg_g1_sum_batch(eng.ctx, blob, count, groups, pfmt, 0, out, ofmt)
    return rc, out.raw


def g1_upload(eng, blob, n, pfmt):
    """(rc, the n resident points as affine Montgomery bytes or None): kzg_srs_upload_g1 + kzg_srs_download_g1"""
    h = VP()
    rc = eng.lib.kzg_srs_upload_g1(eng.ctx, blob, n, pfmt, ctypes.byref(h))
    if rc:
        return rc, None
    try:
        out = ctypes.create_string_buffer(96 * n)
        assert eng.lib.kzg_srs_download_g1(eng.ctx, h, 0, n, out, L.G1_AFFINE_MONT) == 0, eng.last_error()
        return 0, out.raw
    finally:
        eng.lib.kzg_srs_free(eng.ctx, h)


def g2_upload(eng, blob, n, pfmt, back=()):
    """(rc, {fmt: the n resident points in fmt}): kzg_srs_upload_g2 + kzg_srs_download_g2 in affine Montgomery and in `back`"""
    h = VP()
    rc = eng.lib.kzg_srs_upload_g2(eng.ctx, blob, n, pfmt, ctypes.byref(h))
    if rc:
        return rc, None
    try:
        got = {}
        for fmt in (L.G2_AFFINE_MONT,) + tuple(back):
            out = ctypes.create_string_buffer(L.G2_POINT_BYTES[fmt] * n)
            assert eng.lib.kzg_srs_download_g2(eng.ctx, h, 0, n, out, fmt) == 0, eng.last_error()
            got[fmt] = out.raw
        return 0, got
    finally:
        eng.lib.kzg_srs_g2_free(eng.ctx, h)


def levels(eng):
    """(level, enter, leave): the subgroup level is the default, option trusted_points = 1 gives the on-curve level"""
    return ((2, lambda: None, lambda: None),
            (1, lambda: eng.set_option("trusted_points", 1), lambda: eng.set_option("trusted_points", 0)))


# ---- 1. one encoding per call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", DC.FORMATS, ids=FMT_IDS)
def test_g1_on_curve_level_one_encoding_per_call(eng, fmt):
    """kzg_g1_sum of ONE point decodes at the on-curve level and hands the decoded point back: the verdict of every corpus entry,
    the point of every accepted one, and for the wire formats the input's own bytes when the point is written in its format."""
    wrong = []
    for e in DC.entries("g1", fmt):
        ok, P = reference(e, 1)
        rc, out = g1_sum(eng, e.data, 1, 1, fmt, L.G1_AFFINE_MONT)
        if rc != (0 if ok else BAD):
            wrong.append((e.name, e.cls, "rc %d" % rc))
        elif ok and out != want_bytes("g1", P):
            wrong.append((e.name, e.cls, "another point"))
        elif ok and fmt in D.WIRE_FORMATS and g1_sum(eng, e.data, 1, 1, fmt, fmt) != (0, e.data):
            wrong.append((e.name, e.cls, "re-encoded differently"))
    assert not wrong, wrong


@pytest.mark.parametrize("fmt", DC.FORMATS, ids=FMT_IDS)
def test_g1_upload_both_levels_one_encoding_per_call(eng, fmt):
    """kzg_srs_upload_g1 of ONE point, by default (subgroup level) and under trusted_points = 1 (on-curve level).  The download is
    affine Montgomery (the only form kzg_srs_download_g1 writes); a wire encoding is re-encoded from it by kzg_g1_sum."""
    wrong = []
    for level, enter, leave in levels(eng):
        enter()
        try:
            for e in DC.entries("g1", fmt):
                ok, P = reference(e, level)
                rc, got = g1_upload(eng, e.data, 1, fmt)
                if rc != (0 if ok else BAD):
                    wrong.append((level, e.name, e.cls, "rc %d" % rc))
                elif ok and got != want_bytes("g1", P):
                    wrong.append((level, e.name, e.cls, "another point"))
                elif ok and fmt in D.WIRE_FORMATS and g1_sum(eng, got, 1, 1, L.G1_AFFINE_MONT, fmt) != (0, e.data):
                    wrong.append((level, e.name, e.cls, "re-encoded differently"))
        finally:
            leave()
    assert not wrong, wrong


@pytest.mark.parametrize("fmt", DC.FORMATS, ids=FMT_IDS)
def test_g2_upload_both_levels_one_encoding_per_call(eng, fmt):
    wrong = []
    for level, enter, leave in levels(eng):
        enter()
        try:
            for e in DC.entries("g2", fmt):
                ok, P = reference(e, level)
                rc, got = g2_upload(eng, e.data, 1, fmt, back=(fmt,) if fmt in D.WIRE_FORMATS else ())
                if rc != (0 if ok else BAD):
                    wrong.append((level, e.name, e.cls, "rc %d" % rc))
                elif ok and got[L.G2_AFFINE_MONT] != want_bytes("g2", P):
                    wrong.append((level, e.name, e.cls, "another point"))
                elif ok and fmt in D.WIRE_FORMATS and got[fmt] != e.data:
                    wrong.append((level, e.name, e.cls, "re-encoded differently"))
        finally:
            leave()
    assert not wrong, wrong


def test_entries_labelled_on_curve_only_need_trusted_points(eng):
    """the same bytes: refused by default, accepted under trusted_points = 1, refused again afterwards"""
    for group, upload in (("g1", g1_upload), ("g2", g2_upload)):
        es = DC.entries(group, classes=("ok-oncurve-only",))
        assert len(es) >= 12
        for e in es:
            assert upload(eng, e.data, 1, e.fmt)[0] == BAD, e.name
        eng.set_option("trusted_points", 1)
        try:
            for e in es:
                assert upload(eng, e.data, 1, e.fmt)[0] == 0, e.name
        finally:
            eng.set_option("trusted_points", 0)
        assert upload(eng, es[0].data, 1, es[0].fmt)[0] == BAD


# ---- 2. many lanes ----------------------------------------------------------------------------------------------------------------
def mixed(group, fmt, classes, n, seed):
    """n accepted encodings of one format: every entry of `classes` in turn, shuffled"""
    es = DC.entries(group, fmt, classes)
    picked = [es[k % len(es)] for k in range(n)]
    random.Random(seed).shuffle(picked)
    return picked


@pytest.mark.parametrize("fmt", DC.FORMATS, ids=FMT_IDS)
def test_g1_mixed_lanes(eng, fmt):
    """4096 + 45 encodings in one launch (sixteen full blocks of k_decode_points and a partial one), every accepted kind next to
    every other: each lane decodes its own point -- through kzg_g1_sum_batch (on-curve level, so the points outside the subgroup ride
    along) and through one upload (subgroup level)."""
    n = 4096 + 45
    picked = mixed("g1", fmt, DC.OK_CLASSES, n, 11)
    rc, out = g1_sum(eng, b"".join(e.data for e in picked), 1, n, fmt, L.G1_AFFINE_MONT)
    assert rc == 0, eng.last_error()
    want = b"".join(want_bytes("g1", e.point) for e in picked)
    assert [k for k in range(n) if out[96 * k:96 * k + 96] != want[96 * k:96 * k + 96]] == []
    picked = mixed("g1", fmt, ("ok",), n, 12)
    rc, got = g1_upload(eng, b"".join(e.data for e in picked), n, fmt)
    assert rc == 0, eng.last_error()
    want = b"".join(want_bytes("g1", e.point) for e in picked)
    assert [k for k in range(n) if got[96 * k:96 * k + 96] != want[96 * k:96 * k + 96]] == []


@pytest.mark.parametrize("fmt", DC.FORMATS, ids=FMT_IDS)
def test_g2_mixed_lanes(eng, fmt):
    """2 * 64 + 45 encodings: two full blocks of k_g2_decode and a partial one, at both levels"""
    n = 2 * 64 + 45
    for level, enter, leave in levels(eng):
        picked = mixed("g2", fmt, ("ok",) if level == 2 else DC.OK_CLASSES, n, 13 + level)
        enter()
        try:
            rc, got = g2_upload(eng, b"".join(e.data for e in picked), n, fmt)
        finally:
            leave()
        assert rc == 0, eng.last_error()
        want = b"".join(want_bytes("g2", e.point) for e in picked)
        assert [k for k in range(n) if got[L.G2_AFFINE_MONT][192 * k:192 * k + 192] != want[192 * k:192 * k + 192]] == [], level


def representative(group, cls):
    """one encoding of a bad class whose fault is of that class ALONE -- a point of the subgroup under the infinity flag, with one
    coordinate written as v + q, with y + 1 -- so that no later check (the subgroup test) can refuse it for another reason"""
    fmt = D.COMPRESSED if cls == "bad-flags" else D.UNCOMPRESSED
    name = {"bad-flags": "flags6_", "bad-range": "alias_sub_1_plus_q", "bad-curve": "y_plus_1"}[cls]
    es = [e for e in DC.entries(group, fmt, (cls,)) if name in e.name]
    assert es, (group, cls)
    return es[0]


@pytest.mark.parametrize("cls", ["bad-flags", "bad-range", "bad-curve"])
@pytest.mark.parametrize("group", DC.GROUPS)
def test_one_bad_among_many(eng, group, cls):
    """the verdict of a launch is one flag every lane ORs into: a bad encoding is seen wherever it sits -- first and last lane of a
    wave, of a block of either kernel (64 and 256 threads), of the launch"""
    n = 300
    bad = representative(group, cls)
    good = [e.data for e in mixed(group, bad.fmt, ("ok",), n, 21)]
    upload = g1_upload if group == "g1" else g2_upload
    assert upload(eng, b"".join(good), n, bad.fmt)[0] == 0, eng.last_error()
    for pos in (0, 63, 64, 255, 256, n - 1):
        blob = b"".join(good[:pos] + [bad.data] + good[pos + 1:])
        assert upload(eng, blob, n, bad.fmt)[0] == BAD, (bad.name, pos)
        if group == "g1":
            assert g1_sum(eng, blob, 1, n, bad.fmt, L.G1_AFFINE_MONT)[0] == BAD, (bad.name, pos)
            assert g1_sum(eng, blob, n, 1, bad.fmt, L.G1_AFFINE_MONT)[0] == BAD, (bad.name, pos)


# ---- 3. routing: every verifier entry point decodes through the same two kernels ----------------------------------------------------
@pytest.fixture(scope="module")
def world(eng):
    params = kzg_amd.setup(eng, TAU, 16, g2_len=5)
    lag_g = kzg_amd.setup_lagrange(eng, TAU, 4)
    lag_h = kzg_amd.setup_lagrange_g2(eng, TAU, 4)
    ver = kzg_amd.CosetVerifier(eng, params, 3, 1)
    yield params, lag_g, lag_h, ver
    ver.free()
    for s in (params.gs, params.hs, lag_g, lag_h):
        s.free()


def routing_cases():
    """(name, pfmt, commitment, witness, honest commitment, honest witness): a lax identity as the witness -- the infinity flag over
    a payload, which used to decode to the identity -- and a sign-flagged uncompressed commitment"""
    base = dict(DC.base_points()["g1"]["sub"])
    Cm, W = base["2G"], base["3G"]
    cc, cw = (D.encode_point("g1", D.COMPRESSED, P) for P in (Cm, W))
    uc, uw = (D.encode_point("g1", D.UNCOMPRESSED, P) for P in (Cm, W))
    return [("lax_identity_witness", L.G1_ZCASH_COMPRESSED, cc, b"\xc0" + b"\x01" * 47, cc, cw),
            ("sign_flagged_commitment", L.G1_ZCASH_UNCOMPRESSED, DC.with_flags(uc, 1), uw, uc, uw)]


@pytest.mark.parametrize("case", routing_cases(), ids=lambda c: c[0])
def test_routing_g1(eng, world, case):
    """Each entry point answers KZG_ERR_BAD_POINT and leaves `ok` as it was; the same call with the honest encodings goes through
    (whatever its verdict: the openings are not honest ones), so nothing but the decoder refused it."""
    _name, pfmt, bad_c, bad_w, good_c, good_w = case
    params, lag_g, lag_h, ver = world
    lib, ctx, gs, hs = eng.lib, eng.ctx, params.gs.handle, params.hs.handle
    sc = lambda *v: kzg_amd.pack_scalars(list(v))  # noqa: E731
    idx2, ids2 = (U32 * 2)(0, 0), (SZ * 2)(0, 1)

    def calls(c, w):
        """{entry point: (rc, ok afterwards)}"""
        out = {}
        ok8 = ctypes.create_string_buffer(bytes([SENTINEL]) * 2, 2)
        out["verify_eval"] = lib.kzg_verify_eval(ctx, gs, hs, sc(7, 8), sc(9, 10), L.FR_CANONICAL, good_c + c, good_w + w, pfmt, 2, ok8), ok8.raw
        ok = I32(SENTINEL)
        out["verify_eval_batched"] = lib.kzg_verify_eval_batched(ctx, gs, hs, sc(7, 8), 2, sc(1, 2), 2, L.FR_CANONICAL, c, w, pfmt,
                                                                 ctypes.byref(ok)), ok.value
        ok = I32(SENTINEL)
        out["verify_eval_all"] = lib.kzg_verify_eval_all(ctx, lag_g.handle, lag_h.handle, hs, sc(1, 2, 3, 4), 4, L.FR_CANONICAL, c, w, pfmt,
                                                         ctypes.byref(ok)), ok.value
        ok8 = ctypes.create_string_buffer(bytes([SENTINEL]), 1)
        g2 = D.encode_point("g2", D.AFFINE_MONT, DC.base_points()["g2"]["sub"][0][1])
        out["pairing_check"] = lib.kzg_pairing_check(ctx, c + w, pfmt, g2 + g2, L.G2_AFFINE_MONT, 2, 1, ok8), ok8.raw
        ok8 = ctypes.create_string_buffer(bytes([SENTINEL]) * 2, 2)
        out["verify_cosets"] = lib.kzg_verify_cosets(ctx, ver.handle, c, 1, idx2, ids2, sc(1, 2, 3, 4), good_w + w, 2, L.FR_CANONICAL, pfmt, 0,
                                                     ok8), ok8.raw
        ok = I32(SENTINEL)
        out["verify_cosets_batch"] = lib.kzg_verify_cosets_batch(ctx, ver.handle, c, 1, idx2, ids2, sc(1, 2, 3, 4), good_w + w, 2, sc(5),
                                                                 L.FR_CANONICAL, pfmt, 0, ctypes.byref(ok)), ok.value
        ok = I32(SENTINEL)
        out["verify_eval_batch"] = lib.kzg_verify_eval_batch(ctx, gs, hs, sc(7, 8), sc(9, 10), L.FR_CANONICAL, c, 1, (U32 * 2)(0, 0),
                                                             good_w + w, pfmt, 2, sc(5), ctypes.byref(ok)), ok.value
        ok = I32(SENTINEL)
        out["verify_eval_batch_one_commitment_each"] = lib.kzg_verify_eval_batch(ctx, gs, hs, sc(7), sc(9), L.FR_CANONICAL, c, 1, None, w, pfmt,
                                                                                 1, sc(5), ctypes.byref(ok)), ok.value
        return out

    untouched = {1: bytes([SENTINEL]), 2: bytes([SENTINEL]) * 2}
    for name, (rc, ok) in calls(good_c, good_w).items():
        assert rc == 0, (name, eng.last_error())
        assert ok != (untouched.get(len(ok)) if isinstance(ok, bytes) else SENTINEL), name
    wrong = [(name, rc, ok) for name, (rc, ok) in calls(bad_c, bad_w).items()
             if rc != BAD or ok != (untouched[len(ok)] if isinstance(ok, bytes) else SENTINEL)]
    assert not wrong, wrong


@pytest.mark.parametrize("side", ["g1", "g2"])
def test_routing_pairing_check_both_sides(eng, side):
    base1, base2 = DC.base_points()["g1"]["sub"], DC.base_points()["g2"]["sub"]
    P, Qp = base1[1][1], base2[1][1]
    good = {("g1", D.COMPRESSED): D.encode_point("g1", D.COMPRESSED, P), ("g1", D.UNCOMPRESSED): D.encode_point("g1", D.UNCOMPRESSED, P),
            ("g2", D.COMPRESSED): D.encode_point("g2", D.COMPRESSED, Qp), ("g2", D.UNCOMPRESSED): D.encode_point("g2", D.UNCOMPRESSED, Qp)}
    size = D.point_bytes(side, D.COMPRESSED)
    bads = [(D.COMPRESSED, b"\xc0" + b"\x01" * (size - 1)), (D.UNCOMPRESSED, DC.with_flags(good[(side, D.UNCOMPRESSED)], 1))]
    for fmt, bad in bads:
        for blob, want in ((good[(side, fmt)], 0), (bad, BAD)):
            g1 = blob if side == "g1" else good[("g1", fmt)]
            g2 = blob if side == "g2" else good[("g2", fmt)]
            ok = ctypes.create_string_buffer(bytes([SENTINEL]), 1)
            rc = eng.lib.kzg_pairing_check(eng.ctx, g1, fmt, g2, fmt, 1, 1, ok)
            assert rc == want, (side, fmt, want, eng.last_error())
            assert (ok.raw == bytes([SENTINEL])) == (want == BAD)
