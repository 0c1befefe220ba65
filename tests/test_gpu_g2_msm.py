"""kzg_msm_g2_bucket (kzg_amd/csrc/g2_msm.hip) on the GPU: g2_madd value by value through its hook, the call byte for byte against
kzg_msm_g2 across slice and chunk boundaries, formats, residency, lifted scalars, extreme digits, equal / opposite / identity points,
2^16 + 1 terms under a known secret, the shape errors and concurrent callers."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import kzg_model as M
from oracle import pairing_model as P
from tests import residue_lift as RL

pytestmark = pytest.mark.gpu

R, Q = M.R, P.Q
TAU = 0x5EED0F71A5
X80 = int.from_bytes(b"\x80" * 32, "little")
ENC = {L.G2_AFFINE_MONT: P.g2_to_affine_mont, L.G2_JACOBIAN_MONT: P.g2_to_jacobian_mont, L.G2_UNCOMPRESSED: P.g2_to_uncompressed,
       L.G2_COMPRESSED: P.g2_to_compressed}


@pytest.fixture(scope="module")
def engine():  # noqa: F811
    """contexts of this module's own: in the suite's order (tests/conftest.py ORDER) the file runs behind the tests that close the
    session's contexts"""
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks_engine():  # noqa: F811
    from tests.gpu_common import HooksEngine
    h = HooksEngine(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def hs(engine):
    s = kzg_amd.setup_g2(engine, TAU, 5003)
    yield s
    s.free()


@pytest.fixture
def small_shape(engine):
    """slices of 4 points, 2 slice slots: a chunk is 8 points"""
    engine.set_option("g2_msm_slice", 4)
    engine.set_option("g2_msm_slots", 2)
    yield 4, 8
    engine.set_option("g2_msm_slice", 0)
    engine.set_option("g2_msm_slots", 0)


def scalars(rng, n):
    sc = [rng.randrange(R) for _ in range(n)]
    for i, v in enumerate([R - 1, 0, 1, X80 % R][:n]):
        sc[i] = v
    return sc


def mont(x):
    return x * M.FQ_MONT_R % Q


def f2b(a):
    return mont(a[0]).to_bytes(48, "little") + mont(a[1]).to_bytes(48, "little")


def jacobian(pt, z):
    """(X, Y, Z) = (x z^2, y z^3, z) in Montgomery form; None is Z = 0 with arbitrary X, Y"""
    if pt is None:
        return f2b((3, 4)) + f2b((5, 6)) + bytes(96)
    z2 = P.f2_sqr(z)
    return f2b(P.f2_mul(pt[0], z2)) + f2b(P.f2_mul(pt[1], P.f2_mul(z2, z))) + f2b(z)


# ---------------------------------------------------------------------------------------------------------------------
# g2_madd
# ---------------------------------------------------------------------------------------------------------------------
def test_g2_madd_value_by_value(hooks_engine):
    fn = hooks_engine.lib.kzg_test_g2_madd
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    rng = random.Random(21)
    pool = [P.g2_mul(P.G2, rng.randrange(1, R)) for _ in range(6)]
    cases = []
    for i in range(100):  # more than one wave, the classes mixed lane by lane
        a, b = pool[rng.randrange(6)], pool[rng.randrange(6)]
        cls = i % 7
        if cls == 1:
            b = a
        elif cls == 2:
            b = P.g2_neg(a)
        elif cls == 3:
            a = None
        elif cls == 4:
            b = None
        elif cls == 5:
            a = b = None
        elif cls == 6 and a == b:
            b = P.g2_add(b, P.G2)
        z = (1, 0) if i % 3 == 0 else (rng.randrange(1, Q), rng.randrange(Q))
        cases.append((a, b, z))
    acc = b"".join(jacobian(a, z) for a, _, z in cases)
    pts = b"".join(P.g2_to_affine_mont(b) for _, b, _ in cases)
    out = ctypes.create_string_buffer(192 * len(cases))
    assert fn(hooks_engine.ctx, acc, pts, len(cases), out) == 0, hooks_engine.last_error()
    for i, (a, b, _) in enumerate(cases):
        assert out.raw[192 * i:192 * i + 192] == P.g2_to_affine_mont(P.g2_add(a, b)), (i, i % 7)
    for args in [(None, pts, 1, out), (acc, None, 1, out), (acc, pts, 1, None), (acc, pts, 0, out), (acc, pts, 4097, out)]:
        assert fn(hooks_engine.ctx, *args) == 3


# ---------------------------------------------------------------------------------------------------------------------
# the call against kzg_msm_g2
# ---------------------------------------------------------------------------------------------------------------------
def test_matches_msm_g2_across_slice_and_chunk_boundaries(engine, hs, small_shape):
    S, CH = small_shape
    rng = random.Random(31)
    for n in [0, 1, 2, S - 1, S, S + 1, 2 * S + 3, CH - 1, CH, CH + 1, 2 * CH + 3]:
        sc = scalars(rng, n)
        for off in (0, 5):
            assert hs.msm_bucket(sc, offset=off) == hs.msm(sc, offset=off), (n, off)
    assert hs.msm_bucket([]) == bytes(192)
    # the model's value too, once: a chunk and a half
    sc = scalars(rng, 12)
    assert hs.msm_bucket(sc, offset=1) == P.g2_to_affine_mont(P.g2_multi_exp(P.setup_g2(TAU, 13)[1:], sc))


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 5000])
def test_matches_msm_g2_at_the_default_slice(engine, hs, n):
    sc = scalars(random.Random(n), n)
    assert hs.msm_bucket(sc, offset=3) == hs.msm(sc, offset=3)


def test_the_options_change_no_bytes(engine, hs):
    sc = scalars(random.Random(41), 300)
    want = hs.msm_bucket(sc)
    try:
        for S, G in [(1, 1), (1, 16), (64, 3), (2048, 1), (256, 0), (0, 5)]:
            engine.set_option("g2_msm_slice", S)
            engine.set_option("g2_msm_slots", G)
            assert hs.msm_bucket(sc) == want, (S, G)
        for key, bad in [("g2_msm_slice", 3), ("g2_msm_slice", 4096), ("g2_msm_slice", -1), ("g2_msm_slots", 17), ("g2_msm_slots", -1)]:
            with pytest.raises(kzg_amd.ReferencePanic):
                engine.set_option(key, bad)
    finally:
        engine.set_option("g2_msm_slice", 0)
        engine.set_option("g2_msm_slots", 0)


def test_scalar_formats_residency_and_output_formats(engine, hs, small_shape):
    rng = random.Random(51)
    n, off = 19, 2
    sc = scalars(rng, n)
    want_pt = P.g2_multi_exp(P.setup_g2(TAU, off + n)[off:], sc)
    can = b"".join(v.to_bytes(32, "little") for v in sc)
    mon = b"".join((v * (1 << 256) % R).to_bytes(32, "little") for v in sc)
    for ofmt, enc in ENC.items():
        assert hs.msm_bucket(sc, offset=off, ofmt=ofmt) == enc(want_pt), ofmt
    for sfmt, blob in [(L.FR_CANONICAL, can), (L.FR_MONT, mon)]:
        out = ctypes.create_string_buffer(b"\xa5" * 192, 192)
        rc = engine.lib.kzg_msm_g2_bucket(engine.ctx, hs.handle, off, blob, n, sfmt, 0, out, L.G2_UNCOMPRESSED)
        assert rc == 0 and out.raw == P.g2_to_uncompressed(want_pt), sfmt
        buf = engine.alloc_scalars(n, sfmt).upload(blob)
        try:
            assert hs.msm_bucket(buf, offset=off, ofmt=L.G2_UNCOMPRESSED) == P.g2_to_uncompressed(want_pt), sfmt
            assert buf.download() == blob  # the caller's scalars are not converted in place
        finally:
            buf.free()


@pytest.mark.parametrize("mode", RL.MODES)
def test_lifted_canonical_scalars_count_as_their_residues(engine, hs, mode):
    base = RL.base(random.Random(61), 40)
    want = hs.msm_bucket(RL.pack(base))
    assert want == hs.msm(base)
    lifted = RL.pack(RL.lift(base, mode))
    assert hs.msm_bucket(lifted) == want
    buf = engine.alloc_scalars(40).upload(lifted)
    try:
        assert hs.msm_bucket(buf) == want
    finally:
        buf.free()


def test_extreme_digits(engine, hs, small_shape):
    n = 21
    geo = lambda c: c * (pow(TAU, n, R) - 1) * pow(TAU - 1, -1, R) % R  # sum_i c tau^i
    enc = lambda k: P.g2_to_affine_mont(P.g2_mul(P.G2, k))
    assert hs.msm_bucket([R - 1] * n) == enc(geo(R - 1))          # every digit of every scalar at its largest
    assert hs.msm_bucket(b"\x80" * (32 * n)) == enc(geo(X80 % R))  # all-0x80 bytes, taken mod r before the digits
    assert hs.msm_bucket(b"\x7f" * (32 * n)) == enc(geo(int.from_bytes(b"\x7f" * 32, "little") % R))
    assert hs.msm_bucket([0] * n) == bytes(192)
    one = [0] * n
    one[13] = 0xDEADBEEF
    assert hs.msm_bucket(one) == enc(0xDEADBEEF * pow(TAU, 13, R) % R)


def test_equal_opposite_and_identity_points_in_one_bucket(engine, small_shape):
    rng = random.Random(71)
    n = 19
    sc = [rng.randrange(R) for _ in range(n)]
    sc[1] = sc[0]                 # the same digits on the same point: P + P in every bucket they meet
    sc[5] = sc[4] = sc[3]
    same = kzg_amd.setup_g2(engine, 1, n)          # every point H
    alt = kzg_amd.setup_g2(engine, R - 1, n)       # H, -H, H, ...
    try:
        assert same.msm_bucket(sc) == P.g2_to_affine_mont(P.g2_mul(P.G2, sum(sc) % R)) == same.msm(sc)
        assert alt.msm_bucket(sc) == P.g2_to_affine_mont(P.g2_mul(P.G2, sum(s if i % 2 == 0 else -s for i, s in enumerate(sc)) % R)) == alt.msm(sc)
        assert alt.msm_bucket([7, 7]) == bytes(192)  # P + (-P): the identity out of one bucket
    finally:
        same.free()
        alt.free()
    pts = [P.G2, None, P.g2_mul(P.G2, 5), None, None, P.g2_neg(P.G2), P.g2_mul(P.G2, 5), None, P.G2]
    up = kzg_amd.SrsG2.upload(engine, b"".join(P.g2_to_affine_mont(p) for p in pts), len(pts))
    try:
        s9 = [3, 3, 3, 9, 0, 3, 3, R - 1, 2]
        assert up.msm_bucket(s9) == P.g2_to_affine_mont(P.g2_multi_exp(pts, s9)) == up.msm(s9)
        assert up.msm_bucket([5, 7], offset=3) == bytes(192)  # identity points alone
    finally:
        up.free()


def test_two_to_the_16_plus_one_terms_under_a_known_secret(engine):
    n = (1 << 16) + 1
    rng = random.Random(81)
    big = kzg_amd.setup_g2(engine, TAU, n)
    try:
        blob = rng.randbytes(32 * n)  # uniform 256-bit words: most are above r
        k, t = 0, 1
        for i in range(n):
            k = (k + int.from_bytes(blob[32 * i:32 * i + 32], "little") * t) % R
            t = t * TAU % R
        assert big.msm_bucket(blob, ofmt=L.G2_COMPRESSED) == P.g2_to_compressed(P.g2_mul(P.G2, k))
    finally:
        big.free()


# ---------------------------------------------------------------------------------------------------------------------
# errors, threads
# ---------------------------------------------------------------------------------------------------------------------
def test_every_shape_error_leaves_out_untouched(engine, hs, hooks_engine):
    lib, ctx = engine.lib, engine.ctx
    sc = b"".join(v.to_bytes(32, "little") for v in range(1, 9))
    fill = b"\x5a" * 288
    out = ctypes.create_string_buffer(fill, 288)
    N = len(hs)
    bad = [
        (ctx, hs.handle, N - 7, sc, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),   # the range exceeds the SRS
        (ctx, hs.handle, N + 1, sc, 0, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),
        (ctx, hs.handle, 0, sc, N + 1, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),
        (ctx, hs.handle, 0, sc, 8, 2, 0, out, L.G2_AFFINE_MONT),                    # unknown scalar format
        (ctx, hs.handle, 0, sc, 8, L.FR_CANONICAL, 0, out, 4),                      # unknown point format
        (ctx, hs.handle, 0, sc, 8, L.FR_CANONICAL, 0, out, -1),
        (ctx, None, 0, sc, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),            # NULL arguments
        (ctx, hs.handle, 0, None, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),
        (None, hs.handle, 0, sc, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT),
    ]
    for args in bad:
        assert lib.kzg_msm_g2_bucket(*args) == 3, args[2:7]
        assert out.raw == fill
    assert lib.kzg_msm_g2_bucket(ctx, hs.handle, 0, sc, 8, L.FR_CANONICAL, 0, None, L.G2_AFFINE_MONT) == 3
    assert lib.kzg_msm_g2_bucket(ctx, hs.handle, 0, None, 0, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT) == 0  # no scalars are read at n = 0
    assert out.raw[:192] == bytes(192)
    # an SRS of another GPU: the hooks library can say so of its own points
    hl, hc = hooks_engine.lib, hooks_engine.ctx
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    hl.kzg_srs_setup_g2.argtypes = [vp, vp, i32, sz, ctypes.POINTER(vp)]
    hl.kzg_srs_g2_free.argtypes = [vp, vp]
    hl.kzg_srs_g2_free.restype = None
    hl.kzg_test_srs_g2_set_device.argtypes = [vp, i32]
    hl.kzg_msm_g2_bucket.argtypes = [vp, vp, sz, vp, sz, i32, i32, vp, i32]
    h = vp()
    assert hl.kzg_srs_setup_g2(hc, (7).to_bytes(32, "little"), L.FR_CANONICAL, 8, ctypes.byref(h)) == 0
    try:
        out = ctypes.create_string_buffer(fill, 288)
        assert hl.kzg_msm_g2_bucket(hc, h, 0, sc, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT) == 0
        assert out.raw[:192] == P.g2_to_affine_mont(P.g2_mul(P.G2, sum((i + 1) * 7 ** i for i in range(8)) % R))
        out = ctypes.create_string_buffer(fill, 288)
        assert hl.kzg_test_srs_g2_set_device(h, 5) == 0
        assert hl.kzg_msm_g2_bucket(hc, h, 0, sc, 8, L.FR_CANONICAL, 0, out, L.G2_AFFINE_MONT) == 3
        assert out.raw == fill and "another GPU" in hooks_engine.last_error()
        assert hl.kzg_test_srs_g2_set_device(h, 0) == 0
    finally:
        hl.kzg_srs_g2_free(hc, h)


def test_four_threads_on_one_context(engine, hs):
    rng = random.Random(91)
    jobs = [(scalars(rng, n), off) for n, off in [(700, 0), (2049, 1), (64, 9), (1500, 100)]]
    want = [hs.msm(sc, offset=off) for sc, off in jobs]
    got, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = hs.msm_bucket(jobs[i][0], offset=jobs[i][1])
                assert got[i] == want[i]
        except Exception as e:  # noqa: BLE001
            errs.append((i, repr(e)))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and got == want
