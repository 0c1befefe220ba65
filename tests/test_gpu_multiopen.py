"""kzg_fr_lincomb / kzg_multiopen_eval_* / kzg_multiopen_coeff_* / kzg_verify_multiopen (kzg_amd/csrc/multiopen.hip, capi.hip,
verify_eval_batch.hip): many polynomials opened at many points with one two-element proof.  The linear combination is compared with
the same sum in Python integers; the two phases, on bytes, with the existing single-polynomial calls on the host-combined vectors
(kzg_commit_eval / kzg_open_eval / kzg_eval_form_eval / kzg_quotient_eval_at, kzg_commit_coeff / kzg_witness_coeff / kzg_poly_eval) and,
at small sizes, with the big-int model (tests/multiopen_model.py); the verifier with the model's verdicts and with kzg_verify_eval on
E - D.  Like the fold file this one sorts after the tests that release the session's contexts, so it opens and closes its own
module-scoped Engine."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars, unpack_scalars
from oracle import kzg_model as M
from tests import multiopen_model as MO
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
AFF = L.G1_AFFINE_MONT
TAU = 0x0123456789ABCDEF0FEDCBA987654321
A5 = b"\xa5"
UNTOUCHED = -7
SH = L.KZG_ERR_SHAPE


def le(v):
    return (v % R).to_bytes(32, "little")


def raw32(v):
    return int(v).to_bytes(32, "little")


def omega(d):
    return M.compute_omega(d)[2]


def points_for(d, rng):
    w = omega(d)
    return [rng.randrange(R), 0, 1, w, R - 1, pow(w, d - 1, R), omega(2 * d), 7]


def u32s(xs):
    return None if xs is None else (ctypes.c_uint32 * max(len(xs), 1))(*xs)


def flat(vecs):
    return [x for v in vecs for x in v]


def fresh(rng, zs):
    t = rng.randrange(R)
    while t in zs:
        t = rng.randrange(R)
    return t


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
def lincomb_raw(eng, vecs, d, n_vecs, idx, weights, sfmt=CAN, flags=0, out=None):
    """(rc, out bytes or None); vecs / weights: bytes (or a device pointer for vecs)"""
    buf = out if out is not None else ctypes.create_string_buffer(A5 * (32 * d), 32 * d)
    rc = eng.lib.kzg_fr_lincomb(eng.ctx, vecs, d, n_vecs, u32s(idx), weights, len(idx), sfmt, flags, buf)
    return rc, (buf.raw if out is None else None)


def lincomb_case(rng, n_vecs, count, case):
    """repeated and permuted indices; weights 0, 1, R - 1 and random"""
    menu = [0, 1, R - 1, rng.randrange(R)]
    idx = [rng.randrange(n_vecs) for _ in range(count)]
    if count >= 3:
        idx[1] = idx[0]                      # a vector named twice
        idx[2] = n_vecs - 1
    return idx, [menu[(k + case) % 4] for k in range(count)]


@pytest.mark.parametrize("d", [1, 2, 255, 256, 257, 512, 1 << 13])
def test_lincomb_kernel_against_python_integers(eng, d):
    rng = random.Random(900 + d)
    n_vecs = 5
    vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(n_vecs)]
    vecs[1], vecs[4] = [0] * d, [R - 1] * d
    blob = pack_scalars(flat(vecs))
    for case, count in enumerate((1, 2, 3, 17, 33)):
        idx, weights = lincomb_case(rng, n_vecs, count, case)
        rc, got = lincomb_raw(eng, blob, d, n_vecs, idx, pack_scalars(weights))
        assert rc == 0, eng.last_error()
        assert got == pack_scalars(MO.lincomb(vecs, idx, weights)), (d, count)
    rc, got = lincomb_raw(eng, blob, d, n_vecs, [], b"")  # no term: zero
    assert rc == 0 and got == bytes(32 * d)


def test_lincomb_formats_device_buffers_and_residues(eng):
    rng = random.Random(91)
    d, n_vecs, count = 257, 4, 17
    vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(n_vecs)]
    idx, weights = lincomb_case(rng, n_vecs, count, 3)
    want = MO.lincomb(vecs, idx, weights)
    n_in, n_out = n_vecs * d * 32, d * 32
    d_in, d_out = dev_buffer(eng, n_in), dev_buffer(eng, n_out + 32)
    try:
        for sfmt, k in ((CAN, 1), (MONT, MONT_R)):
            blob = pack_scalars([x * k % R for x in flat(vecs)])
            wb = pack_scalars([w * k % R for w in weights])
            expect = pack_scalars([x * k % R for x in want])
            assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, n_in) == 0
            for in_dev in (0, L.IN_DEVICE):
                src = d_in if in_dev else blob
                rc, got = lincomb_raw(eng, src, d, n_vecs, idx, wb, sfmt, in_dev)
                assert rc == 0 and got == expect, (sfmt, in_dev)
                assert eng.lib.kzg_dev_upload(eng.ctx, d_out, A5 * (n_out + 32), n_out + 32) == 0
                rc, _ = lincomb_raw(eng, src, d, n_vecs, idx, wb, sfmt, in_dev | L.OUT_DEVICE, out=d_out)
                back = dev_download(eng, d_out, n_out + 32)
                assert rc == 0 and back[:n_out] == expect and back[n_out:] == A5 * 32, (sfmt, in_dev)  # nothing behind the last sum
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)
        eng.lib.kzg_dev_free(eng.ctx, d_out)
    # canonical inputs of any 256-bit value count as their residues
    big = [R, R + 5, (1 << 256) - 1, 2 * R, 2 * R + 1, R - 1, 0]
    vecs = [[big[(i + j) % len(big)] if (i + j) % 3 else rng.randrange(1 << 256) for j in range(d)] for i in range(n_vecs)]
    rc, got = lincomb_raw(eng, b"".join(raw32(x) for x in flat(vecs)), d, n_vecs, idx, pack_scalars(weights))
    assert rc == 0 and got == pack_scalars(MO.lincomb(vecs, idx, weights))
    # the Python surface, with the carry of a host input staged vector by vector behind it
    assert eng.fr_lincomb(flat(vecs), d, idx, weights) == MO.lincomb(vecs, idx, weights)


def test_lincomb_host_input_staged_in_pieces_with_carry(eng):
    """count x d x 32 bytes of named vectors beyond one staging piece (64 MiB): the running sum is carried on the device between the
    pieces.  The columns at the block edges and a random sample are compared."""
    rng = random.Random(92)
    d, n_vecs, count = (1 << 17) + 1, 3, 17
    blob = rng.randbytes(32 * n_vecs * d)  # any 256-bit values: their residues count
    idx = [k % n_vecs for k in range(count)]
    weights = [rng.randrange(R) for _ in range(count)]
    rc, got = lincomb_raw(eng, blob, d, n_vecs, idx, pack_scalars(weights))
    assert rc == 0, eng.last_error()
    cols = [0, 1, 255, 256, 257, d - 257, d - 2, d - 1] + [rng.randrange(d) for _ in range(56)]
    for j in cols:
        col = [[int.from_bytes(blob[32 * (i * d + j):32 * (i * d + j) + 32], "little")] for i in range(n_vecs)]
        assert got[32 * j:32 * j + 32] == le(MO.lincomb(col, idx, weights)[0]), j


def test_lincomb_shape_errors_leave_the_output_untouched(eng):
    d, blob, one = 4, pack_scalars(range(8)), le(1)
    bad = [
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, blob, 0, 2, u32s([0]), one, 1, CAN, 0, b),          # d == 0
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, blob, d, 2, u32s([2]), one, 1, CAN, 0, b),          # index out of range
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, blob, d, 2, u32s([0]), raw32(R), 1, CAN, 0, b),     # weight >= modulus
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, blob, d, 2, u32s([0]), one, 1, 77, 0, b),           # unknown format
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, None, d, 2, u32s([0]), one, 1, CAN, 0, b),          # NULL vecs
        lambda b: eng.lib.kzg_fr_lincomb(eng.ctx, blob, d, 2, None, one, 1, CAN, 0, b),               # NULL idx
    ]
    for i, call in enumerate(bad):
        buf = ctypes.create_string_buffer(A5 * (32 * d), 32 * d)
        assert call(buf) == SH and buf.raw == A5 * (32 * d), i
    assert eng.lib.kzg_fr_lincomb(eng.ctx, blob, d, 2, u32s([0]), one, 1, CAN, 0, None) == SH


# ---- 2. evaluation form ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lags(eng):
    """lags(d) -> setup_lagrange(TAU, d), built once per size"""
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = kzg_amd.setup_lagrange(eng, TAU, d)
        return cache[d]
    yield get
    for lag in cache.values():
        lag.free()


@pytest.fixture(scope="module")
def params(eng):
    """the monomial parameters of the same tau, long enough for n = 2^13 + 1 coefficients"""
    p = kzg_amd.setup(eng, TAU, (1 << 13) + 1, g2_len=2)
    yield p
    p.gs.free()
    p.hs.free()


def commit_raw(fn, eng, srs, blob, length, n_polys, idx, zs, r, glen, sfmt=CAN, flags=0, g_out=None, d_out=None, ofmt=AFF):
    """(rc, ys, g, D) of a first phase, every host output pre-filled with 0xA5; zs, r: ints"""
    count, psz = len(zs), L.POINT_BYTES[ofmt]
    k = MONT_R if sfmt == MONT else 1
    ys = ctypes.create_string_buffer(A5 * (32 * count + 32), 32 * count + 32)
    g = g_out if g_out is not None else ctypes.create_string_buffer(A5 * (32 * glen + 32), 32 * glen + 32)
    D = d_out if d_out is not None else ctypes.create_string_buffer(A5 * psz, psz)
    rc = fn(eng.ctx, srs.handle, blob, length, n_polys, u32s(idx), b"".join(le(z * k) for z in zs), count, le(r * k), sfmt, flags, ys, g, D, ofmt)
    assert ys.raw[32 * count:] == A5 * 32 and (g_out is not None or g.raw[32 * glen:] == A5 * 32)  # nothing behind the outputs
    return rc, ys.raw[:32 * count], (None if g_out is not None else g.raw[:32 * glen]), (None if d_out is not None else D.raw)


def finish_raw(fn, eng, srs, blob, length, n_polys, idx, zs, r, t, g, sfmt=CAN, flags=0, pi_out=None, ofmt=AFF):
    """(rc, v(t), pi) of a second phase; g: bytes or a device pointer"""
    count, psz = len(zs), L.POINT_BYTES[ofmt]
    k = MONT_R if sfmt == MONT else 1
    y = ctypes.create_string_buffer(A5 * 32, 32)
    pi = pi_out if pi_out is not None else ctypes.create_string_buffer(A5 * psz, psz)
    rc = fn(eng.ctx, srs.handle, blob, length, n_polys, u32s(idx), b"".join(le(z * k) for z in zs), count, le(r * k), le(t * k), g, sfmt, flags, y, pi, ofmt)
    return rc, y.raw, (None if pi_out is not None else pi.raw)


def commit_eval_bytes(eng, lag, vec):
    out = ctypes.create_string_buffer(96)
    assert eng.lib.kzg_commit_eval(eng.ctx, lag.handle, pack_scalars(vec), len(vec), CAN, 0, out, AFF) == 0, eng.last_error()
    return out.raw


def open_eval_raw(eng, lag, vec, z):
    """(y bytes, witness bytes) of kzg_open_eval for one vector"""
    ys, ws = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    assert eng.lib.kzg_open_eval(eng.ctx, lag.handle, pack_scalars(vec), len(vec), 1, le(z), CAN, 0, ys, ws, AFF) == 0, eng.last_error()
    return ys.raw, ws.raw


def eval_expect(eng, lag, evals, idx, zs, r, t):
    """(ys, g, D, v(t), pi as bytes) from the single-polynomial calls: per distinct (polynomial, point) the value and the quotient of
    kzg_quotient_eval_at, combined in Python integers into g and v; D = kzg_commit_eval(g), (v(t), pi) = kzg_open_eval(v, t)"""
    d, n_polys = len(evals[0]), len(evals)
    idx = list(range(len(zs))) if idx is None else idx
    cache, ys, g = {}, [], [0] * d
    for k, (m, z) in enumerate(zip(idx, zs)):
        if (m, z) not in cache:
            y, q = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * d)
            assert eng.lib.kzg_quotient_eval_at(eng.ctx, pack_scalars(evals[m]), d, le(z), CAN, 0, y, q) == 0, eng.last_error()
            cache[(m, z)] = (int.from_bytes(y.raw, "little"), unpack_scalars(q.raw))
        y, q = cache[(m, z)]
        ys.append(y)
        rk = pow(r, k, R)
        g = [(a + rk * b) % R for a, b in zip(g, q)]
    assert ys == eng.eval_form_eval([evals[m] for m in idx], zs)  # the values of kzg_eval_form_eval
    w, W = MO.poly_weights(zs, idx, n_polys, r, t)
    v = MO.lincomb(evals, range(n_polys), W, carry=[(R - x) % R for x in g])
    vt, pi = open_eval_raw(eng, lag, v, t)
    assert vt == le(sum(a * b for a, b in zip(w, ys)))  # v(t) = g2
    return pack_scalars(ys), pack_scalars(g), commit_eval_bytes(eng, lag, g), vt, pi


def check_eval(eng, lag, evals, idx, zs, r, t, expect=None, blob=None, sfmt=CAN, flags=0):
    d, n_polys = len(evals[0]), len(evals)
    want = expect or eval_expect(eng, lag, evals, idx, zs, r, t)
    k = MONT_R if sfmt == MONT else 1
    src = blob if blob is not None else pack_scalars([x * k % R for x in flat(evals)])
    conv = (lambda b: pack_scalars([x * k % R for x in unpack_scalars(b)]))
    rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, src, d, n_polys, idx, zs, r, d, sfmt, flags & ~L.IN_DEVICE if blob is None else flags)
    assert rc == 0, eng.last_error()
    assert ys == conv(want[0]) and g == conv(want[1]) and D == want[2], (d, len(zs))
    rc, vt, pi = finish_raw(eng.lib.kzg_multiopen_eval_finish, eng, lag, src, d, n_polys, idx, zs, r, t, g, sfmt, 0 if blob is None else flags)
    assert rc == 0, eng.last_error()
    assert vt == conv(want[3]) and pi == want[4], (d, len(zs))
    return want


@pytest.mark.parametrize("d", [1, 2, 256, 512, 2048, 1 << 13])
def test_eval_form_against_the_single_polynomial_calls(eng, lags, d):
    """nine claims on three polynomials at the points of the fold tests' menu (on and off the domain, shared and not); t off the domain
    and on it"""
    rng = random.Random(1000 + d)
    lag = lags(d)
    evals = [[rng.randrange(R) for _ in range(d)] for _ in range(3)]
    pts = points_for(d, rng)
    zs = [pts[k % len(pts)] for k in range(9)]
    idx = [0, 1, 2, 2, 1, 0, 0, 0, 2]
    r = rng.randrange(1, R)
    want = check_eval(eng, lag, evals, idx, zs, r, fresh(rng, zs))
    on = [pow(omega(d), m, R) for m in range(min(d, 4))]
    t_on = [x for x in on if x not in zs]
    if t_on:  # t on the domain (none is left at d = 1, 2)
        check_eval(eng, lag, evals, idx, zs, r, t_on[-1])
    if d <= 64 or d == 256:  # the big-int model end to end
        mys, mg = MO.commit_eval(evals, idx, zs, r)
        assert want[0] == pack_scalars(mys) and want[1] == pack_scalars(mg)


@pytest.fixture(scope="module")
def polys64(eng, lags):
    rng = random.Random(101)
    d = 64
    return d, lags(d), [[rng.randrange(R) for _ in range(d)] for _ in range(40)]


def test_eval_form_one_claim_is_the_plain_opening(eng, polys64):
    d, lag, evals = polys64
    rng = random.Random(102)
    for z in (rng.randrange(R), pow(omega(d), 9, R)):
        r = rng.randrange(1, R)
        rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, pack_scalars(evals[3]), d, 1, None, [z], r, d)
        assert rc == 0, eng.last_error()
        assert (ys, D) == open_eval_raw(eng, lag, evals[3], z)  # D is kzg_open_eval's witness of that polynomial
        check_eval(eng, lag, [evals[3]], None, [z], r, fresh(rng, [z]))


def test_eval_form_all_claims_at_one_point_is_the_folded_witness(eng, polys64):
    d, lag, evals = polys64
    rng = random.Random(103)
    t_polys = 5
    for z in (rng.randrange(R), pow(omega(d), 63, R)):
        r = rng.randrange(1, R)
        rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, pack_scalars(flat(evals[:t_polys])), d, t_polys, None, [z] * t_polys, r, d)
        assert rc == 0, eng.last_error()
        fy, fw = ctypes.create_string_buffer(32 * t_polys), ctypes.create_string_buffer(96)
        assert eng.lib.kzg_open_fold_eval(eng.ctx, lag.handle, pack_scalars(flat(evals[:t_polys])), d, t_polys, 1, le(z), le(r), CAN, 0, fy, fw, AFF) == 0
        assert ys == fy.raw and D == fw.raw  # kzg_open_fold_eval's witness with gamma = r
        check_eval(eng, lag, evals[:t_polys], None, [z] * t_polys, r, fresh(rng, [z]))


@pytest.mark.parametrize("n_points", [16, 17, 33])
def test_eval_form_distinct_points_across_the_chunk_of_sixteen(eng, polys64, n_points):
    d, lag, evals = polys64
    rng = random.Random(110 + n_points)
    zs = [rng.randrange(R) for _ in range(n_points)]
    zs[5] = pow(omega(d), 5, R)  # one on the domain among them
    idx = [rng.randrange(4) for _ in range(n_points)]
    check_eval(eng, lag, evals[:4], idx, zs, rng.randrange(1, R), fresh(rng, zs))
    check_eval(eng, lag, evals[:n_points], None, zs, rng.randrange(1, R), fresh(rng, zs))  # identity indices


@pytest.mark.parametrize("chunk", [1, 3])
def test_eval_form_lowered_points_chunk(eng, polys64, chunk):
    d, lag, evals = polys64
    rng = random.Random(120)
    pts = [rng.randrange(R) for _ in range(7)]
    zs = [pts[k % 7] for k in range(12)]
    idx = [rng.randrange(3) for _ in range(12)]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    want = check_eval(eng, lag, evals[:3], idx, zs, r, t)
    eng.set_option("multiopen_points_chunk", chunk)
    try:
        check_eval(eng, lag, evals[:3], idx, zs, r, t, expect=want)
    finally:
        eng.set_option("multiopen_points_chunk", 0)
    with pytest.raises(kzg_amd.ReferencePanic):
        eng.set_option("multiopen_points_chunk", 17)


def test_eval_form_points_of_the_domain_only(eng, lags):
    """the Verkle shape: d = 256, every claim at a point of the domain"""
    rng = random.Random(130)
    d = 256
    lag = lags(d)
    evals = [[rng.randrange(R) for _ in range(d)] for _ in range(4)]
    ms = [0, 1, 255, 128, 77, 1, 0, 200, 255, 3]
    zs = [pow(omega(d), m, R) for m in ms]
    idx = [k % 4 for k in range(len(ms))]
    want = check_eval(eng, lag, evals, idx, zs, rng.randrange(1, R), fresh(rng, zs))
    assert want[0] == pack_scalars([evals[i][m] for i, m in zip(idx, ms)])


def test_eval_form_one_polynomial_many_points_many_polynomials_one_point(eng, polys64):
    d, lag, evals = polys64
    rng = random.Random(140)
    zs = points_for(d, rng) + [rng.randrange(R) for _ in range(4)]
    check_eval(eng, lag, evals[:1], [0] * len(zs), zs, rng.randrange(1, R), fresh(rng, zs))
    z = rng.randrange(R)
    idx = [rng.randrange(40) for _ in range(150)]  # more claims at one point than the block that sums their values has lanes
    check_eval(eng, lag, evals, idx, [z] * 150, rng.randrange(1, R), fresh(rng, [z]))


def test_eval_form_formats_device_buffers_and_null_outputs(eng, polys64):
    d, lag, evals = polys64
    rng = random.Random(150)
    evals = evals[:3]
    pts = points_for(d, rng)
    zs, idx = [pts[k % 8] for k in range(10)], [k % 3 for k in range(10)]
    r, t = rng.randrange(1, R), fresh(rng, pts)
    want = check_eval(eng, lag, evals, idx, zs, r, t)
    check_eval(eng, lag, evals, idx, zs, r, t, expect=want, sfmt=MONT)
    n_in = 3 * d * 32
    d_in, d_g, d_pt = dev_buffer(eng, n_in), dev_buffer(eng, d * 32 + 32), dev_buffer(eng, 96 + 32)
    try:
        for sfmt, k in ((CAN, 1), (MONT, MONT_R)):
            conv = (lambda b: pack_scalars([x * k % R for x in unpack_scalars(b)]))
            assert eng.lib.kzg_dev_upload(eng.ctx, d_in, conv(pack_scalars(flat(evals))), n_in) == 0
            assert eng.lib.kzg_dev_upload(eng.ctx, d_g, A5 * (d * 32 + 32), d * 32 + 32) == 0
            assert eng.lib.kzg_dev_upload(eng.ctx, d_pt, A5 * 128, 128) == 0
            rc, ys, _, _ = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, d_in, d, 3, idx, zs, r, d, sfmt, L.IN_DEVICE | L.OUT_DEVICE, g_out=d_g, d_out=d_pt)
            assert rc == 0, eng.last_error()
            back = dev_download(eng, d_g, d * 32 + 32)
            assert ys == conv(want[0]) and back == conv(want[1]) + A5 * 32
            assert dev_download(eng, d_pt, 128) == want[2] + A5 * 32
            rc, vt, _ = finish_raw(eng.lib.kzg_multiopen_eval_finish, eng, lag, d_in, d, 3, idx, zs, r, t, d_g, sfmt, L.IN_DEVICE | L.OUT_DEVICE, pi_out=d_pt)
            assert rc == 0, eng.last_error()
            assert vt == conv(want[3]) and dev_download(eng, d_pt, 128) == want[4] + A5 * 32
    finally:
        for p in (d_in, d_g, d_pt):
            eng.lib.kzg_dev_free(eng.ctx, p)
    # each output alone
    fn, blob, zb = eng.lib.kzg_multiopen_eval_commit, pack_scalars(flat(evals)), b"".join(le(z) for z in zs)
    ys, g, D = ctypes.create_string_buffer(320), ctypes.create_string_buffer(32 * d), ctypes.create_string_buffer(96)
    assert fn(eng.ctx, lag.handle, blob, d, 3, u32s(idx), zb, 10, le(r), CAN, 0, ys, None, None, AFF) == 0 and ys.raw == want[0]
    assert fn(eng.ctx, lag.handle, blob, d, 3, u32s(idx), zb, 10, le(r), CAN, 0, None, g, None, AFF) == 0 and g.raw == want[1]
    assert fn(eng.ctx, lag.handle, blob, d, 3, u32s(idx), zb, 10, le(r), CAN, 0, None, None, D, AFF) == 0 and D.raw == want[2]
    assert fn(eng.ctx, lag.handle, blob, d, 3, u32s(idx), zb, 10, le(r), CAN, 0, None, None, None, AFF) == SH
    # no claim: g zeroed, D and pi the identity
    ident = eng.g1_sum([])
    rc, ys, g, D = commit_raw(fn, eng, lag, None, d, 0, None, [], r, d)
    assert rc == 0 and g == bytes(32 * d) and D == ident
    rc, vt, pi = finish_raw(eng.lib.kzg_multiopen_eval_finish, eng, lag, None, d, 0, None, [], r, t, g)
    assert rc == 0 and vt == bytes(32) and pi == ident


def test_eval_form_shape_errors_leave_the_outputs_untouched(eng, polys64):
    d, lag, evals = polys64
    blob, idx, zs, r, t = pack_scalars(flat(evals[:2])), [0, 1, 1], [5, 6, 7], 3, 9
    zb = b"".join(le(z) for z in zs)
    cf, ff = eng.lib.kzg_multiopen_eval_commit, eng.lib.kzg_multiopen_eval_finish
    gb = bytes(32 * d)
    commit_bad = {
        "d no power of two": lambda y, g, D: cf(eng.ctx, lag.handle, blob, 48, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "d != srs": lambda y, g, D: cf(eng.ctx, lag.handle, blob, 32, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "z >= modulus": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), le(5) + raw32(R) + le(7), 3, le(r), CAN, 0, y, g, D, AFF),
        "r >= modulus": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, raw32(R + 1), CAN, 0, y, g, D, AFF),
        "r == 0": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, bytes(32), CAN, 0, y, g, D, AFF),
        "index out of range": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s([0, 2, 1]), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL indices, count != n_polys": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, None, zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "scalar format": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), 9, 0, y, g, D, AFF),
        "point format": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, 99),
        "NULL evals": lambda y, g, D: cf(eng.ctx, lag.handle, None, d, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL zs": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), None, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL r": lambda y, g, D: cf(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, None, CAN, 0, y, g, D, AFF),
        "NULL srs": lambda y, g, D: cf(eng.ctx, None, blob, d, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
    }
    finish_bad = {
        "t equals a z": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), le(6), gb, CAN, 0, y, D, AFF),
        "t >= modulus": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), raw32(R), gb, CAN, 0, y, D, AFF),
        "NULL t": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), None, gb, CAN, 0, y, D, AFF),
        "NULL g": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, le(r), le(t), None, CAN, 0, y, D, AFF),
        "r == 0": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s(idx), zb, 3, bytes(32), le(t), gb, CAN, 0, y, D, AFF),
        "index out of range": lambda y, g, D: ff(eng.ctx, lag.handle, blob, d, 2, u32s([0, 1, 7]), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
        "d != srs": lambda y, g, D: ff(eng.ctx, lag.handle, blob, 128, 2, u32s(idx), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
    }
    for name, call in list(commit_bad.items()) + list(finish_bad.items()):
        y, g, D = (ctypes.create_string_buffer(A5 * n, n) for n in (96, 32 * d, 96))
        assert call(y, g, D) == SH, name
        assert y.raw == A5 * 96 and g.raw == A5 * (32 * d) and D.raw == A5 * 96, name


def test_eval_form_two_threads_on_one_context(eng, polys64):
    d, lag, evals = polys64
    rng = random.Random(160)
    jobs = []
    for j in range(2):
        zs = [rng.randrange(R) for _ in range(5)] + [pow(omega(d), 3 + j, R)]
        idx = [rng.randrange(3) for _ in range(6)]
        r, t = rng.randrange(1, R), fresh(rng, zs)
        jobs.append((idx, zs, r, t, eval_expect(eng, lag, evals[:3], idx, zs, r, t)))
    blob, out = pack_scalars(flat(evals[:3])), {}

    def work(name, job):
        idx, zs, r, t, want = job
        res = []
        for _ in range(3):
            rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, blob, d, 3, idx, zs, r, d)
            rc2, vt, pi = finish_raw(eng.lib.kzg_multiopen_eval_finish, eng, lag, blob, d, 3, idx, zs, r, t, g)
            res.append((rc, rc2, (ys, g, D, vt, pi) == want))
        out[name] = res
    threads = [threading.Thread(target=work, args=(n, j)) for n, j in zip("ab", jobs)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert out == {"a": [(0, 0, True)] * 3, "b": [(0, 0, True)] * 3}, out


def test_eval_form_one_msm_per_call(eng, lags):
    """with profiling on, a first phase of 33 claims launches the accumulation kernel as often as ONE kzg_commit_eval at the same d;
    so does a second phase"""
    rng = random.Random(170)
    d = 2048
    lag = lags(d)
    evals = [[rng.randrange(R) for _ in range(d)] for _ in range(3)]
    zs = [rng.randrange(R) for _ in range(33)]
    idx = [k % 3 for k in range(33)]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    blob = pack_scalars(flat(evals))
    eng.prof_enable(True)
    try:
        eng.prof_reset()
        commit_eval_bytes(eng, lag, evals[0])
        one = eng.prof_get("k_accum_affine")[0]
        eng.prof_reset()
        rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_eval_commit, eng, lag, blob, d, 3, idx, zs, r, d)
        first = eng.prof_get("k_accum_affine")[0]
        passes = eng.prof_get("k_multiopen_accum")[0]
        eng.prof_reset()
        rc2, vt, pi = finish_raw(eng.lib.kzg_multiopen_eval_finish, eng, lag, blob, d, 3, idx, zs, r, t, g)
        second = eng.prof_get("k_accum_affine")[0]
    finally:
        eng.prof_enable(False)
    assert rc == 0 and rc2 == 0, eng.last_error()
    assert one > 0 and first == one and second == one, (one, first, second)
    assert passes == 3  # 33 distinct points: chunks of 16, 16, 1


# ---- 3. coefficient form -------------------------------------------------------------------------------------------------------------
def coeff_expect(eng, params, polys, idx, zs, r, t):
    """(ys, g, D, v(t), pi) from kzg_poly_eval, kzg_commit_coeff and kzg_witness_coeff on the host-combined polynomials"""
    n = len(polys[0])
    ys, g = MO.commit_coeff(polys, idx, zs, r)
    ii = list(range(len(zs))) if idx is None else idx
    assert ys == [eng.poly_eval(polys[m], z) for m, z in zip(ii, zs)]
    w, W = MO.poly_weights(zs, idx, len(polys), r, t)
    v = [(a - b) % R for a, b in zip(MO.lincomb(polys, range(len(polys)), W), g + [0])]
    vt = MO.poly_eval(v, t)
    assert vt == sum(a * b for a, b in zip(w, ys)) % R
    if n == 1:  # no quotient: both elements are the identity
        return pack_scalars(ys), b"", eng.g1_sum([]), le(vt), eng.g1_sum([])
    D, pi = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
    assert eng.lib.kzg_commit_coeff(eng.ctx, params.gs.handle, pack_scalars(g), n - 1, CAN, 0, D, AFF) == 0, eng.last_error()
    assert eng.lib.kzg_witness_coeff(eng.ctx, params.gs.handle, pack_scalars(v), n, le(t), le(vt), CAN, 0, pi, AFF) == 0, eng.last_error()
    return pack_scalars(ys), pack_scalars(g), D.raw, le(vt), pi.raw


@pytest.mark.parametrize("n", [1, 2, 300, (1 << 13) + 1])
def test_coeff_form_against_the_single_polynomial_calls(eng, params, n):
    rng = random.Random(2000 + n)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    pts = [rng.randrange(R), 0, 1, R - 1]
    zs = [pts[k % 4] for k in range(7)]
    idx = [0, 1, 2, 2, 1, 0, 0]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    want = coeff_expect(eng, params, polys, idx, zs, r, t)
    blob = pack_scalars(flat(polys))
    rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_coeff_commit, eng, params.gs, blob, n, 3, idx, zs, r, n - 1)
    assert rc == 0, eng.last_error()
    assert (ys, g, D) == want[:3], n
    rc, vt, pi = finish_raw(eng.lib.kzg_multiopen_coeff_finish, eng, params.gs, blob, n, 3, idx, zs, r, t, g + bytes(32))
    assert rc == 0, eng.last_error()
    assert (vt, pi) == want[3:], n
    # identity indices, Montgomery form, device buffers
    zs3 = zs[:3]
    want = coeff_expect(eng, params, polys, None, zs3, r, t)
    mont = pack_scalars([x * MONT_R % R for x in flat(polys)])
    d_in, d_g = dev_buffer(eng, len(mont)), dev_buffer(eng, 32 * n + 32)
    try:
        assert eng.lib.kzg_dev_upload(eng.ctx, d_in, mont, len(mont)) == 0
        rc, ys, _, D = commit_raw(eng.lib.kzg_multiopen_coeff_commit, eng, params.gs, d_in, n, 3, None, zs3, r, n - 1, MONT, L.IN_DEVICE, g_out=d_g)
        assert rc == 0, eng.last_error()
        conv = (lambda b: pack_scalars([x * MONT_R % R for x in unpack_scalars(b)]))
        assert ys == conv(want[0]) and D == want[2] and dev_download(eng, d_g, 32 * n + 32) == conv(want[1]) + A5 * 64
        rc, vt, pi = finish_raw(eng.lib.kzg_multiopen_coeff_finish, eng, params.gs, d_in, n, 3, None, zs3, r, t, d_g, MONT, L.IN_DEVICE)
        assert rc == 0, eng.last_error()
        assert vt == conv(want[3]) and pi == want[4]
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)
        eng.lib.kzg_dev_free(eng.ctx, d_g)


def test_coeff_form_shape_errors_leave_the_outputs_untouched(eng, params):
    n = 8
    blob, idx, zs, r, t = pack_scalars(range(16)), [0, 1, 1], [5, 6, 7], 3, 9
    zb = b"".join(le(z) for z in zs)
    cf, ff = eng.lib.kzg_multiopen_coeff_commit, eng.lib.kzg_multiopen_coeff_finish
    gb = bytes(32 * n)
    bad = {
        "n == 0": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, 0, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "n - 1 > srs": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, (1 << 13) + 3, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "r == 0": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, bytes(32), CAN, 0, y, g, D, AFF),
        "index out of range": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s([0, 1, 2]), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL indices": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, None, zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "z >= modulus": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), le(5) + raw32(R) + le(7), 3, le(r), CAN, 0, y, g, D, AFF),
        "r >= modulus": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, raw32(R + 1), CAN, 0, y, g, D, AFF),
        "scalar format": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), 9, 0, y, g, D, AFF),
        "point format": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, 99),
        "NULL coeffs": lambda y, g, D: cf(eng.ctx, params.gs.handle, None, n, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL zs": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), None, 3, le(r), CAN, 0, y, g, D, AFF),
        "NULL r": lambda y, g, D: cf(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, None, CAN, 0, y, g, D, AFF),
        "NULL srs": lambda y, g, D: cf(eng.ctx, None, blob, n, 2, u32s(idx), zb, 3, le(r), CAN, 0, y, g, D, AFF),
        "finish: t >= modulus": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), raw32(R), gb, CAN, 0, y, D, AFF),
        "finish: NULL t": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), None, gb, CAN, 0, y, D, AFF),
        "finish: NULL g": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), le(t), None, CAN, 0, y, D, AFF),
        "finish: NULL coeffs": lambda y, g, D: ff(eng.ctx, params.gs.handle, None, n, 2, u32s(idx), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
        "finish: NULL srs": lambda y, g, D: ff(eng.ctx, None, blob, n, 2, u32s(idx), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
        "finish: r == 0": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, bytes(32), le(t), gb, CAN, 0, y, D, AFF),
        "finish: n - 1 > srs": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, (1 << 13) + 3, 2, u32s(idx), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
        "finish: t equals a z": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), zb, 3, le(r), le(7), gb, CAN, 0, y, D, AFF),
        "finish: n == 0": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, 0, 2, u32s(idx), zb, 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
        "finish: z >= modulus": lambda y, g, D: ff(eng.ctx, params.gs.handle, blob, n, 2, u32s(idx), raw32(R) + zb[32:], 3, le(r), le(t), gb, CAN, 0, y, D, AFF),
    }
    for name, call in bad.items():
        y, g, D = (ctypes.create_string_buffer(A5 * k, k) for k in (96, 32 * n, 96))
        assert call(y, g, D) == SH, name
        assert y.raw == A5 * 96 and g.raw == A5 * (32 * n) and D.raw == A5 * 96, name


# ---- 4. the verifier ---------------------------------------------------------------------------------------------------------------
def verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi, n_commitments=None, sfmt=CAN):
    """(rc, ok) with ok pre-set to UNTOUCHED; zs, ys, r, t: ints (ys may be any 256-bit value)"""
    k = MONT_R if sfmt == MONT else 1
    ok = ctypes.c_int(UNTOUCHED)
    rc = eng.lib.kzg_verify_multiopen(eng.ctx, params.gs.handle, params.hs.handle, b"".join(raw32(z * k % R if z < R else z) for z in zs),
                                      b"".join(raw32(y * k % R if y < R else y) for y in ys), sfmt, b"".join(commitments),
                                      len(commitments) if n_commitments is None else n_commitments, u32s(idx), len(zs),
                                      raw32(r * k % R if r < R else r), raw32(t * k % R if t < R else t), D, pi, AFF, ctypes.byref(ok))
    return rc, ok.value


@pytest.fixture(scope="module")
def proof(eng, params):
    """a coefficient-form proof of nine claims on four polynomials of 24 coefficients, and its model twin"""
    rng = random.Random(300)
    n, n_polys = 24, 4
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(n_polys)]
    pts = [rng.randrange(R) for _ in range(3)]
    zs = [pts[k % 3] for k in range(9)]
    idx = [rng.randrange(n_polys) for _ in range(9)]
    idx[:4] = [0, 1, 2, 3]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    prover = kzg_amd.KZGProver(params)
    commitments = [prover.commit(kzg_amd.Polynomial(p)) for p in polys]
    blob = pack_scalars(flat(polys))
    rc, ys, g, D = commit_raw(eng.lib.kzg_multiopen_coeff_commit, eng, params.gs, blob, n, n_polys, idx, zs, r, n - 1)
    assert rc == 0, eng.last_error()
    rc, vt, pi = finish_raw(eng.lib.kzg_multiopen_coeff_finish, eng, params.gs, blob, n, n_polys, idx, zs, r, t, g + bytes(32))
    assert rc == 0, eng.last_error()
    model = (TAU, [MO.poly_eval(p, TAU) for p in polys]) + MO.prove(polys, idx, zs, r, t, TAU)[1:]
    return polys, idx, zs, unpack_scalars(ys), r, t, commitments, D, pi, int.from_bytes(vt, "little"), model


def test_verifier_accepts_the_honest_proof_and_agrees_with_kzg_verify_eval(eng, params, proof):
    polys, idx, zs, ys, r, t, commitments, D, pi, vt, model = proof
    tau, mc, mD, mpi = model
    assert MO.verdict(tau, mc, idx, zs, ys, r, t, mD, mpi)
    assert verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi) == (0, 1)
    assert verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi, sfmt=MONT) == (0, 1)
    # the same as a plain opening of E - D at (t, g2): E - D from kzg_srs_upload_g1 of the commitments and D + kzg_msm_g1
    w, W = MO.poly_weights(zs, idx, len(polys), r, t)
    g2 = sum(a * b for a, b in zip(w, ys)) % R
    assert g2 == vt
    srs = kzg_amd.Srs.upload(eng, b"".join(commitments) + D, len(commitments) + 1)
    try:
        EmD = eng.msm(srs, W + [R - 1])
    finally:
        srs.free()
    kv = kzg_amd.KZGVerifier(params)
    assert kv.verify_eval((t, g2), EmD, pi) is True
    assert kv.verify_eval((t, (g2 + 1) % R), EmD, pi) is False
    for host_pairing in (0, 1):  # both pairing sites
        eng.set_option("host_pairing", host_pairing)
        try:
            assert verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi) == (0, 1)
            assert verify_raw(eng, params, zs, ys[:8] + [ys[8] + 1], commitments, idx, r, t, D, pi) == (0, 0)
        finally:
            eng.set_option("host_pairing", 1)
    for chunk in (1, 4, 8):  # a lowered chunk: the weights walk across the boundaries
        eng.set_option("verify_eval_batch_chunk", chunk)
        try:
            assert verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi) == (0, 1)
            assert verify_raw(eng, params, zs, [ys[0] + 1] + ys[1:], commitments, idx, r, t, D, pi) == (0, 0)
        finally:
            eng.set_option("verify_eval_batch_chunk", 0)
    # values beyond the modulus count as their residues
    assert verify_raw(eng, params, zs, [ys[0] + R] + ys[1:], commitments, idx, r, t, D, pi) == (0, 1)


def test_verifier_rejects_one_flip_at_a_time(eng, params, proof):
    polys, idx, zs, ys, r, t, commitments, D, pi, vt, model = proof
    tau, mc, mD, mpi = model
    flips = []
    for k in (0, 4, 8):
        flips.append((zs, ys[:k] + [(ys[k] + 1) % R] + ys[k + 1:], commitments, idx, r, t, D, pi))
        flips.append((zs[:k] + [(zs[k] + 1) % R] + zs[k + 1:], ys, commitments, idx, r, t, D, pi))
        flips.append((zs, ys, commitments, idx[:k] + [(idx[k] + 1) % 4] + idx[k + 1:], r, t, D, pi))
    flips.append((zs, ys, [commitments[1]] + commitments[1:], idx, r, t, D, pi))
    flips.append((zs, ys, commitments, idx, r, t, pi, D))
    flips.append((zs, ys, commitments, idx, r, t, D, commitments[0]))
    flips.append((zs, ys, commitments, idx, (r + 1) % R or 1, t, D, pi))
    flips.append((zs, ys, commitments, idx, r, fresh(random.Random(5), zs + [t]), D, pi))
    for i, (z_, y_, c_, i_, r_, t_, D_, pi_) in enumerate(flips):
        assert verify_raw(eng, params, z_, y_, c_, i_, r_, t_, D_, pi_) == (0, 0), i
    # the model says the same of the flips it can express
    assert not MO.verdict(tau, mc, idx, zs, [(ys[0] + 1) % R] + ys[1:], r, t, mD, mpi)
    assert not MO.verdict(tau, mc, idx, zs, ys, r, t, mpi, mD)


def test_verifier_null_indices_and_the_forgery_of_a_predictable_t(eng, params):
    rng = random.Random(310)
    n = 12
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    zs = [rng.randrange(R), rng.randrange(R), 5]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    prover, kv = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    commitments = [prover.commit(kzg_amd.Polynomial(p)) for p in polys]
    ys, D, pi, t_used = prover.multiopen(polys, zs, r, lambda D_: t)
    assert t_used == t and ys == [MO.poly_eval(p, z) for p, z in zip(polys, zs)]
    assert verify_raw(eng, params, zs, ys, commitments, None, r, t, D, pi) == (0, 1)
    assert verify_raw(eng, params, zs, ys, commitments, [0, 1, 2], r, t, D, pi) == (0, 1)
    assert verify_raw(eng, params, zs, ys, commitments[:2], None, r, t, D, pi)[0] == SH  # without indices: one commitment per claim
    # the header's forgery: ONE wrong claim (C, z, y'), t known in advance, pi = identity, D = (C - [y'] gs[0]) / (t - z)
    z, y_wrong = zs[0], (ys[0] + 1) % R
    ident = ctypes.create_string_buffer(eng.g1_sum([]), 96)
    gen = eng.msm(params.gs, [1])
    inv = M.fr_inv((t - z) % R)
    srs = kzg_amd.Srs.upload(eng, commitments[0] + gen, 2)
    try:
        forged_D = eng.msm(srs, [inv, (R - y_wrong) * inv % R])
    finally:
        srs.free()
    assert verify_raw(eng, params, [z], [y_wrong], commitments[:1], None, r, t, forged_D, ident.raw) == (0, 1)  # the forger knew t
    assert verify_raw(eng, params, [z], [y_wrong], commitments[:1], None, r, fresh(rng, zs + [t]), forged_D, ident.raw) == (0, 0)  # t drawn after D
    assert kv.verify_multiopen([z], [ys[0]], commitments[:1], forged_D, ident.raw, r, t) is False


@pytest.fixture(scope="module")
def proof3(eng, params):
    """three claims, one polynomial of 12 coefficients each: the shape without indices"""
    rng = random.Random(330)
    polys = [[rng.randrange(R) for _ in range(12)] for _ in range(3)]
    zs = [rng.randrange(R) for _ in range(3)]
    r, t = rng.randrange(1, R), fresh(rng, zs)
    prover = kzg_amd.KZGProver(params)
    ys, D, pi, _ = prover.multiopen(polys, zs, r, lambda D_: t)
    return zs, ys, [prover.commit(kzg_amd.Polynomial(p)) for p in polys], r, t, D, pi


@pytest.mark.parametrize("chunk", [1, 2])
def test_verifier_null_indices_at_a_lowered_chunk(eng, params, proof3, chunk):
    """one commitment per claim goes into the third bucket set chunk by chunk: three claims in chunks of 1 and of 2"""
    zs, ys, commitments, r, t, D, pi = proof3
    eng.set_option("verify_eval_batch_chunk", chunk)
    try:
        assert verify_raw(eng, params, zs, ys, commitments, None, r, t, D, pi) == (0, 1)
        assert verify_raw(eng, params, zs, ys[:2] + [(ys[2] + 1) % R], commitments, None, r, t, D, pi) == (0, 0)
    finally:
        eng.set_option("verify_eval_batch_chunk", 0)


def test_verifier_malformed_points_and_shape_errors_leave_ok_unwritten(eng, params, proof):
    polys, idx, zs, ys, r, t, commitments, D, pi, vt, model = proof
    off_curve = (1).to_bytes(48, "little") * 2
    for args in ((commitments, off_curve, pi), (commitments, D, off_curve), ([commitments[0], off_curve] + commitments[2:], D, pi)):
        assert verify_raw(eng, params, zs, ys, args[0], idx, r, t, args[1], args[2]) == (L.KZG_ERR_BAD_POINT, UNTOUCHED)
    bad = [
        (zs, ys, commitments, idx, r, zs[4], D, pi),                    # t equals a z_k
        (zs, ys, commitments, idx, r, R, D, pi),                        # t >= modulus
        (zs, ys, commitments, idx, 0, t, D, pi),                        # r == 0
        (zs, ys, commitments, idx, R + 2, t, D, pi),                    # r >= modulus
        (zs[:8] + [R], ys, commitments, idx, r, t, D, pi),              # z >= modulus
        (zs, ys, commitments, idx[:8] + [4], r, t, D, pi),              # index out of range
        (zs, ys, commitments, None, r, t, D, pi),                       # NULL indices, count != n_commitments
        (zs, ys, commitments, idx, r, t, None, pi),                     # NULL D
        (zs, ys, commitments, idx, r, t, D, None),                      # NULL pi
    ]
    for i, a in enumerate(bad):
        assert verify_raw(eng, params, *a) == (SH, UNTOUCHED), i
    assert verify_raw(eng, params, zs, ys, commitments, idx, r, t, D, pi, sfmt=5) == (SH, UNTOUCHED)
    assert verify_raw(eng, params, [], [], [], None, r, t, D, pi) == (0, 1)  # no claim


def test_eval_form_proofs_verify_against_the_monomial_parameters(eng, params, lags):
    rng = random.Random(320)
    d = 64
    lag = lags(d)
    eprover = kzg_amd.KZGProverEvalForm(params, lag)
    kv = kzg_amd.KZGVerifierEvalForm(params, lag)
    evals = [[rng.randrange(R) for _ in range(d)] for _ in range(4)]
    commitments = [commit_eval_bytes(eng, lag, v) for v in evals]
    pts = points_for(d, rng)
    zs = [pts[k % 8] for k in range(11)]
    idx = [rng.randrange(4) for _ in range(11)]
    r = rng.randrange(1, R)
    seen = []

    def challenge_t(D):
        seen.append(D)
        return int.from_bytes(D[:31], "little") % R  # "a hash that includes D"
    ys, D, pi, t = eprover.multiopen(evals, zs, r, challenge_t, poly_idx=idx)
    assert seen == [D] and t == int.from_bytes(D[:31], "little") % R
    assert ys == eng.eval_form_eval([evals[m] for m in idx], zs)
    assert kv.verify_multiopen(zs, ys, commitments, D, pi, r, t, commitment_idx=idx) is True
    assert kv.verify_multiopen(zs, ys[:10] + [(ys[10] + 1) % R], commitments, D, pi, r, t, commitment_idx=idx) is False
    assert kv.verify_multiopen(zs, ys, commitments, D, pi, r, (t + 1) % R, commitment_idx=idx) is False
    # the phases one by one, device-resident: g stays in HBM between them
    buf = eng.alloc_scalars(4 * d)
    buf.upload(pack_scalars(flat(evals)))
    try:
        ys2, g, D2 = eprover.multiopen_commit(buf, zs, r, poly_idx=idx)
        assert isinstance(g, kzg_amd.api.DeviceBuffer) and (ys2, D2) == (ys, D)
        pi2, vt = eprover.multiopen_finish(buf, zs, r, t, g, poly_idx=idx)
        g.free()
        w, W = MO.poly_weights(zs, idx, 4, r, t)
        assert pi2 == pi and vt == sum(a * b for a, b in zip(w, ys)) % R
    finally:
        buf.free()
    with pytest.raises(kzg_amd.ReferencePanic):
        eprover.multiopen(evals, zs, r, lambda D_: zs[3], poly_idx=idx)  # t equal to a z_k: the caller draws another
    with pytest.raises(kzg_amd.ReferencePanic):
        eprover.multiopen_commit(evals, zs, -1, poly_idx=idx)  # no 256-bit unsigned value
    with pytest.raises(kzg_amd.ReferencePanic):
        eprover.multiopen_commit(evals, zs, R, poly_idx=idx)  # the library refuses r >= modulus


# ---- 5. the C++ mirror -----------------------------------------------------------------------------------------------------------------
def test_cpp_wrapper(tmp_path):
    """fr_lincomb, multiopen_commit / multiopen_finish and verify_multiopen of include/kzg_mi355x.hpp: tests/cpp_multiopen_test.cpp
    against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_multiopen_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_multiopen_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
