"""kzg_fr_fold / kzg_open_fold_eval / kzg_open_fold_coeff / kzg_verify_fold (kzg_amd/csrc/fold.hip, capi.hip, verify_eval_batch.hip):
many polynomials opened at one point with a single folded witness.  The fold is compared with the same sum in Python integers; the
openings, on bytes, with the existing single-polynomial calls on the host-folded polynomial (kzg_open_eval, kzg_witness_eval,
kzg_witness_coeff, kzg_eval_form_eval, kzg_poly_eval, kzg_g1_sum) and, at d <= 64, with the big-int model (tests/open_fold_model.py);
the verifier with the model's verdicts and with kzg_verify_eval on the folded commitment.  Like the FK20 files this one sorts after
the tests that release the session's contexts, so it opens and closes its own module-scoped Engine."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars, unpack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import open_fold_model as FM
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng, hooks  # noqa: F401 -- this module's fixtures

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


def log2(d):
    return d.bit_length() - 1


def omega(d):
    return M.compute_omega(d)[2]


def points_for(d, rng):
    w = omega(d)
    return [rng.randrange(R), 0, 1, w, R - 1, pow(w, d - 1, R), omega(2 * d), 7]


def domain_index(d, z):
    """m with z = w^m, or None"""
    w, x = omega(d), 1
    for m in range(d):
        if x == z % R:
            return m
        x = x * w % R
    return None


def gammas_for(rng, groups, shift=0):
    menu = [1, 2, R - 1, rng.randrange(2, R)]
    return [menu[(g + shift) % 4] for g in range(groups)]


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
def fold_raw(eng, vecs, d, t, gammas, sfmt=CAN, flags=0, out=None):
    """(rc, out bytes or None); vecs / gammas: bytes (or a device pointer for vecs)"""
    groups = len(gammas) // 32
    buf = out if out is not None else ctypes.create_string_buffer(A5 * (32 * groups * d), 32 * groups * d)
    rc = eng.lib.kzg_fr_fold(eng.ctx, vecs, d, t, groups, gammas, sfmt, flags, buf)
    return rc, (buf.raw if out is None else None)


def fold_vectors(rng, d, t, groups):
    """groups x t vectors: random ones, with an all-zero and an all-(R - 1) vector among them when there is room"""
    vecs = [[[rng.randrange(R) for _ in range(d)] for _ in range(t)] for _ in range(groups)]
    if t >= 3:
        vecs[0][1] = [0] * d
        vecs[-1][t - 1] = [R - 1] * d
    return vecs


def flat(vecs):
    return [x for grp in vecs for v in grp for x in v]


@pytest.mark.parametrize("d", [1, 2, 255, 256, 257, 512, 1 << 13])
def test_fold_kernel_against_python_integers(eng, d):
    rng = random.Random(700 + d)
    if d < (1 << 13):
        shapes = [(t, groups) for t in (1, 2, 3, 17, 33) for groups in (1, 3)]
    else:  # every t, both group counts
        shapes = [(1, 1), (2, 3), (3, 1), (17, 3), (33, 1)]
    for case, (t, groups) in enumerate(shapes):
        vecs, gammas = fold_vectors(rng, d, t, groups), gammas_for(rng, groups, case)
        want = pack_scalars([x for grp, g in zip(vecs, gammas) for x in FM.fold(grp, g)])
        rc, got = fold_raw(eng, pack_scalars(flat(vecs)), d, t, pack_scalars(gammas))
        assert rc == 0, eng.last_error()
        assert got == want, (d, t, groups)
    # all zero and all R - 1 as whole inputs
    for fill in (0, R - 1):
        rc, got = fold_raw(eng, pack_scalars([fill] * (3 * d)), d, 3, le(R - 1))
        assert rc == 0 and got == pack_scalars(FM.fold([[fill] * d] * 3, R - 1))


def test_fold_formats_and_device_buffers(eng):
    rng = random.Random(71)
    d, t, groups = 257, 17, 3
    vecs, gammas = fold_vectors(rng, d, t, groups), gammas_for(rng, groups, 1)
    want = [x for grp, g in zip(vecs, gammas) for x in FM.fold(grp, g)]
    n_in, n_out = groups * t * d * 32, groups * d * 32
    d_in, d_out = dev_buffer(eng, n_in), dev_buffer(eng, n_out + 32)
    try:
        for sfmt, k in ((CAN, 1), (MONT, MONT_R)):
            blob = pack_scalars([x * k % R for x in flat(vecs)])
            gb = pack_scalars([g * k % R for g in gammas])
            expect = pack_scalars([x * k % R for x in want])
            assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, n_in) == 0
            for in_dev in (0, L.IN_DEVICE):
                src = d_in if in_dev else blob
                rc, got = fold_raw(eng, src, d, t, gb, sfmt, in_dev)
                assert rc == 0 and got == expect, (sfmt, in_dev)
                assert eng.lib.kzg_dev_upload(eng.ctx, d_out, A5 * (n_out + 32), n_out + 32) == 0
                rc, _ = fold_raw(eng, src, d, t, gb, sfmt, in_dev | L.OUT_DEVICE, out=d_out)
                back = dev_download(eng, d_out, n_out + 32)
                assert rc == 0 and back[:n_out] == expect and back[n_out:] == A5 * 32, (sfmt, in_dev)  # nothing behind the last sum
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)
        eng.lib.kzg_dev_free(eng.ctx, d_out)


def test_fold_canonical_inputs_count_as_their_residues(eng):
    rng = random.Random(72)
    d, t = 257, 5
    big = [R, R + 5, (1 << 256) - 1, 2 * R, 2 * R + 1, R - 1, 0]
    vecs = [[big[(i + j) % len(big)] if (i + j) % 3 else rng.randrange(1 << 256) for j in range(d)] for i in range(t)]
    for gamma in (1, R - 1, rng.randrange(2, R)):
        rc, got = fold_raw(eng, b"".join(raw32(x) for v in vecs for x in v), d, t, le(gamma))
        assert rc == 0, eng.last_error()
        assert got == pack_scalars(FM.fold([[x % R for x in v] for v in vecs], gamma)), gamma


def test_fold_2_16(eng):
    rng = random.Random(73)
    d, t = 1 << 16, 4
    blob = rng.randbytes(32 * t * d)  # any 256-bit values: their residues count
    vecs = [unpack_scalars(blob[32 * i * d:32 * (i + 1) * d]) for i in range(t)]
    gamma = rng.randrange(2, R)
    rc, got = fold_raw(eng, blob, d, t, le(gamma))
    assert rc == 0, eng.last_error()
    assert got == pack_scalars(FM.fold(vecs, gamma))


def test_fold_host_input_staged_in_pieces(eng):
    """t x d x 32 bytes beyond one staging piece (64 MiB): the running sum is carried on the device between the pieces.  The columns at
    the block edges and a random sample are compared."""
    rng = random.Random(74)
    d, t = (1 << 17) + 1, 17
    blob = rng.randbytes(32 * t * d)
    gamma = rng.randrange(2, R)
    rc, got = fold_raw(eng, blob, d, t, le(gamma))
    assert rc == 0, eng.last_error()
    cols = [0, 1, 255, 256, 257, d - 257, d - 2, d - 1] + [rng.randrange(d) for _ in range(56)]
    for j in cols:
        col = [[int.from_bytes(blob[32 * (i * d + j):32 * (i * d + j) + 32], "little")] for i in range(t)]
        assert got[32 * j:32 * j + 32] == le(FM.fold(col, gamma)[0]), j


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
def srs64(eng, lags):
    """(KZGParams of setup(TAU, 64), the Lagrange SRS of the same tau)"""
    p = kzg_amd.setup(eng, TAU, 64, g2_len=2)
    yield p, lags(64)
    p.gs.free()
    p.hs.free()


def open_eval_raw(eng, lag, vecs, zs):
    """(ys bytes, witness bytes) of kzg_open_eval for len(zs) vectors"""
    d, batch = len(vecs[0]), len(zs)
    ys, ws = ctypes.create_string_buffer(32 * batch), ctypes.create_string_buffer(96 * batch)
    rc = eng.lib.kzg_open_eval(eng.ctx, lag.handle, pack_scalars(flat([vecs])), d, batch, b"".join(le(z) for z in zs), CAN, 0, ys, ws, AFF)
    assert rc == 0, eng.last_error()
    return ys.raw, ws.raw


def open_fold_raw(eng, fn, srs_handle, blob, d, t, zs, gammas, sfmt=CAN, flags=0, want_y=True, want_w=True, out_w=None, ofmt=AFF):
    """(rc, ys bytes or None, witness bytes or None) of kzg_open_fold_eval / kzg_open_fold_coeff; zs, gammas: ints"""
    groups, psz = len(zs), L.POINT_BYTES[ofmt]
    k = MONT_R if sfmt == MONT else 1
    ys = ctypes.create_string_buffer(A5 * (32 * groups * t), 32 * groups * t) if want_y else None
    ws = out_w if out_w is not None else (ctypes.create_string_buffer(A5 * (psz * groups), psz * groups) if want_w else None)
    rc = fn(eng.ctx, srs_handle, blob, d, t, groups, b"".join(le(z * k) for z in zs), b"".join(le(g * k) for g in gammas), sfmt, flags, ys, ws, ofmt)
    return rc, (ys.raw if want_y else None), (ws.raw if want_w and out_w is None else None)


def eval_expect(eng, lag, vecs, z, gamma):
    """(ys bytes, witness) of one group from the single-polynomial calls: kzg_eval_form_eval, kzg_open_eval of the host-folded vector
    (KZGProverEvalForm.open_at), kzg_witness_eval of it at a point of the domain (create_witness)"""
    d = len(vecs[0])
    ys = pack_scalars(eng.eval_form_eval(vecs, [z] * len(vecs)))
    folded = FM.fold(vecs, gamma)
    yF, w = open_eval_raw(eng, lag, [folded], [z])
    assert yF == le(FM.fold([[y] for y in unpack_scalars(ys)], gamma)[0])
    m = domain_index(d, z) if d <= 512 or z in (1, R - 1, omega(d), pow(omega(d), d - 1, R)) else None
    if m is not None:
        out = ctypes.create_string_buffer(96)
        assert eng.lib.kzg_witness_eval(eng.ctx, lag.handle, pack_scalars(folded), d, m, CAN, 0, out, AFF) == 0, eng.last_error()
        assert w == out.raw, (d, z)
    return ys, w


@pytest.mark.parametrize("d", [1, 2, 64, 512, 1 << 13])
def test_eval_form_against_the_single_polynomial_calls(eng, lags, d):
    rng = random.Random(800 + d)
    lag = lags(d)
    fn = eng.lib.kzg_open_fold_eval
    t = 3
    vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(t)]
    blob = pack_scalars(flat([vecs]))
    for k, z in enumerate(points_for(d, rng)):
        gamma = gammas_for(rng, 4)[k % 4]
        ys, w = eval_expect(eng, lag, vecs, z, gamma)
        rc, got_y, got_w = open_fold_raw(eng, fn, lag.handle, blob, d, t, [z], [gamma])
        assert rc == 0, eng.last_error()
        assert got_y == ys and got_w == w, (d, z, gamma)
        if gamma == 1:  # the sum of the t single witnesses
            singles = open_eval_raw(eng, lag, vecs, [z] * t)[1]
            assert got_w == eng.g1_sum([singles[96 * i:96 * i + 96] for i in range(t)]), (d, z)
        if d <= 64 and (TAU - z) % R:
            coeffs = [eng.ntt(v, log2(d), inverse=True) if d > 1 else v for v in vecs]
            mys, pi = FM.open_fold(coeffs, z, gamma, TAU)
            assert got_y == pack_scalars(mys) and got_w == C.g1_mul(C.g1_generator(), pi), (d, z)


@pytest.mark.parametrize("t", [1, 17, 33])
def test_eval_form_t_across_the_chunk_of_sixteen(eng, lags, t):
    rng = random.Random(810 + t)
    d = 64
    lag = lags(d)
    vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(t)]
    blob = pack_scalars(flat([vecs]))
    d_in = dev_buffer(eng, len(blob))
    try:
        assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, len(blob)) == 0
        for z in (rng.randrange(R), pow(omega(d), 5, R)):
            gamma = rng.randrange(2, R)
            ys, w = eval_expect(eng, lag, vecs, z, gamma)
            for src, flags in ((blob, 0), (d_in, L.IN_DEVICE)):
                rc, got_y, got_w = open_fold_raw(eng, eng.lib.kzg_open_fold_eval, lag.handle, src, d, t, [z], [gamma], flags=flags)
                assert rc == 0, eng.last_error()
                assert got_y == ys and got_w == w, (t, z, flags)
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)


@pytest.fixture(scope="module")
def groups18(eng, lags):
    """18 groups of 3 vectors at d = 64 (more groups than lanes), distinct points with on-domain ones among them, and what the
    single-polynomial calls give for every group: computed once"""
    rng = random.Random(82)
    d, t, groups = 64, 3, 18
    lag = lags(d)
    vecs = [[[rng.randrange(R) for _ in range(d)] for _ in range(t)] for _ in range(groups)]
    zs = [pow(omega(d), rng.randrange(d), R) if g % 4 == 1 else rng.randrange(R) for g in range(groups)]
    gammas = gammas_for(rng, groups)
    per = [eval_expect(eng, lag, vecs[g], zs[g], gammas[g]) for g in range(groups)]
    return d, t, lag, vecs, zs, gammas, b"".join(p[0] for p in per), b"".join(p[1] for p in per)


@pytest.mark.parametrize("groups", [1, 3, 18])
def test_eval_form_groups_with_distinct_points(eng, groups18, groups):
    d, t, lag, vecs, zs, gammas, ys, ws = groups18
    blob = pack_scalars(flat(vecs[:groups]))
    rc, got_y, got_w = open_fold_raw(eng, eng.lib.kzg_open_fold_eval, lag.handle, blob, d, t, zs[:groups], gammas[:groups])
    assert rc == 0, eng.last_error()
    assert got_y == ys[:32 * t * groups] and got_w == ws[:96 * groups]


def test_eval_form_groups_that_share_a_point_and_fewer_lanes(eng, groups18):
    d, t, lag, vecs, zs, gammas, ys, ws = groups18
    rng = random.Random(83)
    groups = 5
    z = rng.randrange(R)
    per = [eval_expect(eng, lag, vecs[g], z, gammas[g]) for g in range(groups)]
    rc, got_y, got_w = open_fold_raw(eng, eng.lib.kzg_open_fold_eval, lag.handle, pack_scalars(flat(vecs[:groups])), d, t, [z] * groups, gammas[:groups])
    assert rc == 0, eng.last_error()
    assert got_y == b"".join(p[0] for p in per) and got_w == b"".join(p[1] for p in per)
    eng.set_option("streams", 4)  # 18 groups: five chunks of groups, the last one ragged
    try:
        rc, got_y, got_w = open_fold_raw(eng, eng.lib.kzg_open_fold_eval, lag.handle, pack_scalars(flat(vecs)), d, t, zs, gammas)
        assert rc == 0, eng.last_error()
        assert got_y == ys and got_w == ws
    finally:
        eng.set_option("streams", 13)


def test_eval_form_null_outputs_device_buffers_and_montgomery(eng, groups18):
    d, t, lag, vecs, zs, gammas, ys, ws = groups18
    fn = eng.lib.kzg_open_fold_eval
    groups = 4
    blob = pack_scalars(flat(vecs[:groups]))
    zs, gammas, ys, ws = zs[:groups], gammas[:groups], ys[:32 * t * groups], ws[:96 * groups]
    d_in, d_out = dev_buffer(eng, len(blob)), dev_buffer(eng, 96 * groups + 96)
    try:
        assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, len(blob)) == 0
        for in_dev in (0, L.IN_DEVICE):
            src = d_in if in_dev else blob
            rc, got_y, got_w = open_fold_raw(eng, fn, lag.handle, src, d, t, zs, gammas, flags=in_dev, want_w=False)
            assert rc == 0 and got_y == ys and got_w is None, in_dev
            rc, got_y, got_w = open_fold_raw(eng, fn, lag.handle, src, d, t, zs, gammas, flags=in_dev, want_y=False)
            assert rc == 0 and got_y is None and got_w == ws, in_dev
            rc, got_y, _ = open_fold_raw(eng, fn, lag.handle, src, d, t, zs, gammas, flags=in_dev | L.OUT_DEVICE, out_w=d_out)
            back = dev_download(eng, d_out, 96 * groups + 96)
            assert rc == 0 and got_y == ys and back[:96 * groups] == ws and back[96 * groups:] == A5 * 96, in_dev
        mont = pack_scalars([x * MONT_R % R for x in flat(vecs[:groups])])
        rc, got_y, got_w = open_fold_raw(eng, fn, lag.handle, mont, d, t, zs, gammas, sfmt=MONT)
        assert rc == 0, eng.last_error()
        assert got_y == pack_scalars([y * MONT_R % R for y in unpack_scalars(ys)]) and got_w == ws
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)
        eng.lib.kzg_dev_free(eng.ctx, d_out)


# ---- 3. coefficient form -----------------------------------------------------------------------------------------------------------
N_MAX = (1 << 13) + 1


@pytest.fixture(scope="module")
def params(eng):
    p = kzg_amd.setup(eng, TAU, N_MAX, g2_len=2)
    yield p
    p.gs.free()
    p.hs.free()


def witness_coeff(eng, params, coeffs, z, y):
    out = ctypes.create_string_buffer(96)
    rc = eng.lib.kzg_witness_coeff(eng.ctx, params.gs.handle, pack_scalars(coeffs), len(coeffs), le(z), le(y), CAN, 0, out, AFF)
    assert rc == 0, eng.last_error()
    return out.raw


def coeff_expect(eng, params, polys, z, gamma):
    """(ys bytes, witness) of one group: kzg_poly_eval per polynomial, kzg_witness_coeff of the host-folded polynomial at (z, F(z))"""
    ys = [eng.poly_eval(p, z) for p in polys]
    F = FM.fold(polys, gamma)
    return pack_scalars(ys), witness_coeff(eng, params, F, z, FM.fold([[y] for y in ys], gamma)[0])


@pytest.mark.parametrize("n,t", [(1, 3), (2, 3), (100, 1), (100, 3), (100, 17), (2049, 3), (N_MAX, 3)])
def test_coeff_form_against_the_single_polynomial_calls(eng, params, n, t):
    rng = random.Random(900 + 31 * n + t)
    fn = eng.lib.kzg_open_fold_coeff
    groups = 3 if n <= 100 else 1
    polys = [[[rng.randrange(R) for _ in range(n)] for _ in range(t)] for _ in range(groups)]
    zs = [rng.randrange(R), 0, 1][:groups]
    gammas = gammas_for(rng, groups, n + t)
    per = [coeff_expect(eng, params, polys[g], zs[g], gammas[g]) for g in range(groups)]
    ys, ws = b"".join(p[0] for p in per), b"".join(p[1] for p in per)
    blob = pack_scalars(flat(polys))
    rc, got_y, got_w = open_fold_raw(eng, fn, params.gs.handle, blob, n, t, zs, gammas)
    assert rc == 0, eng.last_error()
    assert got_y == ys and got_w == ws, (n, t)
    if n == 1:
        assert got_w == bytes(96 * groups)  # constants: the identity
    if n <= 100:
        mys, pi = FM.open_fold(polys[0], zs[0], gammas[0], TAU)
        assert got_y[:32 * t] == pack_scalars(mys) and got_w[:96] == C.g1_mul(C.g1_generator(), pi)
    if n == 100 and t == 17:  # device input, each output alone
        d_in = dev_buffer(eng, len(blob))
        try:
            assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, len(blob)) == 0
            assert open_fold_raw(eng, fn, params.gs.handle, d_in, n, t, zs, gammas, flags=L.IN_DEVICE) == (0, ys, ws)
            assert open_fold_raw(eng, fn, params.gs.handle, d_in, n, t, zs, gammas, flags=L.IN_DEVICE, want_w=False) == (0, ys, None)
            assert open_fold_raw(eng, fn, params.gs.handle, blob, n, t, zs, gammas, want_y=False) == (0, None, ws)
        finally:
            eng.lib.kzg_dev_free(eng.ctx, d_in)


# ---- 4. the verifier ---------------------------------------------------------------------------------------------------------------
class FoldCall:
    """`groups` folded openings of the SAME t polynomials of 100 coefficients at z, z w, z w^2 ...: t commitments named through
    indices, produced by kzg_open_fold_coeff"""

    def __init__(self, eng, params, groups, t=3, seed=1):
        rng = random.Random(1000 + seed)
        self.t, self.groups = t, groups
        self.polys = [[rng.randrange(R) for _ in range(100)] for _ in range(t)]
        z, w = rng.randrange(R), omega(128)
        self.zs = [z * pow(w, g, R) % R for g in range(groups)]
        self.gammas = [rng.randrange(1, R) for _ in range(groups)]
        prover = kzg_amd.KZGProver(params)
        ys, self.witnesses = prover.open_fold_batch([self.polys] * groups, self.zs, self.gammas)
        self.ys = [y for grp in ys for y in grp]
        self.commitments = [prover.commit(kzg_amd.Polynomial(p)) for p in self.polys]
        self.idx = [i for _ in range(groups) for i in range(t)]

    def copy(self):
        c = object.__new__(FoldCall)
        c.__dict__ = {k: (list(v) if isinstance(v, list) else v) for k, v in self.__dict__.items()}
        return c

    def per_value(self):
        """the same call with one commitment per value and NULL indices"""
        c = self.copy()
        c.commitments, c.idx = [self.commitments[i] for i in self.idx], None
        return c


def verify_raw(eng, params, c, r, sfmt=CAN, pfmt=AFF, gs=0, hs=0, ok=0, **kw):
    """(rc, *ok) of kzg_verify_fold; *ok starts at UNTOUCHED; kw overrides t / groups / n_commitments or blanks a pointer with None"""
    a = dict(zs=pack_scalars(c.zs), ys=pack_scalars(c.ys), commitments=b"".join(c.commitments), witnesses=b"".join(c.witnesses),
             gammas=b"".join(g if isinstance(g, bytes) else raw32(g) for g in c.gammas), r=None if r is None else (r if isinstance(r, bytes) else raw32(r)),
             t=c.t, groups=c.groups, n_commitments=len(c.commitments))
    a.update(kw)
    idx = None if c.idx is None else (ctypes.c_uint32 * len(c.idx))(*c.idx)
    v = ctypes.c_int(UNTOUCHED)
    rc = eng.lib.kzg_verify_fold(eng.ctx, params.gs.handle if gs == 0 else gs, params.hs.handle if hs == 0 else hs, a["zs"], a["ys"], sfmt,
                                 a["commitments"], a["n_commitments"], idx, a["witnesses"], pfmt, a["t"], a["groups"], a["gammas"], a["r"],
                                 ctypes.byref(v) if ok == 0 else ok)
    return rc, v.value


@pytest.fixture(scope="module")
def calls(eng, params):
    return {g: FoldCall(eng, params, g, seed=g) for g in (1, 2, 5)}


@pytest.mark.parametrize("groups", [1, 2, 5])
def test_verify_fold_honest_and_one_flip_at_a_time(eng, params, calls, groups):
    c = calls[groups]
    rng = random.Random(110 + groups)
    r = rng.randrange(1, R)
    one = c.per_value()
    assert verify_raw(eng, params, c, r) == (0, 1) and verify_raw(eng, params, one, r) == (0, 1)
    if groups == 1:
        assert verify_raw(eng, params, c, None) == (0, 1)  # r may be NULL for one group
    # the folded witness is a plain opening of the folded polynomial: kzg_verify_eval against commit(F)
    kv, prover = kzg_amd.KZGVerifier(params), kzg_amd.KZGProver(params)
    for g in range(groups):
        F = FM.fold(c.polys, c.gammas[g])
        yF = FM.fold([[y] for y in c.ys[g * c.t:(g + 1) * c.t]], c.gammas[g])[0]
        assert kv.verify_eval((c.zs[g], yF), prover.commit(kzg_amd.Polynomial(F)), c.witnesses[g])
    # the model's verdict with the scalars behind the points
    tau_c = [FM.poly_eval(p, TAU) for p in c.polys]
    pis = [FM.open_fold(c.polys, z, g, TAU)[1] for z, g in zip(c.zs, c.gammas)]
    assert FM.verdict(TAU, r, c.gammas, c.t, c.zs, c.ys, tau_c, c.idx, pis)
    g, k = groups - 1, groups * c.t - 2
    flips = []
    for field, at in (("ys", k), ("zs", g), ("gammas", g)):
        b = c.copy()
        getattr(b, field)[at] = getattr(b, field)[at] % (R - 1) + 1
        flips.append((field, b))
    b = c.copy()
    b.commitments[1] = c.commitments[0]
    flips.append(("commitment", b))
    b = c.copy()
    b.witnesses[g] = c.commitments[0]
    flips.append(("witness", b))
    for name, b in flips:
        assert verify_raw(eng, params, b, r) == (0, 0), name
        assert verify_raw(eng, params, b.per_value(), r) == (0, 0), name


def test_verify_fold_chunks_and_both_pairing_sites(eng, params, calls):
    c = calls[5]  # 15 values, 5 witnesses
    bad = c.copy()
    bad.ys[13] = (bad.ys[13] + 1) % R
    try:
        for chunk in (0, 4, 7):
            eng.set_option("verify_eval_batch_chunk", chunk)
            for host in (1, 0):
                eng.set_option("host_pairing", host)
                for call, want in ((c, 1), (c.per_value(), 1), (bad, 0), (bad.per_value(), 0)):
                    assert verify_raw(eng, params, call, 0xABCDEF) == (0, want), (chunk, host)
    finally:
        eng.set_option("verify_eval_batch_chunk", 0)
        eng.set_option("host_pairing", 1)


def test_verify_fold_at_t_1_is_kzg_verify_eval_batch(eng, params):
    """t = 1: rho_{g,0} = r^g, so both calls compute the same equation.  Five openings, the same r, points, values, commitments and
    witnesses into both, with indices and with one commitment per opening: the same verdict, honest and with one value flipped."""
    c = FoldCall(eng, params, 5, t=1, seed=77)
    bad = c.copy()
    bad.ys[3] = (bad.ys[3] + 1) % R
    r = 0x1234567

    def eval_batch(call):
        idx = None if call.idx is None else (ctypes.c_uint32 * len(call.idx))(*call.idx)
        v = ctypes.c_int(UNTOUCHED)
        rc = eng.lib.kzg_verify_eval_batch(eng.ctx, params.gs.handle, params.hs.handle, pack_scalars(call.zs), pack_scalars(call.ys), CAN,
                                           b"".join(call.commitments), len(call.commitments), idx, b"".join(call.witnesses), AFF, 5, raw32(r),
                                           ctypes.byref(v))
        return rc, v.value
    for call, want in ((c, 1), (c.per_value(), 1), (bad, 0), (bad.per_value(), 0)):
        assert verify_raw(eng, params, call, r) == (0, want), (want, call.idx)
        assert eval_batch(call) == (0, want), (want, call.idx)


def test_verify_fold_of_evaluation_form_openings(eng, srs64):
    rng = random.Random(120)
    d, t, groups = 64, 4, 3
    params, lag = srs64
    prover = kzg_amd.KZGProverEvalForm(params, lag)
    doms = [[kzg_amd.EvaluationDomain.from_coeffs([rng.randrange(R) for _ in range(d)]) for _ in range(t)] for _ in range(groups)]
    zs = [rng.randrange(R), pow(omega(d), 3, R), 0]
    gammas = [rng.randrange(1, R) for _ in range(groups)]
    ys, ws = prover.open_fold_batch(doms, zs, gammas)
    commitments = [prover.commit(ev) for grp in doms for ev in grp]
    kv = kzg_amd.KZGVerifierEvalForm(params, lag)
    assert kv.verify_fold_batch(zs, ys, commitments, ws, gammas) is True  # r drawn by the method
    assert kv.verify_fold_batch(zs, ys, commitments, ws, gammas, r=5) is True
    for g in range(groups):
        assert prover.open_fold(doms[g], zs[g], gammas[g]) == (ys[g], ws[g])
        assert kv.verify_fold(zs[g], ys[g], commitments[g * t:(g + 1) * t], ws[g], gammas[g]) is True
    bad = [list(y) for y in ys]
    bad[1][2] = (bad[1][2] + 1) % R
    assert kv.verify_fold_batch(zs, bad, commitments, ws, gammas) is False
    assert kv.verify_fold(zs[1], bad[1], commitments[t:2 * t], ws[1], gammas[1]) is False
    # the header's cancellation: with gamma known in advance y_0 + D and y_1 - D / gamma pass, and a fresh gamma catches them
    g0 = gammas[0]
    forged = [(ys[0][0] + 9) % R, (ys[0][1] - 9 * pow(g0, R - 2, R)) % R] + ys[0][2:]
    assert kv.verify_fold(zs[0], forged, commitments[:t], ws[0], g0) is True
    fresh = g0 % (R - 1) + 1
    assert kv.verify_fold(zs[0], forged, commitments[:t], prover.open_fold(doms[0], zs[0], fresh)[1], fresh) is False
    assert kzg_amd.KZGVerifier(params).verify_fold_batch([], [], [], [], []) is True


def test_verify_fold_malformed_point_leaves_ok_unwritten(eng, params, calls):
    c = calls[2]
    off = bytearray(c.witnesses[1])
    off[0] ^= 1
    for field, k in (("witnesses", 1), ("commitments", 0)):
        for b in (c.copy(), c.per_value()):
            getattr(b, field)[k] = bytes(off)
            assert verify_raw(eng, params, b, 77) == (L.KZG_ERR_BAD_POINT, UNTOUCHED), field


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_shape_errors_leave_the_outputs_untouched(eng, hooks, lags, params, calls):
    d, t = 64, 3
    lag = lags(d)
    lib, ctx, h, gsh = eng.lib, eng.ctx, lag.handle, params.gs.handle
    blob = pack_scalars(list(range(2 * t * d)))
    z, g, zero, big = le(7) * 2, le(5) * 2, le(7) + bytes(32), le(7) + raw32(R)
    ys, ws, out = (ctypes.create_string_buffer(A5 * (32 * 2 * t), 32 * 2 * t), ctypes.create_string_buffer(A5 * 288, 288),
                   ctypes.create_string_buffer(A5 * (64 * d), 64 * d))
    huge = 1 << 62
    bad = [
        lib.kzg_fr_fold(ctx, blob, d, 0, 2, g, CAN, 0, out),                       # t == 0
        lib.kzg_fr_fold(ctx, blob, 0, t, 2, g, CAN, 0, out),                       # d == 0
        lib.kzg_fr_fold(ctx, blob, d, t, 2, zero, CAN, 0, out),                    # gamma == 0
        lib.kzg_fr_fold(ctx, blob, d, t, 2, big, CAN, 0, out),                     # gamma >= modulus
        lib.kzg_fr_fold(ctx, blob, d, t, 2, big, MONT, 0, out),
        lib.kzg_fr_fold(ctx, blob, d, t, 2, g, 2, 0, out),                         # unknown format
        lib.kzg_fr_fold(ctx, None, d, t, 2, g, CAN, 0, out),                       # NULL inputs with work to do
        lib.kzg_fr_fold(ctx, blob, d, t, 2, None, CAN, 0, out),
        lib.kzg_fr_fold(ctx, blob, d, t, 2, g, CAN, 0, None),
        lib.kzg_fr_fold(ctx, blob, huge, huge, 2, g, CAN, 0, out),                 # size overflow
        lib.kzg_fr_fold(None, blob, d, t, 2, g, CAN, 0, out),
    ]
    for fn, hd, n in ((lib.kzg_open_fold_eval, h, d), (lib.kzg_open_fold_coeff, gsh, d)):
        bad += [
            fn(ctx, hd, blob, n, 0, 2, z, g, CAN, 0, ys, ws, AFF),                 # t == 0
            fn(ctx, hd, blob, n, t, 2, z, zero, CAN, 0, ys, ws, AFF),              # gamma == 0
            fn(ctx, hd, blob, n, t, 2, z, big, CAN, 0, ys, ws, AFF),               # gamma >= modulus
            fn(ctx, hd, blob, n, t, 2, big, g, CAN, 0, ys, ws, AFF),               # z >= modulus
            fn(ctx, hd, blob, n, t, 2, big, g, MONT, 0, ys, ws, AFF),
            fn(ctx, hd, blob, n, t, 2, z, g, 2, 0, ys, ws, AFF),                   # unknown formats
            fn(ctx, hd, blob, n, t, 2, z, g, CAN, 0, ys, ws, 4),
            fn(ctx, None, blob, n, t, 2, z, g, CAN, 0, ys, ws, AFF),               # NULL inputs with work to do
            fn(ctx, hd, None, n, t, 2, z, g, CAN, 0, ys, ws, AFF),
            fn(ctx, hd, blob, n, t, 2, None, g, CAN, 0, ys, ws, AFF),
            fn(ctx, hd, blob, n, t, 2, z, None, CAN, 0, ys, ws, AFF),
            fn(ctx, hd, blob, n, t, 2, z, g, CAN, 0, None, None, AFF),             # both outputs NULL
            fn(ctx, hd, blob, n, huge, huge, z, g, CAN, 0, ys, ws, AFF),           # size overflow
            fn(None, hd, blob, n, t, 2, z, g, CAN, 0, ys, ws, AFF),
        ]
    bad += [
        lib.kzg_open_fold_eval(ctx, h, blob, 48, t, 2, z, g, CAN, 0, ys, ws, AFF),     # d not a power of two
        lib.kzg_open_fold_eval(ctx, h, blob, d // 2, t, 2, z, g, CAN, 0, ys, ws, AFF),  # d != len(lagrange)
        lib.kzg_open_fold_eval(ctx, h, blob, 0, t, 2, z, g, CAN, 0, ys, ws, AFF),
        lib.kzg_open_fold_coeff(ctx, gsh, blob, 0, t, 2, z, g, CAN, 0, ys, ws, AFF),    # n == 0
        lib.kzg_open_fold_coeff(ctx, gsh, blob, N_MAX + 2, t, 2, z, g, CAN, 0, ys, ws, AFF),  # n - 1 > len(srs)
    ]
    assert bad == [SH] * len(bad), bad
    hooks.lib.kzg_test_srs_set_device.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hooks.lib.kzg_test_srs_set_device.restype = ctypes.c_int
    for fn, hd in ((lib.kzg_open_fold_eval, h), (lib.kzg_open_fold_coeff, gsh)):    # an SRS on another GPU
        assert hooks.lib.kzg_test_srs_set_device(hd, 1) == 0
        try:
            assert fn(ctx, hd, blob, d, t, 2, z, g, CAN, 0, ys, ws, AFF) == SH
            assert "another GPU" in eng.last_error()
            if hd == gsh:
                assert verify_raw(eng, params, calls[2], 5) == (SH, UNTOUCHED)
        finally:
            hooks.lib.kzg_test_srs_set_device(hd, 0)
    assert ys.raw == A5 * (32 * 2 * t) and ws.raw == A5 * 288 and out.raw == A5 * (64 * d)
    # groups == 0
    assert lib.kzg_fr_fold(ctx, None, d, t, 0, None, CAN, 0, None) == 0
    assert lib.kzg_open_fold_eval(ctx, h, None, d, t, 0, None, None, CAN, 0, ys, ws, AFF) == 0
    assert lib.kzg_open_fold_coeff(ctx, gsh, None, d, t, 0, None, None, CAN, 0, ys, ws, AFF) == 0
    assert ys.raw == A5 * (32 * 2 * t) and ws.raw == A5 * 288
    # the verifier
    c, r = calls[2], 12345
    assert verify_raw(eng, params, c, r) == (0, 1)
    shape = [
        verify_raw(eng, params, c, r, t=0),
        verify_raw(eng, params, c, 0), verify_raw(eng, params, c, R), verify_raw(eng, params, c, None),  # r, groups > 1
        verify_raw(eng, params, c, R, sfmt=MONT),
        verify_raw(eng, params, c, r, gammas=raw32(5) + bytes(32)), verify_raw(eng, params, c, r, gammas=raw32(5) + raw32(R)),
        verify_raw(eng, params, c, r, zs=le(1) + raw32(R)),
        verify_raw(eng, params, c, r, sfmt=2), verify_raw(eng, params, c, r, pfmt=7), verify_raw(eng, params, c, r, pfmt=L.G1_JACOBIAN_MONT),
        verify_raw(eng, params, c, r, gs=None), verify_raw(eng, params, c, r, hs=None),
        verify_raw(eng, params, c.per_value(), r, n_commitments=5),  # NULL indices with n_commitments != groups x t
        verify_raw(eng, params, c, r, t=1 << 62, groups=1 << 62),    # size overflow
    ]
    for hole in ("zs", "ys", "commitments", "witnesses", "gammas"):
        shape.append(verify_raw(eng, params, c, r, **{hole: None}))
    b = c.copy()
    b.idx[4] = 3  # an index out of range
    shape.append(verify_raw(eng, params, b, r))
    assert shape == [(SH, UNTOUCHED)] * len(shape), shape
    assert verify_raw(eng, params, c, r, ok=None)[0] == SH
    assert verify_raw(eng, params, c, r, groups=0) == (0, 1)
    # and the context is fine afterwards
    assert verify_raw(eng, params, c, R - 1) == (0, 1)
    rc, got, _ = open_fold_raw(eng, lib.kzg_open_fold_eval, h, blob, d, t, [7, 7], [5, 5], want_w=False)
    assert rc == 0 and got == pack_scalars(eng.eval_form_eval(blob, [7] * (2 * t), d))


# ---- 6. two threads on one context ---------------------------------------------------------------------------------------------------
def test_two_threads_verify_fold_on_one_context(eng, params, calls):
    good, bad = calls[5], calls[5].copy()
    bad.ys[7] = (bad.ys[7] + 1) % R
    jobs = [(good, 1), (bad, 0), (good.per_value(), 1), (calls[2], 1)]
    verify_raw(eng, params, good, 3)  # the lanes exist before the threads start
    out = {}

    def work(name):
        out[name] = [verify_raw(eng, params, c, 1000 + k) for k, (c, _) in enumerate(jobs * 2)]
    th = [threading.Thread(target=work, args=(n,)) for n in ("a", "b")]
    for t in th:
        t.start()
    for t in th:
        t.join()
    want = [(0, w) for _, w in jobs * 2]
    assert out == {"a": want, "b": want}, out


# ---- 7. the C++ mirror and the Python surface ----------------------------------------------------------------------------------------
def test_cpp_wrapper(tmp_path):
    """fr_fold, open_fold_batch and verify_fold of include/kzg_mi355x.hpp: tests/cpp_open_fold_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_open_fold_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_open_fold_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_python_surface(eng, params):
    rng = random.Random(130)
    prover, kv = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    polys = [kzg_amd.Polynomial([rng.randrange(R) for _ in range(n)]) for n in (40, 7, 25)]  # padded to the longest by the method
    z, gamma = rng.randrange(R), rng.randrange(1, R)
    ys, w = prover.open_fold(polys, z, gamma)
    assert ys == [p.eval(eng, z) for p in polys]
    commitments = [prover.commit(p) for p in polys]
    assert kv.verify_fold(z, ys, commitments, w, gamma) is True
    assert kv.verify_fold(z, ys, commitments, w, gamma % (R - 1) + 1) is False
    assert kv.verify_fold_batch([z, z], [ys, ys], commitments, [w, w], [gamma, gamma], commitment_idx=[0, 1, 2, 0, 1, 2]) is True
    vecs = [rng.randrange(R) for _ in range(2 * 3 * 10)]
    want = FM.fold([vecs[0:10], vecs[10:20], vecs[20:30]], 3) + FM.fold([vecs[30:40], vecs[40:50], vecs[50:60]], R - 1)
    assert eng.fr_fold(vecs, 10, 3, [3, R - 1]) == want
    buf, out = eng.alloc_scalars(60).upload(pack_scalars(vecs)), eng.alloc_scalars(20)
    try:
        assert eng.fr_fold(buf, 10, 3, [3, R - 1], out=out) is out and unpack_scalars(out.download()) == want
    finally:
        buf.free()
        out.free()
    for g in (0, R):
        with pytest.raises(kzg_amd.ReferencePanic):
            eng.fr_fold(vecs, 10, 3, [3, g])
