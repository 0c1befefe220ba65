"""kzg_verify_eval_batch (kzg_amd/csrc/verify_eval_batch.hip): one verdict per call of single-point openings from one pairing check.
The scalars and the four points of the combination through the hook against the model (tests/verify_eval_batch_model.py) and
kzg_msm_g1, the call across the slices of the variable-base sum, the verdicts for honest, tampered and compensating openings against
kzg_verify_eval, edge inputs, formats, options, validation, concurrency and the Python surface.  Like tests/test_gpu_verify_cosets.py
this file opens and closes its own module-scoped Engine and HooksEngine."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import verify_eval_batch_model as E
from tests.fk20_common import MONT_R, VP, SZ, I32, U32
from tests.fk20_common import eng, hooks, params, plans  # noqa: F401 -- this module's fixtures
from tests.gpu_common import rand_scalars
from tests.test_gpu_verify_cosets import AFFINE, U32P
from tests.test_gpu_validation import _non_subgroup_g1

pytestmark = pytest.mark.gpu

R = M.R
TAU = 0x5EED_CE115
SRS_LEN = 1 << 12
G2_LEN = 2
PLAN = kzg_amd.FK20Plan
UNTOUCHED = 0x5A5A5A5A
BATCH_ARGS = [VP, VP, VP, VP, VP, I32, VP, SZ, U32P, VP, I32, SZ, VP, ctypes.POINTER(I32)]
IDENTITY = bytes(96)


def scalar(x):
    return (x % (1 << 256)).to_bytes(32, "little")


def blob_of(values, sfmt=L.FR_CANONICAL):
    """the scalars as the call reads them: canonical as they are (unreduced ones included), Montgomery of their residues"""
    return b"".join(scalar(v if sfmt == L.FR_CANONICAL else v * MONT_R % R) for v in values)


def raw_batch(e, gs, hs, xs, ys, commitments, idx, witnesses, r, sfmt=L.FR_CANONICAL, pfmt=L.G1_AFFINE_MONT, count=None, n_commitments=None,
              ok="own"):
    """(rc, *ok) of one kzg_verify_eval_batch call; *ok starts as UNTOUCHED.  xs, ys: lists of ints or None, r: an int (sent as it is)
    or None, idx: a list or None"""
    count = len(witnesses) if count is None else count
    okv = I32(UNTOUCHED)
    if e.lib.kzg_verify_eval_batch.argtypes != BATCH_ARGS:  # (the hooks library; set before any thread calls)
        e.lib.kzg_verify_eval_batch.argtypes = BATCH_ARGS
        e.lib.kzg_verify_eval_batch.restype = I32
    rc = e.lib.kzg_verify_eval_batch(e.ctx, gs, hs, blob_of(xs, sfmt) if xs is not None else None, blob_of(ys, sfmt) if ys is not None else None,
                                     sfmt, b"".join(commitments) if commitments is not None else None,
                                     len(commitments) if n_commitments is None else n_commitments,
                                     (U32 * max(len(idx), 1))(*idx) if idx is not None else None,
                                     b"".join(witnesses) if witnesses is not None else None, pfmt, count, scalar(r) if r is not None else None,
                                     ctypes.byref(okv) if ok == "own" else None)
    return rc, okv.value


def raw_each(e, gs, hs, xs, ys, commitments, witnesses, pfmt=L.G1_AFFINE_MONT):
    """the verdicts of kzg_verify_eval for the same openings, one commitment per opening"""
    n = len(xs)
    okb = ctypes.create_string_buffer(b"\xa5" * n, n)
    rc = e.lib.kzg_verify_eval(e.ctx, gs, hs, blob_of(xs), blob_of(ys), L.FR_CANONICAL, b"".join(commitments), b"".join(witnesses), pfmt, n, okb)
    assert rc == 0, e.last_error()
    return [bool(b) for b in okb.raw]


def tamper_point(blob, k=1):
    """another point of the subgroup: blob + [k]G"""
    return C.point_to_blob(M.g1_add(C.blob_to_point(blob), M.g1_mul(M.G1, k)))


class Call:
    """the arguments of one call, kept as lists so that a test can tamper with a copy"""

    def __init__(self, xs, ys, commitments, idx, witnesses):
        self.xs, self.ys, self.commitments, self.idx, self.witnesses = list(xs), list(ys), list(commitments), idx and list(idx), list(witnesses)

    def copy(self):
        return Call(self.xs, self.ys, self.commitments, self.idx, self.witnesses)

    def per_opening(self):
        """one commitment per opening: what NULL indices and kzg_verify_eval take"""
        cm = self.commitments if self.idx is None else [self.commitments[m] for m in self.idx]
        return Call(self.xs, self.ys, cm, None, self.witnesses)

    def batch(self, e, p, r, **kw):
        return raw_batch(e, p.gs.handle, p.hs.handle, self.xs, self.ys, self.commitments, self.idx, self.witnesses, r, **kw)

    def each(self, e, p):
        q = self.per_opening()
        return raw_each(e, p.gs.handle, p.hs.handle, q.xs, q.ys, q.commitments, q.witnesses)


_CALLS = {}


def mixed_call(params, count, seed=0):
    """`count` honest openings at random points of three polynomials (8, 2 and 5 coefficients) in random order; a fourth commitment
    that no opening names, opening count - 1 repeats opening 0.  Computed once per (count, seed) and left unchanged"""
    if (count, seed) not in _CALLS:
        rng = random.Random(77 * count + seed)
        prover = kzg_amd.KZGProver(params)
        polys = [kzg_amd.Polynomial.new_from_coeffs(rand_scalars(rng, n), n - 1) for n in (8, 2, 5, 3)]
        idx = [k % 3 if k < 3 else rng.randrange(3) for k in range(count)]
        xs = [rng.randrange(R) for _ in range(count)]
        if count > 1:
            idx[-1], xs[-1] = idx[0], xs[0]
        ys = [E.poly_eval(polys[m].slice_coeffs(), x) for m, x in zip(idx, xs)]
        ws = [None] * count
        for m in range(3):
            mine = [k for k in range(count) if idx[k] == m]
            if not mine:
                continue
            got, fine = prover.create_witness_many(polys[m], [(xs[k], ys[k]) for k in mine[1:]])
            assert all(fine)
            for k, w in zip(mine, [prover.create_witness(polys[m], (xs[mine[0]], ys[mine[0]]))] + got):
                ws[k] = w
        _CALLS[(count, seed)] = Call(xs, ys, [prover.commit(p) for p in polys], idx, ws)
    return _CALLS[(count, seed)].copy()


# ---- 1. the parts of the combination, through the hook ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook_srs(hooks):
    """(gs, hs) of the same tau in the hooks build of the library"""
    lib = hooks.lib
    lib.kzg_srs_setup_g1.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    lib.kzg_srs_setup_g2.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    lib.kzg_srs_free.argtypes = lib.kzg_srs_g2_free.argtypes = [VP, VP]
    lib.kzg_srs_free.restype = lib.kzg_srs_g2_free.restype = None
    lib.kzg_test_verify_eval_batch_parts.argtypes = BATCH_ARGS + [VP, VP, VP]
    lib.kzg_test_verify_eval_batch_parts.restype = I32
    lib.kzg_test_srs_set_device.argtypes = lib.kzg_test_srs_g2_set_device.argtypes = [VP, I32]
    gs, hs = VP(), VP()
    assert lib.kzg_srs_setup_g1(hooks.ctx, scalar(TAU), L.FR_CANONICAL, 4, ctypes.byref(gs)) == 0
    assert lib.kzg_srs_setup_g2(hooks.ctx, scalar(TAU), L.FR_CANONICAL, 2, ctypes.byref(hs)) == 0
    yield gs, hs
    lib.kzg_srs_free(hooks.ctx, gs)
    lib.kzg_srs_g2_free(hooks.ctx, hs)


def parts(hooks, hook_srs, call, r, sfmt=L.FR_CANONICAL):
    """(ok, yagg, c, [P1, P2, third set, Ragg slot]) of kzg_test_verify_eval_batch_parts"""
    n = len(call.commitments)
    yagg, cw, pts, ok = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(4 * 96), I32(UNTOUCHED)
    idx = (U32 * len(call.idx))(*call.idx) if call.idx is not None else None
    rc = hooks.lib.kzg_test_verify_eval_batch_parts(hooks.ctx, hook_srs[0], hook_srs[1], blob_of(call.xs, sfmt), blob_of(call.ys, sfmt), sfmt,
                                                    b"".join(call.commitments), n, idx, b"".join(call.witnesses), L.G1_AFFINE_MONT,
                                                    len(call.witnesses), blob_of([r], sfmt), ctypes.byref(ok), yagg, cw, pts)
    assert rc == 0, hooks.last_error()
    return ok.value, yagg.raw, cw.raw, [pts.raw[96 * i:96 * (i + 1)] for i in range(4)]


@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("count", [1, 2, 65, 130])  # 65 and 130 cross the 64 openings of a fold workgroup
def test_parts_equal_the_model_and_msm_in_one_chunk_and_in_many(eng, hooks, params, hook_srs, count, indexed):
    call = mixed_call(params, count)
    if not indexed:
        call = call.per_opening()
    n = len(call.commitments)
    r = random.Random(count).randrange(2, R)
    rho, rho_x, c, yagg = E.scalars(r, call.xs, call.ys, call.idx, n)
    got = parts(hooks, hook_srs, call, r)
    assert got[0] == 1
    assert got[1] == scalar(yagg) and got[2] == pack_scalars(c)
    if indexed:
        assert c[3] == 0  # the commitment no opening names
    ws, cs = kzg_amd.Srs.upload(eng, b"".join(call.witnesses), count), kzg_amd.Srs.upload(eng, b"".join(call.commitments), n)
    try:
        P1, P2, Cagg = eng.msm(ws, rho), eng.msm(ws, rho_x), eng.msm(cs, c)
    finally:
        ws.free()
        cs.free()
    assert got[3][:2] == [P1, P2]
    # third-set total - Ragg slot == sum_m c_m C_m - [yagg] gs[0]; this implementation carries -[yagg] gs[0] in the third set
    assert got[3][3] == IDENTITY
    assert got[3][2] == C.g1_add(Cagg, C.g1_mul(C.g1_generator(), (R - yagg) % R))
    assert parts(hooks, hook_srs, call, r, sfmt=L.FR_MONT) == got
    try:  # the finish in its kernel hands out the same four points
        assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"host_pairing", ctypes.c_int64(0)) == 0
        assert parts(hooks, hook_srs, call, r) == got
    finally:
        assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"host_pairing", ctypes.c_int64(1)) == 0
    try:  # the weights, the fold and the buckets across chunks
        for chunk in (5, 1):
            assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"verify_eval_batch_chunk", ctypes.c_int64(chunk)) == 0
            assert parts(hooks, hook_srs, call, r) == got, chunk
            assert E.scalars(r, call.xs, call.ys, call.idx, n, chunk) == (rho, rho_x, c, yagg)
    finally:
        assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"verify_eval_batch_chunk", ctypes.c_int64(0)) == 0
    # a tampered value moves yagg and the third set only, and the verdict
    bad = call.copy()
    bad.ys[count // 2] = (bad.ys[count // 2] + 1) % R
    moved = parts(hooks, hook_srs, bad, r)
    assert moved[0] == 0 and moved[1] != got[1] and moved[2] == got[2] and moved[3][:2] == got[3][:2] and moved[3][2] != got[3][2]


# ---- 2. across the slices of the variable-base sum ---------------------------------------------------------------------------------
def test_4099_openings_across_slices_agree_with_verify_eval(eng, params, plans):
    rng = random.Random(12)
    N = 1 << 12
    coeffs = rand_scalars(rng, N)
    poly, other = kzg_amd.Polynomial.new_from_coeffs(coeffs, N - 1), kzg_amd.Polynomial.new_from_coeffs(rand_scalars(rng, 6), 5)
    prover = kzg_amd.KZGProver(params)
    w = kzg_amd.compute_omega(N)[2]
    xs, x = [], 1
    for _ in range(N):
        xs.append(x)
        x = x * w % R
    ys = C.fft(coeffs)
    ws = prover.create_witness_all_points(poly, plans(12))
    extra = [rng.randrange(R) for _ in range(3)]
    ey = [E.poly_eval(other.slice_coeffs(), x) for x in extra]
    ew, fine = prover.create_witness_many(other, list(zip(extra, ey)))
    assert all(fine)
    call = Call(xs + extra, ys + ey, [prover.commit(poly), prover.commit(other)], [0] * N + [1] * 3, ws + ew)  # 2 x 2048 + 3
    r = rng.randrange(2, R)
    assert call.batch(eng, params, r) == (0, 1)
    assert all(call.each(eng, params))
    call.ys[2048] = (call.ys[2048] + 1) % R
    assert call.batch(eng, params, r) == (0, 0)
    assert [k for k, v in enumerate(call.each(eng, params)) if not v] == [2048]


# ---- 3. verdicts --------------------------------------------------------------------------------------------------------------------
def agree(eng, params, call, r):
    """the batch verdict, checked against all(kzg_verify_eval); the opening kzg_verify_eval names, or None"""
    rc, ok = call.batch(eng, params, r)
    assert rc == 0 and ok in (0, 1), eng.last_error()
    each = call.each(eng, params)
    assert bool(ok) == all(each), (ok, each)
    return [k for k, v in enumerate(each) if not v]


@pytest.mark.parametrize("indexed", [True, False])
def test_honest_openings_pass_and_every_single_tampering_fails(eng, params, indexed):
    call = mixed_call(params, 9, seed=1)
    if not indexed:
        call = call.per_opening()
    rng = random.Random(5)
    r = rng.randrange(2, R)
    assert agree(eng, params, call, r) == []
    assert agree(eng, params, call, R - 1) == []
    for k in (0, 4, 8):
        for field in ("xs", "ys"):
            bad = call.copy()
            getattr(bad, field)[k] = (getattr(bad, field)[k] + 1) % R
            assert agree(eng, params, bad, r) == [k], (field, k)
        bad = call.copy()
        bad.witnesses[k] = tamper_point(bad.witnesses[k])
        assert agree(eng, params, bad, r) == [k], ("witness", k)
    if indexed:
        for m in range(3):
            bad = call.copy()
            bad.commitments[m] = tamper_point(bad.commitments[m])
            assert agree(eng, params, bad, r) == [k for k in range(9) if call.idx[k] == m], ("commitment", m)
        bad = call.copy()
        bad.idx[4] = (bad.idx[4] + 1) % 3
        assert agree(eng, params, bad, r) == [4]
    else:
        bad = call.copy()
        bad.commitments[4] = tamper_point(bad.commitments[4])
        assert agree(eng, params, bad, r) == [4]


def test_compensating_pair_passes_at_r_1_only(eng, params):
    call = mixed_call(params, 9, seed=1)
    ka, kb = 0, 8  # mixed_call's duplicate: one commitment, one x
    assert (call.idx[ka], call.xs[ka]) == (call.idx[kb], call.xs[kb])
    D = M.g1_mul(M.G1, 0xD1FF)
    call.witnesses[ka] = C.point_to_blob(M.g1_add(C.blob_to_point(call.witnesses[ka]), D))
    call.witnesses[kb] = C.point_to_blob(M.g1_add(C.blob_to_point(call.witnesses[kb]), M.g1_neg(D)))
    assert call.batch(eng, params, 1) == (0, 1)  # the weights are all 1: the errors cancel
    assert call.batch(eng, params, random.Random(9).randrange(2, R)) == (0, 0)
    assert [k for k, v in enumerate(call.each(eng, params)) if not v] == [ka, kb]


# ---- 4. edge inputs -----------------------------------------------------------------------------------------------------------------
def test_edge_points_values_and_identities(eng, params):
    rng = random.Random(21)
    prover = kzg_amd.KZGProver(params)
    root = rng.randrange(R)
    q = rand_scalars(rng, 5)
    with_root = [(-root * q[0]) % R] + [(q[j - 1] - root * q[j]) % R for j in range(1, 5)] + [q[4]]  # (X - root) q(X): y = 0 at root
    poly = kzg_amd.Polynomial.new_from_coeffs(with_root, 5)
    const = kzg_amd.Polynomial.new_from_coeffs([0xC0FFEE], 0)
    d = 1 << 6
    dom = kzg_amd.EvaluationDomain.from_coeffs(rand_scalars(rng, d))
    small = kzg_amd.setup(eng, TAU, d, g2_len=2)
    lag = kzg_amd.setup_lagrange(eng, TAU, d)
    try:
        ev = kzg_amd.KZGProverEvalForm(small, lag)
        on_domain = [(pow(ev.omega(), i, R), dom.coeffs[i], ev.commit(dom), ev.create_witness(dom, i)) for i in (0, 5, d - 1)]
    finally:
        small.gs.free()
        small.hs.free()
        lag.free()
    xs = [0, R - 1, root, 7, 7, 12345, 99]
    ys = [E.poly_eval(with_root, x) for x in xs[:5]] + [0xC0FFEE, 0]
    assert ys[2] == 0
    ws, fine = prover.create_witness_many(poly, list(zip(xs[:5], ys[:5])))
    assert all(fine)
    cw = IDENTITY  # the witness of a constant polynomial, with C = [y] G
    assert prover.commit(const) == C.g1_mul(C.g1_generator(), 0xC0FFEE)
    call = Call(xs + [p[0] for p in on_domain], ys + [p[1] for p in on_domain],
                [prover.commit(poly), prover.commit(const), IDENTITY, on_domain[0][2]],  # the zero polynomial: the identity commitment
                [0, 0, 0, 0, 0, 1, 2, 3, 3, 3], ws + [cw, IDENTITY] + [p[3] for p in on_domain])
    assert call.xs[3] == call.xs[4] and call.witnesses[3] == call.witnesses[4]  # a duplicated opening
    r = rng.randrange(2, R)
    assert agree(eng, params, call, r) == []
    assert agree(eng, params, call.per_opening(), r) == []
    for k in range(len(call.xs)):
        bad = call.copy()
        bad.ys[k] = (bad.ys[k] + 1) % R
        assert agree(eng, params, bad, r) == [k]
    same_x = Call([7] * 4, [ys[3]] * 3 + [0xC0FFEE], call.commitments, [0, 0, 0, 1], [ws[3]] * 3 + [IDENTITY])  # all x equal
    assert agree(eng, params, same_x, r) == []
    same_x.ys[1] = 1
    assert agree(eng, params, same_x, r) == [1]
    # scalars as kzg_verify_eval takes them: not range-checked, a value >= the modulus counts as its residue
    big = call.copy()
    big.xs[3] += R
    big.ys[0] += R
    assert big.batch(eng, params, r) == (0, 1) and all(big.each(eng, params))


# ---- 5. formats and options ---------------------------------------------------------------------------------------------------------
def test_formats_host_pairing_and_trusted_points(eng, params):
    call = mixed_call(params, 9, seed=1)
    bad = call.copy()
    bad.ys[6] = (bad.ys[6] + 1) % R
    r = random.Random(4).randrange(2, R)
    try:
        for hp in (0, 1):
            eng.set_option("host_pairing", hp)
            for c in (call, call.per_opening()):
                assert c.batch(eng, params, r) == (0, 1), hp
            for c in (bad, bad.per_opening()):
                assert c.batch(eng, params, r) == (0, 0), hp
    finally:
        eng.set_option("host_pairing", 1)
    enc = {L.G1_AFFINE_MONT: M.g1_to_affine_mont, L.G1_ZCASH_UNCOMPRESSED: M.g1_to_uncompressed, L.G1_ZCASH_COMPRESSED: M.g1_to_compressed}
    for pfmt in AFFINE:
        for c, want in ((call, 1), (bad, 0)):
            f = c.copy()
            f.commitments = [bytes(enc[pfmt](C.blob_to_point(b))) for b in c.commitments]
            f.witnesses = [bytes(enc[pfmt](C.blob_to_point(b))) for b in c.witnesses]
            assert f.batch(eng, params, r, pfmt=pfmt) == (0, want), pfmt
            assert f.per_opening().batch(eng, params, r, pfmt=pfmt) == (0, want), pfmt
    for c, want in ((call, 1), (bad, 0)):  # with Montgomery scalars r travels in Montgomery form too
        assert c.batch(eng, params, r * MONT_R % R, sfmt=L.FR_MONT) == (0, want)
    try:
        for chunk in (5, 1):
            eng.set_option("verify_eval_batch_chunk", chunk)
            assert call.batch(eng, params, r) == (0, 1) and bad.batch(eng, params, r) == (0, 0)
            assert call.per_opening().batch(eng, params, r) == (0, 1) and bad.per_opening().batch(eng, params, r) == (0, 0)
    finally:
        eng.set_option("verify_eval_batch_chunk", 0)
    # on the curve, outside the r-torsion subgroup: rejected, unless the caller vouches for its points
    outside = C.point_to_blob(_non_subgroup_g1())
    for field, k in (("witnesses", 5), ("commitments", 1)):
        c = call.copy()
        getattr(c, field)[k] = outside
        assert c.batch(eng, params, r) == (L.KZG_ERR_BAD_POINT, UNTOUCHED)
        try:
            eng.set_option("trusted_points", 1)
            rc, ok = c.batch(eng, params, r)
            assert rc == 0 and ok in (0, 1)
        finally:
            eng.set_option("trusted_points", 0)


# ---- 6. validation ------------------------------------------------------------------------------------------------------------------
def test_validation_leaves_ok_untouched(eng, hooks, params, hook_srs):
    call = mixed_call(params, 9, seed=1)
    one = call.per_opening()
    gs, hs = params.gs.handle, params.hs.handle
    SHAPE, r = L.KZG_ERR_SHAPE, 12345

    def go(e=eng, gs=gs, hs=hs, c=call, r=r, **kw):
        return raw_batch(e, gs, hs, c.xs, c.ys, c.commitments, c.idx, c.witnesses, r, **kw)
    assert go() == (0, 1)
    for bad_r in (0, R, (1 << 256) - 1):
        assert go(r=bad_r) == (SHAPE, UNTOUCHED)
    assert go(r=R, sfmt=L.FR_MONT) == (SHAPE, UNTOUCHED)
    assert go(r=R - 1) == (0, 1)
    # gs without a point, hs with fewer than two
    empty, short = kzg_amd.Srs.upload(eng, b"", 0), kzg_amd.setup_g2(eng, TAU, 1)
    try:
        assert go(gs=empty.handle) == (SHAPE, UNTOUCHED)
        assert go(hs=short.handle) == (SHAPE, UNTOUCHED)
    finally:
        empty.free()
        short.free()
    assert go(gs=None) == (SHAPE, UNTOUCHED) and go(hs=None) == (SHAPE, UNTOUCHED)
    c = call.copy()
    c.idx[8] = 4  # an index >= n_commitments
    assert go(c=c) == (SHAPE, UNTOUCHED)
    c.idx[8] = (1 << 32) - 1
    assert go(c=c) == (SHAPE, UNTOUCHED)
    assert go(c=one) == (0, 1)
    assert go(c=one, n_commitments=8) == (SHAPE, UNTOUCHED)  # NULL indices with n_commitments != count
    assert go(c=one, n_commitments=10) == (SHAPE, UNTOUCHED)
    assert go(sfmt=2) == (SHAPE, UNTOUCHED)
    assert go(pfmt=7) == (SHAPE, UNTOUCHED)
    assert go(pfmt=L.G1_JACOBIAN_MONT) == (SHAPE, UNTOUCHED)
    for hole in ("xs", "ys", "commitments", "witnesses", "r"):
        a = dict(xs=call.xs, ys=call.ys, commitments=call.commitments, witnesses=call.witnesses, r=r)
        a[hole] = None
        assert raw_batch(eng, gs, hs, a["xs"], a["ys"], a["commitments"], call.idx, a["witnesses"], a["r"], count=9, n_commitments=4) \
            == (SHAPE, UNTOUCHED), hole
    assert go(ok=None)[0] == SHAPE
    # count == 0: *ok = 1, and a NULL ok is accepted
    assert go(count=0) == (0, 1)
    assert raw_batch(eng, gs, hs, None, None, None, None, None, None, count=0, n_commitments=0, ok=None)[0] == 0
    # a malformed witness or commitment: KZG_ERR_BAD_POINT
    off = bytearray(call.witnesses[3])
    off[0] ^= 1
    for field, k in (("witnesses", 3), ("commitments", 0), ("commitments", 3)):  # commitment 3 is named by no opening
        for c in (call.copy(), one.copy()):
            if k < len(getattr(c, field)):
                getattr(c, field)[k] = bytes(off)
                assert go(c=c) == (L.KZG_ERR_BAD_POINT, UNTOUCHED), (field, k)
    # an SRS on another GPU (the hooks build can pretend)
    hgs, hhs = hook_srs
    assert go(e=hooks, gs=hgs, hs=hhs) == (0, 1)
    for setter, h in ((hooks.lib.kzg_test_srs_set_device, hgs), (hooks.lib.kzg_test_srs_g2_set_device, hhs)):
        assert setter(h, 5) == 0
        try:
            assert go(e=hooks, gs=hgs, hs=hhs) == (SHAPE, UNTOUCHED)
            assert go(e=hooks, gs=hgs, hs=hhs, count=0) == (SHAPE, UNTOUCHED)
        finally:
            assert setter(h, 0) == 0
    assert go(e=hooks, gs=hgs, hs=hhs) == (0, 1)


# ---- 7. concurrency and the Python surface ------------------------------------------------------------------------------------------
def test_one_srs_two_contexts_four_threads(eng, params):
    call = mixed_call(params, 9, seed=1)
    bad = call.copy()
    bad.ys[2] = (bad.ys[2] + 1) % R
    call.batch(eng, params, 7)  # the argtypes are set before the threads start
    other = kzg_amd.Engine(0)
    out = {}

    def work(name, e):
        out[name] = [c.batch(e, params, 1000 + k) for k, c in enumerate((call, bad, call.per_opening()))]
    try:
        call.batch(other, params, 7)
        th = [threading.Thread(target=work, args=(n, e)) for n, e in (("a", eng), ("b", other), ("c", eng), ("d", other))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        other.close()
    assert len(out) == 4 and all(rs == [(0, 1), (0, 0), (0, 1)] for rs in out.values()), out


def test_cpp_wrapper(tmp_path):
    """KZGVerifier::verify_eval_batch of include/kzg_mi355x.hpp: tests/cpp_verify_eval_batch_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_verify_eval_batch_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_verify_eval_batch_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


def test_python_surface(eng, params, plans):
    call = mixed_call(params, 9, seed=1)
    one = call.per_opening()
    kv = kzg_amd.KZGVerifier(params)
    pts = list(zip(call.xs, call.ys))
    assert kv.verify_eval_batch(pts, call.commitments, call.witnesses, commitment_idx=call.idx) is True  # r drawn by the method
    assert kv.verify_eval_batch(pts, one.commitments, call.witnesses, r=5) is True
    assert kv.verify_eval_with_fallback(pts, call.commitments, call.witnesses, commitment_idx=call.idx) == [True] * 9
    bad = list(pts)
    bad[6] = (bad[6][0], (bad[6][1] + 1) % R)
    assert kv.verify_eval_batch(bad, call.commitments, call.witnesses, commitment_idx=call.idx) is False
    assert kv.verify_eval_batch(bad, one.commitments, call.witnesses, r=77) is False
    assert kv.verify_eval_with_fallback(bad, call.commitments, call.witnesses, commitment_idx=call.idx) == [k != 6 for k in range(9)]
    assert kv.verify_eval_with_fallback(bad, one.commitments, call.witnesses) == [k != 6 for k in range(9)]
    assert kv.verify_eval_batch([], [], []) is True
    for r in (0, R):
        with pytest.raises(kzg_amd.ReferencePanic):
            kv.verify_eval_batch(pts, one.commitments, call.witnesses, r=r)
    with pytest.raises(kzg_amd.ReferencePanic):
        kv.verify_eval_batch(pts, call.commitments, call.witnesses, commitment_idx=[4] * 9)
    with pytest.raises(kzg_amd.ReferencePanic):
        kv.verify_eval_batch(pts, call.commitments, call.witnesses)  # four commitments, nine openings, no indices
    # the evaluation form: points as (i, y); FK20's 2^6 proofs of one commitment with commitment_idx = [0] * 64
    rng = random.Random(8)
    d = 1 << 6
    small, lag = kzg_amd.setup(eng, TAU, d, g2_len=2), kzg_amd.setup_lagrange(eng, TAU, d)
    plan = kzg_amd.FK20Plan(eng, small.gs, 6)
    try:
        prover, ver = kzg_amd.KZGProverEvalForm(small, lag), kzg_amd.KZGVerifierEvalForm(small, lag)
        doms = [kzg_amd.EvaluationDomain.from_coeffs(rand_scalars(rng, d)) for _ in range(3)]
        cm = prover.commit(doms[0])
        proofs = prover.create_witness_all_points(doms[0], plan)
        ipts = [(i, doms[0].coeffs[i]) for i in range(d)]
        assert ver.verify_eval_batch(ipts, [cm], proofs, commitment_idx=[0] * d) is True
        assert ver.verify_eval_with_fallback(ipts, [cm], proofs, commitment_idx=[0] * d) == [True] * d
        ipts[40] = (40, (ipts[40][1] + 1) % R)
        assert ver.verify_eval_batch(ipts, [cm], proofs, r=3, commitment_idx=[0] * d) is False
        assert ver.verify_eval_with_fallback(ipts, [cm], proofs, commitment_idx=[0] * d) == [i != 40 for i in range(d)]
        # the blob shape: what open_at_batch produced, the claimed values recomputed from the evaluations
        zs = [rng.randrange(R), pow(prover.omega(), 5, R), 0]
        _ys, ws = prover.open_at_batch(doms, zs)
        cms = [prover.commit(dom) for dom in doms]
        assert ver.verify_open_at_batch(doms, zs, cms, ws) is True
        assert ver.verify_open_at_batch(doms, zs, cms, ws, r=11) is True
        changed = [kzg_amd.EvaluationDomain.from_coeffs(list(dom.coeffs)) for dom in doms]
        changed[0].coeffs[9] = (changed[0].coeffs[9] + 1) % R  # zs[0] is off the domain: p(z) depends on every evaluation
        assert ver.verify_open_at_batch(changed, zs, cms, ws) is False
    finally:
        plan.free()
        small.gs.free()
        small.hs.free()
        lag.free()
