"""kzg_verify_cosets_batch (kzg_amd/csrc/verify_cosets_batch.hip): one verdict per call from one pairing check.  The variable-base
multi-scalar sum alone through its hook (bit-exact against kzg_msm_g1 on the same SRS), the scalars and the four points of the
combination against the model (tests/verify_cosets_batch_model.py) and kzg_msm_g1, the verdicts for honest, tampered and compensating
cells against kzg_verify_cosets, options, formats, validation, concurrency and the Python surface.  Like
tests/test_gpu_verify_cosets.py, whose cells and fixtures it shares, this file opens and closes its own module-scoped Engine and
HooksEngine."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import verify_cosets_batch_model as B
from tests.fk20_common import MONT_R, SIZE_MAX, VP, SZ, I32, U32
from tests.fk20_common import eng, hooks, params, plans  # noqa: F401 -- this module's fixtures
from tests.gpu_common import rand_scalars
from tests.test_gpu_verify_cosets import AFFINE, G2_LEN, PLAN, SRS_LEN, TAU, U32P, SZP  # noqa: F401 -- read by the fixtures
from tests.test_gpu_verify_cosets import hook_plans, verifiers  # noqa: F401 -- fixtures
from tests.test_gpu_verify_cosets import flat, opened, raw_verify
from tests.test_gpu_validation import _non_subgroup_g1

pytestmark = pytest.mark.gpu

R = M.R
S = 2048  # VCB_S: points per slice of the variable-base sum
UNTOUCHED = 0x5A5A5A5A
SHAPES = [(10, 4), (8, 6), (6, 0), (4, 4)]
BATCH_ARGS = [VP, VP, VP, SZ, U32P, SZP, VP, VP, SZ, VP, I32, I32, I32, ctypes.POINTER(I32)]


def scalar(x):
    return (x % (1 << 256)).to_bytes(32, "little")


def raw_batch(e, plan, commitments, idx, ids, cells, proofs, r, sfmt=L.FR_CANONICAL, pfmt=L.G1_AFFINE_MONT, flags=0, count=None,
              n_commitments=None, ok="own"):
    """(rc, *ok) of one kzg_verify_cosets_batch call; *ok starts as UNTOUCHED.  cells: a blob or a device pointer; r: an int or None"""
    count = len(proofs) if count is None else count
    okv = I32(UNTOUCHED)
    if e.lib.kzg_verify_cosets_batch.argtypes != BATCH_ARGS:  # (the hooks library; set before any thread calls)
        e.lib.kzg_verify_cosets_batch.argtypes = BATCH_ARGS
        e.lib.kzg_verify_cosets_batch.restype = I32
    rc = e.lib.kzg_verify_cosets_batch(e.ctx, plan, b"".join(commitments) if commitments is not None else None,
                                       len(commitments) if n_commitments is None else n_commitments,
                                       (U32 * max(len(idx), 1))(*idx) if idx is not None else None,
                                       (SZ * max(len(ids), 1))(*ids) if ids is not None else None, cells,
                                       b"".join(proofs) if proofs is not None else None, count, scalar(r) if r is not None else None, sfmt, pfmt,
                                       flags, ctypes.byref(okv) if ok == "own" else None)
    return rc, okv.value


def mixed_call(eng, params, plans, log_n, log_l, count=24):
    """(commitments, idx, ids, cells, proofs): honest cells of two polynomials in random order, with a duplicate (commitment, coset)"""
    K = 1 << (log_n - log_l)
    polys = [opened(eng, params, plans, log_n, log_l, seed=s) for s in (0, 1)]
    rng = random.Random(31 * log_n + log_l)
    idx = [rng.randrange(2) for _ in range(count)]
    ids = [rng.randrange(K) for _ in range(count)]
    idx[-1], ids[-1] = idx[0], ids[0]
    return [p[0] for p in polys], idx, ids, [list(polys[m][1][i]) for m, i in zip(idx, ids)], [polys[m][2][i] for m, i in zip(idx, ids)]


def tamper_point(blob, k=1):
    """another point of the subgroup: blob + [k]G"""
    return C.point_to_blob(M.g1_add(C.blob_to_point(blob), M.g1_mul(M.G1, k)))


# ---- 1. the variable-base sum alone, bit-exact against kzg_msm_g1 on the same SRS ----------------------------------------------
@pytest.fixture(scope="module")
def vb(hooks):
    lib = hooks.lib
    lib.kzg_srs_setup_g1.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    lib.kzg_srs_upload_g1.argtypes = [VP, VP, SZ, I32, ctypes.POINTER(VP)]
    lib.kzg_srs_free.argtypes = [VP, VP]
    lib.kzg_srs_free.restype = None
    lib.kzg_msm_g1.argtypes = [VP, VP, SZ, VP, SZ, I32, I32, VP, I32]
    lib.kzg_msm_g1.restype = I32
    lib.kzg_test_vb_msm.argtypes = [VP, VP, SZ, VP, SZ, I32, VP]
    lib.kzg_test_vb_msm.restype = I32
    gs = VP()
    assert lib.kzg_srs_setup_g1(hooks.ctx, scalar(TAU), L.FR_CANONICAL, 2 * S + 16, ctypes.byref(gs)) == 0

    def both(scalars, offset=0, sfmt=L.FR_CANONICAL, srs=gs):
        """(the variable-base sum, kzg_msm_g1) of the same arguments"""
        blob, got, want = pack_scalars(scalars), ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        assert lib.kzg_test_vb_msm(hooks.ctx, srs, offset, blob, len(scalars), sfmt, got) == 0, hooks.last_error()
        assert lib.kzg_msm_g1(hooks.ctx, srs, offset, blob, len(scalars), sfmt, 0, want, L.G1_AFFINE_MONT) == 0, hooks.last_error()
        return got.raw, want.raw
    yield both
    lib.kzg_srs_free(hooks.ctx, gs)


def test_vb_msm_sizes_formats_and_offset(vb):
    sc = rand_scalars(random.Random(1), 2 * S + 3)
    for n in (1, 2, S - 1, S, S + 1, 2 * S + 3):
        got, want = vb(sc[:n])
        assert got == want and got != bytes(96), n
    got, want = vb([s * MONT_R % R for s in sc[:S + 1]], sfmt=L.FR_MONT)
    assert got == want == vb(sc[:S + 1])[0]
    got, want = vb(sc[:S + 1], offset=5)
    assert got == want != vb(sc[:S + 1])[0]
    got, want = vb([s * MONT_R % R for s in sc[:130]], offset=2 * S + 16 - 130, sfmt=L.FR_MONT)  # up to the SRS's last point
    assert got == want


def test_vb_msm_special_scalars(vb, hooks):
    carries = int("80" * 31, 16)  # every digit of the low 31 windows is -128 with a carry into the next
    special = [0, 1, R - 1, carries, int("80" * 32, 16) % R, ((1 << 255) - 1) % R, R - 2, int("ff" * 31, 16), int("7f" * 32, 16) % R]
    for s in special:  # one value for all points: every point of a window in ONE bucket (or in none)
        got, want = vb([s] * 200)
        assert got == want, hex(s)
    got, want = vb([special[k % len(special)] for k in range(S + 1)])
    assert got == want
    assert vb([0] * (S + 1)) == (bytes(96), bytes(96))
    # equal and opposite points in one bucket: [P, P, -P, Q, -Q] with all scalars 1 sums to P
    P, Q = M.g1_mul(M.G1, 7), M.g1_mul(M.G1, 11)
    pts = [P, P, M.g1_neg(P), Q, M.g1_neg(Q)]
    h = VP()
    assert hooks.lib.kzg_srs_upload_g1(hooks.ctx, b"".join(C.point_to_blob(p) for p in pts), 5, L.G1_AFFINE_MONT, ctypes.byref(h)) == 0
    try:
        assert vb([1] * 5, srs=h) == (C.point_to_blob(P),) * 2
        assert vb([R - 1] * 5, srs=h) == (C.point_to_blob(M.g1_neg(P)),) * 2
        assert vb([3, 3, 3, 128, 128], srs=h) == (C.point_to_blob(M.g1_mul(P, 3)),) * 2
    finally:
        hooks.lib.kzg_srs_free(hooks.ctx, h)


# ---- 2. the parts of the combination ------------------------------------------------------------------------------------------
def parts(hooks, plan, commitments, idx, ids, cells, proofs, r, sfmt=L.FR_CANONICAL):
    lib = hooks.lib
    lib.kzg_test_verify_cosets_batch_parts.argtypes = BATCH_ARGS + [VP, VP, VP]
    lib.kzg_test_verify_cosets_batch_parts.restype = I32
    l = len(cells[0])
    vals = [v for c in cells for v in c]
    blob = pack_scalars(vals if sfmt == L.FR_CANONICAL else [v * MONT_R % R for v in vals])
    rr = r if sfmt == L.FR_CANONICAL else r * MONT_R % R
    a, cw, pts, ok = ctypes.create_string_buffer(32 * l), ctypes.create_string_buffer(32 * len(commitments)), ctypes.create_string_buffer(4 * 96), I32(UNTOUCHED)
    rc = lib.kzg_test_verify_cosets_batch_parts(hooks.ctx, plan, b"".join(commitments), len(commitments), (U32 * len(idx))(*idx), (SZ * len(ids))(*ids),
                                                blob, b"".join(proofs), len(proofs), scalar(rr), sfmt, L.G1_AFFINE_MONT, 0, ctypes.byref(ok), a, cw, pts)
    assert rc == 0, hooks.last_error()
    return ok.value, a.raw, cw.raw, [pts.raw[96 * i:96 * (i + 1)] for i in range(4)]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_parts_equal_the_model_and_msm_in_one_chunk_and_in_many(eng, hooks, params, plans, hook_plans, log_n, log_l):
    commitments, idx, ids, cells, proofs = mixed_call(eng, params, plans, log_n, log_l)
    r = random.Random(log_n).randrange(2, R)
    a, c, rho, rho_h = B.scalars(r, idx, ids, cells, 2, log_n, log_l)
    plan = hook_plans(log_n, log_l)
    got = parts(hooks, plan, commitments, idx, ids, cells, proofs, r)
    assert got[0] == 1
    assert got[1] == pack_scalars(a) and got[2] == pack_scalars(c)
    ps, cs = kzg_amd.Srs.upload(eng, b"".join(proofs), len(proofs)), kzg_amd.Srs.upload(eng, b"".join(commitments), 2)
    try:
        want = [eng.msm(ps, rho), eng.msm(ps, rho_h), eng.msm(cs, c), eng.msm(params.gs, a, 1 << log_l)]
    finally:
        ps.free()
        cs.free()
    assert got[3] == want
    assert parts(hooks, plan, commitments, idx, ids, cells, proofs, r, sfmt=L.FR_MONT) == got
    try:  # the weights and the buckets across chunks: 24 = 5 + 5 + 5 + 5 + 4, and one cell per chunk
        for chunk in (5, 1):
            assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"verify_cosets_chunk", ctypes.c_int64(chunk)) == 0
            assert parts(hooks, plan, commitments, idx, ids, cells, proofs, r) == got, chunk
    finally:
        assert hooks.lib.kzg_ctx_set_option(hooks.ctx, b"verify_cosets_chunk", ctypes.c_int64(0)) == 0
    # a tampered value moves a and Ragg only, and the verdict
    bad = [list(v) for v in cells]
    bad[3][0] = (bad[3][0] + 1) % R
    moved = parts(hooks, plan, commitments, idx, ids, bad, proofs, r)
    assert moved[0] == 0 and moved[1] != got[1] and moved[2] == got[2] and moved[3][:3] == got[3][:3] and moved[3][3] != got[3][3]


# ---- 3. verdicts --------------------------------------------------------------------------------------------------------------
def agree(eng, ver, commitments, idx, ids, cells, proofs, r):
    """the batch verdict, checked against all(kzg_verify_cosets)"""
    rc, ok = raw_batch(eng, ver.handle, commitments, idx, ids, flat(cells), proofs, r)
    assert rc == 0 and ok in (0, 1), eng.last_error()
    rc1, each = raw_verify(eng, ver.handle, commitments, idx, ids, flat(cells), proofs)
    assert rc1 == 0 and bool(ok) == all(each), (ok, each)
    return bool(ok)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_honest_cells_pass_and_every_single_tampering_fails(eng, params, plans, verifiers, log_n, log_l):
    commitments, idx, ids, cells, proofs = mixed_call(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    rng = random.Random(log_l)
    r = rng.randrange(2, R)
    assert agree(eng, ver, commitments, idx, ids, cells, proofs, r)
    assert agree(eng, ver, commitments, idx, ids, cells, proofs, 1)
    for k in (0, 7, len(ids) - 1):
        bad = [list(v) for v in cells]
        bad[k][rng.randrange(1 << log_l)] = (bad[k][0] + 1) % R
        assert not agree(eng, ver, commitments, idx, ids, bad, proofs, r), ("value", k)
        p = list(proofs)
        p[k] = tamper_point(p[k])
        assert not agree(eng, ver, commitments, idx, ids, cells, p, r), ("proof", k)
    for m in (0, 1):
        cm = list(commitments)
        cm[m] = tamper_point(cm[m])
        assert not agree(eng, ver, cm, idx, ids, cells, proofs, r), ("commitment", m)
    assert not agree(eng, ver, commitments, [1 - m for m in idx], ids, cells, proofs, r)


def test_compensating_pair_passes_at_r_1_only(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    commitments, idx, ids, cells, proofs = mixed_call(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    ka, kb = 0, len(ids) - 1  # mixed_call's duplicate: the same commitment and coset
    assert (idx[ka], ids[ka]) == (idx[kb], ids[kb])
    D = M.g1_mul(M.G1, 0xD1FF)
    p = list(proofs)
    p[ka] = C.point_to_blob(M.g1_add(C.blob_to_point(p[ka]), D))
    p[kb] = C.point_to_blob(M.g1_add(C.blob_to_point(p[kb]), M.g1_neg(D)))
    blob = flat(cells)
    assert raw_batch(eng, ver.handle, commitments, idx, ids, blob, p, 1) == (0, 1)  # the weights are all 1: the errors cancel
    assert raw_batch(eng, ver.handle, commitments, idx, ids, blob, p, random.Random(9).randrange(2, R)) == (0, 0)
    each = raw_verify(eng, ver.handle, commitments, idx, ids, blob, p)[1]
    assert [k for k, v in enumerate(each) if not v] == [ka, kb]


def test_identity_proofs(eng, params, plans, verifiers):
    log_n, log_l = 6, 3
    K = 8
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l, n=5)
    assert all(p == bytes(96) for p in proofs)  # n <= l: FK20 emits the identity, r = p
    ver = verifiers(log_n, log_l)
    r = random.Random(3).randrange(2, R)
    assert agree(eng, ver, [C0], [0] * K, list(range(K)), cells, proofs, r)
    bad = [list(v) for v in cells]
    bad[K - 1][2] = (bad[K - 1][2] + 1) % R
    assert not agree(eng, ver, [C0], [0] * K, list(range(K)), bad, proofs, r)
    # together with cells that have proofs, three commitments
    full = [opened(eng, params, plans, log_n, log_l, seed=s) for s in (0, 1)]
    cm = [full[0][0], C0, full[1][0]]
    idx = [k % 3 for k in range(3 * K)]
    ids = [k // 3 for k in range(3 * K)]
    src = [full[0], (C0, cells, proofs), full[1]]
    assert agree(eng, ver, cm, idx, ids, [src[m][1][i] for m, i in zip(idx, ids)], [src[m][2][i] for m, i in zip(idx, ids)], r)
    assert not agree(eng, ver, cm, [(m + 1) % 3 for m in idx], ids, [src[m][1][i] for m, i in zip(idx, ids)], [src[m][2][i] for m, i in zip(idx, ids)], r)


# ---- 4. options and formats ---------------------------------------------------------------------------------------------------
def test_host_pairing_formats_and_device_cells(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    K, l = 16, 4
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    bad = [list(c) for c in cells]
    bad[11][0] = (bad[11][0] + 1) % R
    ids, idx = list(range(K)), [0] * K
    r = random.Random(4).randrange(2, R)
    try:
        for hp in (0, 1):
            eng.set_option("host_pairing", hp)
            assert raw_batch(eng, ver.handle, [C0], idx, ids, flat(cells), proofs, r) == (0, 1), hp
            assert raw_batch(eng, ver.handle, [C0], idx, ids, flat(bad), proofs, r) == (0, 0), hp
    finally:
        eng.set_option("host_pairing", 1)
    P = [C.blob_to_point(b) for b in [C0] + proofs]
    enc = {L.G1_AFFINE_MONT: M.g1_to_affine_mont, L.G1_ZCASH_UNCOMPRESSED: M.g1_to_uncompressed, L.G1_ZCASH_COMPRESSED: M.g1_to_compressed}
    for pfmt in AFFINE:
        pts = [bytes(enc[pfmt](p)) for p in P]
        assert raw_batch(eng, ver.handle, pts[:1], idx, ids, flat(cells), pts[1:], r, pfmt=pfmt) == (0, 1), pfmt
        assert raw_batch(eng, ver.handle, pts[:1], idx, ids, flat(bad), pts[1:], r, pfmt=pfmt) == (0, 0), pfmt
    for cs, want in ((cells, 1), (bad, 0)):
        mont = pack_scalars([v * MONT_R % R for c in cs for v in c])
        assert raw_batch(eng, ver.handle, [C0], idx, ids, mont, proofs, r * MONT_R % R, sfmt=L.FR_MONT) == (0, want)
        for blob, sfmt, rr in ((flat(cs), L.FR_CANONICAL, r), (mont, L.FR_MONT, r * MONT_R % R)):
            buf = kzg_amd.DeviceBuffer(eng, K * l, sfmt).upload(blob)
            try:
                assert raw_batch(eng, ver.handle, [C0], idx, ids, buf.ptr, proofs, rr, sfmt=sfmt, flags=L.IN_DEVICE) == (0, want)
                assert ver.verify_batch([C0], idx, ids, buf, proofs, r=r) == bool(want)
            finally:
                buf.free()
    try:
        for chunk in (5, 1):
            eng.set_option("verify_cosets_chunk", chunk)
            assert raw_batch(eng, ver.handle, [C0], idx, ids, flat(cells), proofs, r) == (0, 1)
            assert raw_batch(eng, ver.handle, [C0], idx, ids, flat(bad), proofs, r) == (0, 0)
    finally:
        eng.set_option("verify_cosets_chunk", 0)


# ---- 5. validation ------------------------------------------------------------------------------------------------------------
def test_validation_leaves_ok_untouched(eng, hooks, params, plans, verifiers, hook_plans):
    log_n, log_l = 6, 2
    K = 16
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    ids, idx, blob = list(range(K)), [0] * K, flat(cells)
    SHAPE, r = L.KZG_ERR_SHAPE, 12345
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r) == (0, 1)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, 0) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, R) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, (1 << 256) - 1) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, R, sfmt=L.FR_MONT) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, R - 1) == (0, 1)
    assert raw_batch(eng, ver.handle, [C0], idx, ids[:-1] + [K], blob, proofs, r) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids[:-1] + [SIZE_MAX], blob, proofs, r) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx[:-1] + [1], ids, blob, proofs, r) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r, sfmt=2) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r, pfmt=7) == (SHAPE, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r, pfmt=L.G1_JACOBIAN_MONT) == (SHAPE, UNTOUCHED)
    for hole in ("commitments", "idx", "ids", "cells", "proofs", "r"):
        a = dict(commitments=[C0], idx=idx, ids=ids, cells=blob, proofs=proofs, r=r)
        a[hole] = None
        assert raw_batch(eng, ver.handle, a["commitments"], a["idx"], a["ids"], a["cells"], a["proofs"], a["r"], count=K, n_commitments=1) \
            == (SHAPE, UNTOUCHED), hole
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r, ok=None)[0] == SHAPE
    assert raw_batch(eng, None, [C0], idx, ids, blob, proofs, r) == (SHAPE, UNTOUCHED)
    # count == 0: *ok = 1, and a NULL ok is accepted
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs, r, count=0) == (0, 1)
    assert raw_batch(eng, ver.handle, None, None, None, None, None, None, count=0, n_commitments=0, ok=None)[0] == 0
    # an off-curve proof or commitment, a proof outside the subgroup: KZG_ERR_BAD_POINT
    off = bytearray(proofs[3])
    off[0] ^= 1
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs[:3] + [bytes(off)] + proofs[4:], r) == (L.KZG_ERR_BAD_POINT, UNTOUCHED)
    assert raw_batch(eng, ver.handle, [bytes(off)], idx, ids, blob, proofs, r) == (L.KZG_ERR_BAD_POINT, UNTOUCHED)
    outside = C.point_to_blob(_non_subgroup_g1())  # on the curve, outside the r-torsion subgroup
    assert raw_batch(eng, ver.handle, [C0], idx, ids, blob, proofs[:5] + [outside] + proofs[6:], r) == (L.KZG_ERR_BAD_POINT, UNTOUCHED)
    # a plan on another GPU (the hooks build can pretend)
    hooks.lib.kzg_test_cosets_verifier_set_device.argtypes = [VP, I32]
    hp = hook_plans(log_n, log_l)
    assert raw_batch(hooks, hp, [C0], idx, ids, blob, proofs, r) == (0, 1)
    assert hooks.lib.kzg_test_cosets_verifier_set_device(hp, 5) == 0
    try:
        assert raw_batch(hooks, hp, [C0], idx, ids, blob, proofs, r) == (SHAPE, UNTOUCHED)
        assert raw_batch(hooks, hp, [C0], idx, ids, blob, proofs, r, count=0) == (SHAPE, UNTOUCHED)
    finally:
        assert hooks.lib.kzg_test_cosets_verifier_set_device(hp, 0) == 0
    assert raw_batch(hooks, hp, [C0], idx, ids, blob, proofs, r) == (0, 1)


# ---- 6. concurrency and the Python surface ------------------------------------------------------------------------------------
def test_one_plan_two_contexts_three_threads(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    K = 16
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    bad = [list(c) for c in cells]
    bad[4][1] = (bad[4][1] + 1) % R
    good_blob, bad_blob, ids, idx = flat(cells), flat(bad), list(range(K)), [0] * K
    raw_batch(eng, ver.handle, [C0], idx, ids, good_blob, proofs, 7)  # the argtypes are set before the threads start
    other = kzg_amd.Engine(0)
    out = {}

    def work(name, e):
        out[name] = [raw_batch(e, ver.handle, [C0], idx, ids, blob, proofs, 1000 + k) for k, blob in enumerate((good_blob, bad_blob, good_blob))]
    try:
        raw_batch(other, ver.handle, [C0], idx, ids, good_blob, proofs, 7)
        th = [threading.Thread(target=work, args=(n, e)) for n, e in (("a", eng), ("b", other), ("c", eng), ("d", eng))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        other.close()
    assert len(out) == 4 and all(rs == [(0, 1), (0, 0), (0, 1)] for rs in out.values()), out


def test_python_surface(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    K = 16
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver, kv = verifiers(log_n, log_l), kzg_amd.KZGVerifier(params)
    ids, idx = list(range(K)), [0] * K
    assert ver.verify_batch([C0], idx, ids, cells, proofs) is True  # r drawn by the method
    assert ver.verify_batch([C0], idx, ids, cells, proofs, r=5) is True
    assert kv.verify_cosets_batch(ver, C0, ids, cells, proofs) is True
    assert ver.verify_with_fallback([C0], idx, ids, cells, proofs) == [True] * K
    bad = [list(c) for c in cells]
    bad[9][3] = (bad[9][3] + 1) % R
    assert ver.verify_batch([C0], idx, ids, bad, proofs) is False
    assert kv.verify_cosets_batch(ver, C0, ids, bad, proofs, r=77) is False
    assert ver.verify_with_fallback([C0], idx, ids, bad, proofs) == [k != 9 for k in range(K)]
    assert ver.verify_batch([C0], [], [], [], []) is True
    for r in (0, R):
        with pytest.raises(kzg_amd.ReferencePanic):
            ver.verify_batch([C0], idx, ids, cells, proofs, r=r)
    with pytest.raises(kzg_amd.ReferencePanic):
        ver.verify_batch([C0], [0], [K], [cells[0]], [proofs[0]])
    with pytest.raises(kzg_amd.ReferencePanic):
        ver.verify_batch([C0], [0], [0], cells[0][:3], [proofs[0]])
