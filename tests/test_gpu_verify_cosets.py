"""kzg_verify_cosets (kzg_amd/csrc/verify_cosets.hip): one verdict per cell for the openings kzg_witness_cosets_coeff produces.  The
interpolation and the fixed-base sum alone through their hook (bit-exact against the FK20 call's out_r and against kzg_msm_g1), the
verdicts for honest and tampered cells, agreement with kzg_verify_eval_batched, formats, flags, chunks, validation and the Python
surface.  Like tests/test_gpu_fk20_cosets.py this file sorts after the tests that release the session's contexts, so it opens and
closes its own module-scoped Engine and HooksEngine."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests.fk20_common import MONT_R, SIZE_MAX, VP, SZ, I32, U32
from tests.fk20_common import eng, hooks, params, plans  # noqa: F401 -- this module's fixtures
from tests.gpu_common import rand_scalars

pytestmark = pytest.mark.gpu

TAU = 0x5EED_CE115
SRS_LEN = 1 << 10
G2_LEN = 257  # hs[l] for cosets of up to 256 points
PLAN = kzg_amd.FK20CosetPlan
AFFINE = [L.G1_AFFINE_MONT, L.G1_ZCASH_UNCOMPRESSED, L.G1_ZCASH_COMPRESSED]
U32P, SZP = ctypes.POINTER(U32), ctypes.POINTER(SZ)


@pytest.fixture(scope="module")
def verifiers(eng, params):
    cache = {}

    def get(log_n, log_l):
        if (log_n, log_l) not in cache:
            cache[(log_n, log_l)] = kzg_amd.CosetVerifier(eng, params, log_n, log_l)
        return cache[(log_n, log_l)]
    yield get
    for v in cache.values():
        v.free()


@pytest.fixture(scope="module")
def hook_plans(hooks):
    """hook_plans(log_n, log_l): a kzg_cosets_verifier in the hooks build of the library (its own context and SRS, the same tau)"""
    lib = hooks.lib
    lib.kzg_srs_setup_g1.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    lib.kzg_srs_setup_g2.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    lib.kzg_srs_free.argtypes = lib.kzg_srs_g2_free.argtypes = lib.kzg_cosets_verifier_free.argtypes = [VP, VP]
    lib.kzg_srs_free.restype = lib.kzg_srs_g2_free.restype = lib.kzg_cosets_verifier_free.restype = None
    lib.kzg_cosets_verifier_setup.argtypes = [VP, VP, VP, U32, U32, ctypes.POINTER(VP)]
    lib.kzg_test_verify_cosets_stage.argtypes = [VP, VP, I32, SZP, VP, SZ, I32, VP]
    lib.kzg_test_verify_cosets_stage.restype = I32
    gs, hs = VP(), VP()
    tau = TAU.to_bytes(32, "little")
    assert lib.kzg_srs_setup_g1(hooks.ctx, tau, L.FR_CANONICAL, 256, ctypes.byref(gs)) == 0
    assert lib.kzg_srs_setup_g2(hooks.ctx, tau, L.FR_CANONICAL, G2_LEN, ctypes.byref(hs)) == 0
    cache = {}

    def get(log_n, log_l):
        if (log_n, log_l) not in cache:
            h = VP()
            assert lib.kzg_cosets_verifier_setup(hooks.ctx, gs, hs, log_n, log_l, ctypes.byref(h)) == 0, hooks.last_error()
            cache[(log_n, log_l)] = h
        return cache[(log_n, log_l)]
    yield get
    for h in cache.values():
        lib.kzg_cosets_verifier_free(hooks.ctx, h)
    lib.kzg_srs_free(hooks.ctx, gs)
    lib.kzg_srs_g2_free(hooks.ctx, hs)


def stage(hooks, plan, which, ids, scalars, count, sfmt=L.FR_CANONICAL, out_bytes=None):
    blob = pack_scalars(scalars)
    out = ctypes.create_string_buffer(out_bytes if out_bytes is not None else len(blob))
    id_arr = (SZ * max(count, 1))(*ids) if ids is not None else None
    rc = hooks.lib.kzg_test_verify_cosets_stage(hooks.ctx, plan, which, id_arr, blob, count, sfmt, out)
    assert rc == 0, hooks.last_error()
    return out.raw


_OPENED = {}


def opened(eng, params, plans, log_n, log_l, n=None, seed=0):
    """(commitment, cells, proofs, r): every cell of one random polynomial of n coefficients with its FK20 proof (affine Montgomery)
    and its interpolant bytes (canonical), computed once per shape and left unchanged"""
    key = (log_n, log_l, n, seed)
    if key in _OPENED:
        return _OPENED[key]
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    n = N if n is None else n
    coeffs = rand_scalars(random.Random(1000 * log_n + 10 * log_l + seed), n)
    ev = C.fft(coeffs + [0] * (N - n)) if N > 1 else list(coeffs)
    cells = [[ev[i + t * K] for t in range(l)] for i in range(K)]
    poly = kzg_amd.Polynomial.new_from_coeffs(coeffs, n - 1)
    prover = kzg_amd.KZGProver(params)
    commitment = prover.commit(poly)
    if log_l == 0:  # single points: the FK20 call of that case; the interpolant of one value is the value
        plan = kzg_amd.FK20Plan(eng, params.gs, log_n)
        try:
            proofs = prover.create_witness_all_points(poly, plan)
        finally:
            plan.free()
        r = pack_scalars(ev)
    else:
        plan = plans(log_n, log_l)
        w = ctypes.create_string_buffer(96 * K)
        rb = ctypes.create_string_buffer(32 * N)
        rc = eng.lib.kzg_witness_cosets_coeff(eng.ctx, plan.handle, pack_scalars(coeffs), n, 1, L.FR_CANONICAL, 0, w, L.G1_AFFINE_MONT, rb)
        assert rc == 0, eng.last_error()
        proofs, r = [w.raw[i * 96:(i + 1) * 96] for i in range(K)], rb.raw
    _OPENED[key] = (commitment, cells, proofs, r)
    return _OPENED[key]


def raw_verify(eng, plan, commitments, idx, ids, cells, proofs, sfmt=L.FR_CANONICAL, pfmt=L.G1_AFFINE_MONT, flags=0, ok=None, count=None,
               n_commitments=None):
    """(rc, ok bytes) of one kzg_verify_cosets call; cells: a blob or a device pointer"""
    count = len(proofs) if count is None else count
    okb = ok if ok is not None else ctypes.create_string_buffer(b"\xa5" * max(count, 1), max(count, 1))
    rc = eng.lib.kzg_verify_cosets(eng.ctx, plan, b"".join(commitments) if commitments is not None else None,
                                   len(commitments) if n_commitments is None else n_commitments,
                                   (U32 * max(len(idx), 1))(*idx) if idx is not None else None,
                                   (SZ * max(len(ids), 1))(*ids) if ids is not None else None, cells,
                                   b"".join(proofs) if proofs is not None else None, count, sfmt, pfmt, flags, okb)
    return rc, okb.raw[:count]


def flat(cells):
    return pack_scalars([v for c in cells for v in c])


# ---- 1. the interpolation alone, bit-exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(1, 0), (2, 1), (4, 4), (6, 3), (10, 4), (10, 6), (10, 8)])
def test_interpolation_equals_the_fk20_interpolants(eng, hooks, params, plans, hook_plans, log_n, log_l):
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    _c, cells, _p, r = opened(eng, params, plans, log_n, log_l)
    ids = list(range(K)) if K <= 64 else sorted(set(random.Random(log_n).sample(range(K), 30)) | {0, 1, K - 1})
    vals = [v for i in ids for v in cells[i]]
    want = b"".join(r[i * l * 32:(i + 1) * l * 32] for i in ids)
    plan = hook_plans(log_n, log_l)
    assert stage(hooks, plan, 0, ids, vals, len(ids)) == want
    mont = stage(hooks, plan, 0, ids, [v * MONT_R % M.R for v in vals], len(ids), L.FR_MONT)
    assert mont == pack_scalars([int.from_bytes(want[k:k + 32], "little") * MONT_R % M.R for k in range(0, len(want), 32)])
    # the values 0, 1 and r - 1, against the interpolation of the model's formula on the device's own linearity: a cell of one
    # repeated value c interpolates to the constant c, and the cell (0, .., 0, 1 at t, 0, ..) to u_j = nu^(-jt) w^(-ij) / l
    i = ids[-1]
    for c in (0, 1, M.R - 1):
        assert stage(hooks, plan, 0, [i], [c] * l, 1) == pack_scalars([c] + [0] * (l - 1))
    w = M.compute_omega(N)[2]
    t = l - 1
    unit = [0] * t + [M.R - 1]
    want_u = [(M.R - 1) * pow(l, -1, M.R) * pow(w, -((K * j * t + i * j) % N), M.R) % M.R for j in range(l)]
    assert stage(hooks, plan, 0, [i], unit, 1) == pack_scalars(want_u)


# ---- 2. the fixed-base sum alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_l", [0, 1, 4, 6, 8])
def test_fixed_base_sum_equals_msm(eng, hooks, params, hook_plans, log_l):
    l = 1 << log_l
    rng = random.Random(40 + log_l)
    plan = hook_plans(max(log_l, 1), log_l)
    # every window digit at its extremes: 0, 1, r - 1, all-ones bytes, 0x7f.. / 0x80.. bytes (digits +-128, carries into every
    # window including the top one), and random scalars
    special = [0, 1, M.R - 1, M.R - 2, (1 << 255) - 1 - M.R, int("7f" * 32, 16) % M.R, int("80" * 31, 16), int("ff" * 31, 16), (1 << 248) - 1,
               int("0180" * 15, 16)]
    rows = [[special[(j + k) % len(special)] for j in range(l)] for k in range(len(special))] + [rand_scalars(rng, l) for _ in range(3)]
    rows.append([0] * l)
    got = stage(hooks, plan, 1, None, [s for row in rows for s in row], len(rows), out_bytes=96 * len(rows))
    for k, row in enumerate(rows):
        assert got[k * 96:(k + 1) * 96] == eng.msm(params.gs, row, l), (l, k)
    mont = stage(hooks, plan, 1, None, [s * MONT_R % M.R for s in rows[-2]], 1, L.FR_MONT, out_bytes=96)
    assert mont == got[(len(rows) - 2) * 96:(len(rows) - 1) * 96]


# ---- 3. honest cells verify, each tampering flips its own verdict -------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(10, 4), (8, 6), (6, 0), (4, 4)])
def test_honest_cells_verify_and_tampering_flips_its_own_verdict(eng, params, plans, verifiers, log_n, log_l):
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    C1 = opened(eng, params, plans, log_n, log_l, seed=1)[0]
    ver = verifiers(log_n, log_l)
    assert (ver.domain(), ver.coset_size(), ver.table_bytes()) == (N, l, 32 * l * 128 * 96)
    assert ver.verify([C0], [0] * K, list(range(K)), cells, proofs) == [True] * K
    # 65 cells: across the 64-thread block, shuffled, with duplicates
    rng = random.Random(log_n)
    order = [rng.randrange(K) for _ in range(65)]
    order[64] = order[0]
    idx, ids = [0] * 65, list(order)
    cs, ps = [list(cells[i]) for i in order], [proofs[i] for i in order]
    planted = {3: "value", 64: "commitment"}
    cs[3][rng.randrange(l)] = (cs[3][0] + 1) % M.R
    idx[64] = 1
    if K >= 4:  # (with fewer cosets the quotient does not depend on the coset: tests/test_verify_cosets_model.py)
        other = next(i for i in range(K) if i != order[17])
        ps[17] = proofs[other]
        ids[40] = next(i for i in range(K) if i != order[40])
        planted.update({17: "proof", 40: "id"})
    got = ver.verify([C0, C1], idx, ids, cs, ps)
    assert [k for k, v in enumerate(got) if not v] == sorted(planted), (got, planted)


# ---- 4. agreement with kzg_verify_eval_batched --------------------------------------------------------------------------------
def test_agrees_with_verify_eval_batched(eng, params, plans, verifiers):
    log_n, log_l = 8, 4
    K, l = 16, 16
    C0, cells, proofs, r = opened(eng, params, plans, log_n, log_l)
    plan, ver = plans(log_n, log_l), verifiers(log_n, log_l)
    kv = kzg_amd.KZGVerifier(params)
    cs, ps, ids = [list(c) for c in cells], list(proofs), list(range(K))
    cs[2][5] = (cs[2][5] + 7) % M.R
    ps[9] = proofs[10]
    ids[12] = 13
    got = kv.verify_cosets(ver, C0, ids, cs, ps)
    assert got == [k not in (2, 9, 12) for k in range(K)]
    for k in range(K):
        # the same claim through the one-coset verifier: the interpolant of the claimed values at the claimed coset's points
        xs = plan.coset_points(ids[k])
        coeffs = M.Polynomial.lagrange_interpolation(xs, cs[k]).slice_coeffs()
        wit = kzg_amd.KZGBatchWitness(kzg_amd.Polynomial.new_from_coeffs((coeffs + [0] * l)[:l], l - 1), ps[k])
        assert kv.verify_eval_batched(xs, C0, wit) == got[k], k


# ---- 5. several commitments in one call ---------------------------------------------------------------------------------------
def test_several_commitments_and_identity_proofs(eng, params, plans, verifiers):
    log_n, log_l = 6, 3
    K, l = 8, 8
    polys = [opened(eng, params, plans, log_n, log_l, seed=s) for s in (0, 1)] + [opened(eng, params, plans, log_n, log_l, n=5)]
    assert all(p == bytes(96) for p in polys[2][2])  # n <= l: FK20 emits the identity, r = p
    ver = verifiers(log_n, log_l)
    commitments = [p[0] for p in polys]
    idx = [k % 3 for k in range(3 * K)]
    ids = [k // 3 for k in range(3 * K)]
    cells = [polys[k % 3][1][k // 3] for k in range(3 * K)]
    proofs = [polys[k % 3][2][k // 3] for k in range(3 * K)]
    assert ver.verify(commitments, idx, ids, cells, proofs) == [True] * (3 * K)
    wrong = [(c + 1) % 3 for c in idx]
    assert ver.verify(commitments, wrong, ids, cells, proofs) == [False] * (3 * K)
    assert ver.verify(commitments[2:], [0], [K - 1], [polys[2][1][K - 1]], [polys[2][2][K - 1]]) == [True]


# ---- 6. formats, flags, chunks ------------------------------------------------------------------------------------------------
def test_formats_flags_and_chunks(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    K, l = 16, 4
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    cs = [list(c) for c in cells]
    cs[11][0] = (cs[11][0] + 1) % M.R
    want = bytes(k != 11 for k in range(K))
    ids, idx = list(range(K)), [0] * K
    P = [C.blob_to_point(b) for b in [C0] + proofs]
    enc = {L.G1_AFFINE_MONT: lambda p: M.g1_to_affine_mont(p), L.G1_ZCASH_UNCOMPRESSED: M.g1_to_uncompressed, L.G1_ZCASH_COMPRESSED: M.g1_to_compressed}
    canon, mont = flat(cs), pack_scalars([v * MONT_R % M.R for c in cs for v in c])
    for pfmt in AFFINE:
        pts = [bytes(enc[pfmt](p)) for p in P]
        assert raw_verify(eng, ver.handle, pts[:1], idx, ids, canon, pts[1:], pfmt=pfmt) == (0, want), pfmt
    assert raw_verify(eng, ver.handle, [C0], idx, ids, mont, proofs, sfmt=L.FR_MONT) == (0, want)
    for blob, sfmt in ((canon, L.FR_CANONICAL), (mont, L.FR_MONT)):
        buf = kzg_amd.DeviceBuffer(eng, K * l, sfmt).upload(blob)
        try:
            assert raw_verify(eng, ver.handle, [C0], idx, ids, buf.ptr, proofs, sfmt=sfmt, flags=L.IN_DEVICE) == (0, want)
            assert ver.verify([C0], idx, ids, buf, proofs) == [bool(b) for b in want]
        finally:
            buf.free()
    try:  # chunks of 5 cells: 16 = 5 + 5 + 5 + 1
        eng.set_option("verify_cosets_chunk", 5)
        assert raw_verify(eng, ver.handle, [C0], idx, ids, canon, proofs) == (0, want)
        eng.set_option("verify_cosets_chunk", 1)
        assert raw_verify(eng, ver.handle, [C0], idx, ids, canon, proofs) == (0, want)
    finally:
        eng.set_option("verify_cosets_chunk", 0)


# ---- 7. validation ------------------------------------------------------------------------------------------------------------
def test_validation(eng, hooks, params, plans, verifiers):
    log_n, log_l = 6, 2
    K = 16
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    ids, idx, blob = list(range(K)), [0] * K, flat(cells)
    untouched = b"\xa5" * K
    SHAPE = L.KZG_ERR_SHAPE
    assert raw_verify(eng, ver.handle, [C0], idx, ids[:-1] + [K], blob, proofs) == (SHAPE, untouched)
    assert raw_verify(eng, ver.handle, [C0], idx, ids[:-1] + [SIZE_MAX], blob, proofs) == (SHAPE, untouched)
    assert raw_verify(eng, ver.handle, [C0], idx[:-1] + [1], ids, blob, proofs) == (SHAPE, untouched)
    assert raw_verify(eng, ver.handle, [C0], idx, ids, blob, proofs, sfmt=2) == (SHAPE, untouched)
    assert raw_verify(eng, ver.handle, [C0], idx, ids, blob, proofs, pfmt=7) == (SHAPE, untouched)
    assert raw_verify(eng, ver.handle, [C0], idx, ids, blob, proofs, pfmt=L.G1_JACOBIAN_MONT) == (SHAPE, untouched)
    for hole in ("commitments", "idx", "ids", "cells", "proofs"):
        a = dict(commitments=[C0], idx=idx, ids=ids, cells=blob, proofs=proofs)
        a[hole] = None
        assert raw_verify(eng, ver.handle, a["commitments"], a["idx"], a["ids"], a["cells"], a["proofs"], count=K, n_commitments=1) == (SHAPE, untouched), hole
    assert eng.lib.kzg_verify_cosets(eng.ctx, ver.handle, C0, 1, (U32 * K)(*idx), (SZ * K)(*ids), blob, b"".join(proofs), K, 1, 0, 0, None) == SHAPE
    assert eng.lib.kzg_verify_cosets(eng.ctx, None, C0, 1, (U32 * K)(*idx), (SZ * K)(*ids), blob, b"".join(proofs), K, 1, 0, 0, None) == SHAPE
    assert raw_verify(eng, ver.handle, [C0], idx, ids, blob, proofs, count=0) == (0, b"")
    assert eng.lib.kzg_verify_cosets(eng.ctx, ver.handle, None, 0, None, None, None, None, 0, 1, 0, 0, None) == 0
    # an off-curve proof, an off-curve commitment: KZG_ERR_BAD_POINT for the call, as kzg_verify_eval; the outputs stay as they were
    off = bytearray(proofs[3])
    off[0] ^= 1
    assert raw_verify(eng, ver.handle, [C0], idx, ids, blob, proofs[:3] + [bytes(off)] + proofs[4:]) == (L.KZG_ERR_BAD_POINT, untouched)
    ok1 = ctypes.create_string_buffer(b"\xa5", 1)
    rc = eng.lib.kzg_verify_eval(eng.ctx, params.gs.handle, params.hs.handle, bytes(32), bytes(32), L.FR_CANONICAL, C0, bytes(off), 0, 1, ok1)
    assert rc == L.KZG_ERR_BAD_POINT and ok1.raw == b"\xa5"
    assert raw_verify(eng, ver.handle, [bytes(off)], idx, ids, blob, proofs) == (L.KZG_ERR_BAD_POINT, untouched)
    # setup
    h = VP()
    setup = eng.lib.kzg_cosets_verifier_setup
    short_g = kzg_amd.setup(eng, TAU, 8, g2_len=8)
    try:
        assert setup(eng.ctx, short_g.gs.handle, params.hs.handle, 6, 4, ctypes.byref(h)) == SHAPE   # len(gs) < l
        assert setup(eng.ctx, params.gs.handle, short_g.hs.handle, 6, 3, ctypes.byref(h)) == SHAPE   # len(hs) < l + 1
    finally:
        short_g.gs.free()
        short_g.hs.free()
    assert setup(eng.ctx, params.gs.handle, params.hs.handle, 3, 4, ctypes.byref(h)) == SHAPE        # log_l > log_n
    assert setup(eng.ctx, params.gs.handle, params.hs.handle, 23, 4, ctypes.byref(h)) == SHAPE       # log_n > 22
    assert setup(eng.ctx, params.gs.handle, params.hs.handle, 12, 9, ctypes.byref(h)) == SHAPE       # log_l above the limit
    assert eng.lib.kzg_cosets_verifier_shape(None, None, None, None) == SHAPE
    # an SRS (G1, G2) / a plan on another GPU (the hooks build can pretend)
    hooks.lib.kzg_test_srs_set_device.argtypes = [VP, I32]
    hooks.lib.kzg_srs_setup_g1.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    hooks.lib.kzg_srs_setup_g2.argtypes = [VP, VP, I32, SZ, ctypes.POINTER(VP)]
    hooks.lib.kzg_srs_free.argtypes = hooks.lib.kzg_srs_g2_free.argtypes = [VP, VP]
    hooks.lib.kzg_srs_free.restype = hooks.lib.kzg_srs_g2_free.restype = None
    hooks.lib.kzg_cosets_verifier_setup.argtypes = [VP, VP, VP, U32, U32, ctypes.POINTER(VP)]
    hooks.lib.kzg_cosets_verifier_free.argtypes = [VP, VP]
    hooks.lib.kzg_cosets_verifier_free.restype = None
    gs, hs = VP(), VP()
    tau = TAU.to_bytes(32, "little")
    assert hooks.lib.kzg_srs_setup_g1(hooks.ctx, tau, 1, 4, ctypes.byref(gs)) == 0 and hooks.lib.kzg_srs_setup_g2(hooks.ctx, tau, 1, 5, ctypes.byref(hs)) == 0
    try:
        assert hooks.lib.kzg_test_srs_set_device(gs, 5) == 0
        assert hooks.lib.kzg_cosets_verifier_setup(hooks.ctx, gs, hs, 4, 2, ctypes.byref(h)) == SHAPE
        assert hooks.lib.kzg_test_srs_set_device(gs, 0) == 0
        hooks.lib.kzg_test_srs_g2_set_device.argtypes = hooks.lib.kzg_test_cosets_verifier_set_device.argtypes = [VP, I32]
        assert hooks.lib.kzg_test_srs_g2_set_device(hs, 5) == 0
        assert hooks.lib.kzg_cosets_verifier_setup(hooks.ctx, gs, hs, 4, 2, ctypes.byref(h)) == SHAPE
        assert hooks.lib.kzg_test_srs_g2_set_device(hs, 0) == 0
        # the same cells through a plan of the hooks build: verdicts first, then the plan re-homed
        hp = VP()
        big_g, big_h = VP(), VP()
        assert hooks.lib.kzg_srs_setup_g1(hooks.ctx, tau, 1, 64, ctypes.byref(big_g)) == 0
        assert hooks.lib.kzg_srs_setup_g2(hooks.ctx, tau, 1, 5, ctypes.byref(big_h)) == 0
        try:
            assert hooks.lib.kzg_cosets_verifier_setup(hooks.ctx, big_g, big_h, log_n, log_l, ctypes.byref(hp)) == 0, hooks.last_error()
            hooks.lib.kzg_verify_cosets.argtypes = eng.lib.kzg_verify_cosets.argtypes
            hooks.lib.kzg_verify_cosets.restype = I32
            assert raw_verify(hooks, hp, [C0], idx, ids, blob, proofs) == (0, b"\x01" * K)
            assert hooks.lib.kzg_test_cosets_verifier_set_device(hp, 5) == 0
            assert raw_verify(hooks, hp, [C0], idx, ids, blob, proofs) == (SHAPE, untouched)
            assert raw_verify(hooks, hp, [C0], idx, ids, blob, proofs, count=0) == (SHAPE, b"")
            assert hooks.lib.kzg_test_cosets_verifier_set_device(hp, 0) == 0
            assert raw_verify(hooks, hp, [C0], idx, ids, blob, proofs) == (0, b"\x01" * K)
        finally:
            if hp:
                hooks.lib.kzg_cosets_verifier_free(hooks.ctx, hp)
            hooks.lib.kzg_srs_free(hooks.ctx, big_g)
            hooks.lib.kzg_srs_g2_free(hooks.ctx, big_h)
    finally:
        hooks.lib.kzg_srs_free(hooks.ctx, gs)
        hooks.lib.kzg_srs_g2_free(hooks.ctx, hs)


def test_one_plan_two_threads_two_contexts(eng, params, plans, verifiers):
    log_n, log_l = 6, 2
    K = 16
    C0, cells, proofs, _r = opened(eng, params, plans, log_n, log_l)
    ver = verifiers(log_n, log_l)
    cs = [list(c) for c in cells]
    cs[4][1] = (cs[4][1] + 1) % M.R
    blob, ids, idx = flat(cs), list(range(K)), [0] * K
    other = kzg_amd.Engine(0)
    out = {}

    def work(name, e):
        out[name] = [raw_verify(e, ver.handle, [C0], idx, ids, blob, proofs) for _ in range(3)]
    try:
        th = [threading.Thread(target=work, args=(n, e)) for n, e in (("a", eng), ("b", other), ("c", eng))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        other.close()
    want = (0, bytes(k != 4 for k in range(K)))
    assert all(r == want for rs in out.values() for r in rs) and len(out) == 3


# ---- 8. the Python surface ----------------------------------------------------------------------------------------------------
def test_python_surface(eng, params, plans, verifiers):
    rng = random.Random(5)
    plan, ver = plans(4, 2), verifiers(4, 2)
    poly = kzg_amd.Polynomial(rand_scalars(rng, 13), 12)
    prover, kv = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    commitment = prover.commit(poly)
    wits = prover.create_witness_all_cosets(poly, plan)
    cells = [[M.Polynomial(w.polynomial().slice_coeffs(), 3).eval(x) for x in plan.coset_points(i)] for i, w in enumerate(wits)]
    proofs = [w.elem() for w in wits]
    assert kv.verify_cosets(ver, commitment, range(4), cells, proofs) == [True] * 4
    assert ver.verify([commitment], [0, 0], [2, 1], [cells[2], cells[1]], [proofs[2], proofs[1]]) == [True, True]
    assert ver.verify([commitment], [0, 0], [2, 1], [cells[1], cells[1]], [proofs[2], proofs[1]]) == [False, True]
    assert ver.verify([commitment], [], [], [], []) == []
    with pytest.raises(kzg_amd.ReferencePanic):
        ver.verify([commitment], [0], [4], [cells[0]], [proofs[0]])
    with pytest.raises(kzg_amd.ReferencePanic):
        ver.verify([commitment], [0], [0], cells[0][:3], [proofs[0]])
