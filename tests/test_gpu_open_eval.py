"""kzg_eval_form_eval / kzg_quotient_eval_at / kzg_open_eval (kzg_amd/csrc/open_eval.hip, capi.hip): an evaluation-form polynomial
opened at any point of Fr, in batches.  Every case compares bytes with an independent route on the same GPU (inverse transform,
kzg_poly_eval, kzg_quotient_linear, transform back; kzg_witness_coeff; kzg_witness_eval) and, at d <= 64, with the big-int model
(tests/open_eval_model.py).  Like the FK20 files this one sorts after the tests that release the session's contexts, so it opens
and closes its own module-scoped Engine."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars, unpack_scalars
from oracle import kzg_model as M
from tests import open_eval_model as OM
from tests.fk20_common import FORMATS, MONT_R, dev_buffer, dev_download, same_point, split
from tests.fk20_common import eng, hooks  # noqa: F401 -- this module's fixtures

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
TAU = 0x0123456789ABCDEF0FEDCBA987654321
A5 = b"\xa5"


def le(v):
    return (v % R).to_bytes(32, "little")


def log2(d):
    return d.bit_length() - 1


def omega(d):
    return M.compute_omega(d)[2]


def points_for(d, rng):
    w = omega(d)
    return [rng.randrange(R), 0, 1, w, R - 1, pow(w, d - 1, R), omega(2 * d), 7]


def vectors_for(eng, d, rng):
    top = [rng.randrange(R) for _ in range(d - 1)] + [1]                 # degree exactly d - 1
    top = eng.ntt(top, log2(d)) if d > 1 else top
    return [[rng.randrange(R) for _ in range(d)], [0] * d, [5] * d, [R - 1] * d, top]


def fr_eval(eng, blob, d, zs, sfmt=CAN, flags=0):
    out = ctypes.create_string_buffer(32 * len(zs))
    zb = b"".join(zs) if isinstance(zs[0], bytes) else b"".join(le(z) for z in zs)
    rc = eng.lib.kzg_eval_form_eval(eng.ctx, blob, d, len(zs), zb, sfmt, flags, out)
    assert rc == 0, eng.last_error()
    return out.raw


def fr_quot(eng, blob, d, z, sfmt=CAN):
    y, q = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * d)
    rc = eng.lib.kzg_quotient_eval_at(eng.ctx, blob, d, z if isinstance(z, bytes) else le(z), sfmt, 0, y, q)
    assert rc == 0, eng.last_error()
    return y.raw, q.raw


def other_route(eng, evals, z):
    """(y, q) through the coefficient form: iNTT, kzg_poly_eval, kzg_quotient_linear, NTT"""
    d = len(evals)
    if d == 1:
        return eng.poly_eval(evals, z), [0]
    coeffs = eng.ntt(evals, log2(d), inverse=True)
    y = eng.poly_eval(coeffs, z)
    q = eng.quotient_linear(coeffs, z, y)
    return y, eng.ntt(q + [0], log2(d))


def check_fr(eng, evals, z, model):
    d = len(evals)
    blob = pack_scalars(evals)
    y, q = fr_quot(eng, blob, d, z)
    assert fr_eval(eng, blob, d, [z]) == y
    wy, wq = other_route(eng, evals, z)
    assert y == le(wy) and q == pack_scalars(wq), (d, z)
    if model:
        my, mq = OM.quotient_at(evals, z)
        assert y == le(my) and q == pack_scalars(mq), (d, z)


# ---- 1. the Fr stage alone -----------------------------------------------------------------------------------------------------
# 256: one block; 512: two blocks and a second-stage sum; 2^13: many blocks and several tiles of the batch inversion
@pytest.mark.parametrize("d", [1, 2, 4, 64, 256, 512, 1 << 13])
def test_fr_stage(eng, d):
    rng = random.Random(100 + d)
    pts, vecs = points_for(d, rng), vectors_for(eng, d, rng)
    if d <= 512:
        cases = [(v, z) for v in vecs for z in pts]
    else:  # every point on the random vector, every vector at the random point
        cases = [(vecs[0], z) for z in pts] + [(v, pts[0]) for v in vecs[1:]]
    for v, z in cases:
        check_fr(eng, v, z, model=d <= 64)
    # a constant polynomial: q = 0 at every point
    assert fr_quot(eng, pack_scalars(vecs[2]), d, pts[0])[1] == bytes(32 * d)


def test_fr_stage_2_16(eng):
    rng = random.Random(16)
    d = 1 << 16
    check_fr(eng, [rng.randrange(R) for _ in range(d)], rng.randrange(R), model=False)


def test_fr_montgomery_scalars(eng):
    rng = random.Random(5)
    d = 512
    evals = [rng.randrange(R) for _ in range(d)]
    mont = pack_scalars([v * MONT_R % R for v in evals])
    for z in (rng.randrange(R), omega(d), 0):
        y, q = fr_quot(eng, pack_scalars(evals), d, z)
        ym, qm = fr_quot(eng, mont, d, le(z * MONT_R), MONT)
        assert ym == le(int.from_bytes(y, "little") * MONT_R) and qm == pack_scalars([v * MONT_R % R for v in unpack_scalars(q)])
        assert fr_eval(eng, mont, d, [le(z * MONT_R)], MONT) == ym


# ---- 2. the full call ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def srs(eng):
    """srs(d) -> (KZGParams of setup(TAU, d), setup_lagrange(TAU, d)), built once per size"""
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = (kzg_amd.setup(eng, TAU, d, g2_len=2), kzg_amd.setup_lagrange(eng, TAU, d))
        return cache[d]
    yield get
    for p, lag in cache.values():
        p.gs.free()
        p.hs.free()
        lag.free()


def open_eval(eng, lag, blob, d, zs, sfmt=CAN, flags=0, ofmt=L.G1_AFFINE_MONT, want_y=True, want_w=True, out_w=None):
    """(rc, y bytes or None, witness bytes or None)"""
    batch = len(zs)
    psz = L.POINT_BYTES[ofmt]
    ys = ctypes.create_string_buffer(A5 * (32 * batch), 32 * batch) if want_y else None
    ws = out_w if out_w is not None else (ctypes.create_string_buffer(A5 * (psz * batch), psz * batch) if want_w else None)
    zb = b"".join(z if isinstance(z, bytes) else le(z) for z in zs)
    rc = eng.lib.kzg_open_eval(eng.ctx, lag.handle, blob, d, batch, zb, sfmt, flags, ys, ws, ofmt)
    return rc, (ys.raw if want_y else None), (ws.raw if want_w and out_w is None else None)


def witness_eval(eng, lag, blob, d, m, ofmt=L.G1_AFFINE_MONT):
    out = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
    assert eng.lib.kzg_witness_eval(eng.ctx, lag.handle, blob, d, m, CAN, 0, out, ofmt) == 0, eng.last_error()
    return out.raw


def test_on_domain_is_witness_eval(eng, srs):
    rng = random.Random(21)
    d = 1 << 10
    _, lag = srs(d)
    evals = [rng.randrange(R) for _ in range(d)]
    blob = pack_scalars(evals)
    for m in (0, 1, d // 2, d - 1):
        rc, y, w = open_eval(eng, lag, blob, d, [pow(omega(d), m, R)])
        assert rc == 0, eng.last_error()
        assert y == le(evals[m]) and w == witness_eval(eng, lag, blob, d, m), m


@pytest.mark.parametrize("d", [1 << 10, 1 << 13])
def test_off_domain_is_witness_coeff_and_verifies(eng, srs, d):
    rng = random.Random(22 + d)
    params, lag = srs(d)
    evals = [rng.randrange(R) for _ in range(d)]
    blob = pack_scalars(evals)
    coeffs = pack_scalars(eng.ntt(evals, log2(d), inverse=True))
    commitment = ctypes.create_string_buffer(96)
    assert eng.lib.kzg_commit_eval(eng.ctx, lag.handle, blob, d, CAN, 0, commitment, L.G1_AFFINE_MONT) == 0
    for z in (rng.randrange(R), 0, omega(2 * d), 7):
        ys = set()
        for ofmt in FORMATS:
            rc, y, w = open_eval(eng, lag, blob, d, [z], ofmt=ofmt)
            assert rc == 0, eng.last_error()
            ys.add(y)
            want = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
            assert eng.lib.kzg_witness_coeff(eng.ctx, params.gs.handle, coeffs, d, le(z), y, CAN, 0, want, ofmt) == 0, eng.last_error()
            assert same_point(w, want.raw, ofmt), (d, z, ofmt)
            if ofmt == L.G1_AFFINE_MONT:
                proof = w
        assert len(ys) == 1
        y = ys.pop()
        bad = le(int.from_bytes(y, "little") + 1)
        ok = ctypes.create_string_buffer(2)
        rc = eng.lib.kzg_verify_eval(eng.ctx, params.gs.handle, params.hs.handle, le(z) * 2, y + bad, CAN, commitment.raw * 2, proof * 2,
                                     L.G1_AFFINE_MONT, 2, ok)
        assert rc == 0 and ok.raw == b"\x01\x00", (d, z, ok.raw)


def test_degenerate_sizes(eng):
    rng = random.Random(23)
    for d in (1, 2):
        lag = kzg_amd.setup_lagrange(eng, TAU, d)
        evals = [rng.randrange(R) for _ in range(d)]
        for z in (rng.randrange(R), 1, R - 1, 0):
            rc, y, w = open_eval(eng, lag, pack_scalars(evals), d, [z])
            assert rc == 0, eng.last_error()
            assert y == le(OM.eval_at(evals, z))
            if d == 1:
                assert y == le(evals[0]) and w == bytes(96)          # the witness is the identity
        rc, y, w = open_eval(eng, lag, pack_scalars([9] * d), d, [12345])
        assert rc == 0 and y == le(9) and w == bytes(96)               # a constant polynomial
        lag.free()


# ---- 3. batches ------------------------------------------------------------------------------------------------------------------
def singles(eng, lag, vecs, d, zs):
    ys, ws = b"", b""
    for v, z in zip(vecs, zs):
        rc, y, w = open_eval(eng, lag, pack_scalars(v), d, [z])
        assert rc == 0, eng.last_error()
        ys, ws = ys + y, ws + w
    return ys, ws


@pytest.fixture(scope="module")
def batch35(eng, srs):
    """35 vectors at 2^10 with on- and off-domain points mixed, and their single-call results: computed once"""
    rng = random.Random(31)
    d = 1 << 10
    _, lag = srs(d)
    vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(35)]
    w = omega(d)
    mixed = [pow(w, rng.randrange(d), R) if b % 3 == 1 else rng.randrange(R) for b in range(35)]
    mixed[4] = mixed[0]                                                   # two polynomials of one chunk share an off-domain point
    return d, lag, vecs, mixed, singles(eng, lag, vecs, d, mixed)


def test_batch_shared_distinct_and_mixed_points(eng, batch35):
    d, lag, vecs, mixed, (ys1, ws1) = batch35
    rng = random.Random(32)
    blob = b"".join(pack_scalars(v) for v in vecs)
    rc, ys, ws = open_eval(eng, lag, blob, d, mixed)
    assert rc == 0, eng.last_error()
    assert ys == ys1 and ws == ws1
    n = 6
    shared = [rng.randrange(R)] * n
    distinct = [rng.randrange(R) for _ in range(n)]
    for zs in (shared, distinct):
        rc, ys, ws = open_eval(eng, lag, blob[:n * d * 32], d, zs)
        assert rc == 0, eng.last_error()
        assert (ys, ws) == singles(eng, lag, vecs[:n], d, zs)
        assert fr_eval(eng, blob[:n * d * 32], d, zs) == ys


def test_batch_spans_chunks_with_a_ragged_last_one(eng, batch35):
    d, lag, vecs, mixed, (ys1, ws1) = batch35
    blob = b"".join(pack_scalars(v) for v in vecs)
    eng.set_option("streams", 4)
    try:
        rc, ys, ws = open_eval(eng, lag, blob, d, mixed)
        assert rc == 0, eng.last_error()
        assert ys == ys1 and ws == ws1
        assert fr_eval(eng, blob, d, mixed) == ys1                       # 35 polynomials: three chunks of the Fr-only call
    finally:
        eng.set_option("streams", 13)


def test_batch_device_buffers_null_outputs_and_montgomery(eng, batch35):
    d, lag, vecs, mixed, (ys1, ws1) = batch35
    n = 7
    blob = b"".join(pack_scalars(v) for v in vecs[:n])
    zs = mixed[:n]
    d_in = dev_buffer(eng, len(blob))
    assert eng.lib.kzg_dev_upload(eng.ctx, d_in, blob, len(blob)) == 0
    d_out = dev_buffer(eng, 96 * n + 96)
    try:
        for in_dev in (0, L.IN_DEVICE):
            src = d_in if in_dev else blob
            for out_dev in (0, L.OUT_DEVICE):
                if out_dev:
                    rc, ys, _ = open_eval(eng, lag, src, d, zs, flags=in_dev | out_dev, out_w=d_out)
                    back = dev_download(eng, d_out, 96 * n + 96)
                    ws, tail = back[:96 * n], back[96 * n:]
                    assert tail == A5 * 96                                # nothing behind the last witness is written
                else:
                    rc, ys, ws = open_eval(eng, lag, src, d, zs, flags=in_dev)
                assert rc == 0, eng.last_error()
                assert ys == ys1[:32 * n] and ws == ws1[:96 * n], (in_dev, out_dev)
            rc, ys, ws = open_eval(eng, lag, src, d, zs, flags=in_dev, want_w=False)
            assert rc == 0 and ys == ys1[:32 * n] and ws is None
            rc, ys, ws = open_eval(eng, lag, src, d, zs, flags=in_dev, want_y=False)
            assert rc == 0 and ys is None and ws == ws1[:96 * n]
            assert fr_eval(eng, src, d, zs, flags=in_dev) == ys1[:32 * n]
        mont = b"".join(pack_scalars([v * MONT_R % R for v in vec]) for vec in vecs[:n])
        rc, ys, ws = open_eval(eng, lag, mont, d, [le(z * MONT_R) for z in zs], sfmt=MONT)
        assert rc == 0, eng.last_error()
        assert ys == pack_scalars([v * MONT_R % R for v in unpack_scalars(ys1[:32 * n])]) and ws == ws1[:96 * n]
    finally:
        eng.lib.kzg_dev_free(eng.ctx, d_in)
        eng.lib.kzg_dev_free(eng.ctx, d_out)


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(eng, hooks, srs):
    d = 1 << 10
    _, lag = srs(d)
    blob = pack_scalars(list(range(d)))
    z = le(7)
    lib, ctx, h = eng.lib, eng.ctx, lag.handle
    ys, ws, q = (ctypes.create_string_buffer(A5 * 32, 32), ctypes.create_string_buffer(A5 * 144, 144),
                 ctypes.create_string_buffer(A5 * (32 * d), 32 * d))
    SH = L.KZG_ERR_SHAPE
    aff = L.G1_AFFINE_MONT
    bad = [
        lib.kzg_open_eval(ctx, h, blob, 768, 1, z, CAN, 0, ys, ws, aff),             # d not a power of two
        lib.kzg_open_eval(ctx, h, blob, d // 2, 1, z, CAN, 0, ys, ws, aff),          # d != len(lagrange)
        lib.kzg_open_eval(ctx, h, blob, 0, 1, z, CAN, 0, ys, ws, aff),               # d == 0
        lib.kzg_open_eval(ctx, h, blob, d, 1, z, 2, 0, ys, ws, aff),                 # unknown scalar format
        lib.kzg_open_eval(ctx, h, blob, d, 1, z, CAN, 0, ys, ws, 4),                 # unknown point format
        lib.kzg_open_eval(ctx, None, blob, d, 1, z, CAN, 0, ys, ws, aff),            # NULL inputs
        lib.kzg_open_eval(ctx, h, None, d, 1, z, CAN, 0, ys, ws, aff),
        lib.kzg_open_eval(ctx, h, blob, d, 1, None, CAN, 0, ys, ws, aff),
        lib.kzg_open_eval(ctx, h, blob, d, 1, z, CAN, 0, None, None, aff),           # both outputs NULL
        lib.kzg_open_eval(None, h, blob, d, 1, z, CAN, 0, ys, ws, aff),
        lib.kzg_open_eval(ctx, h, blob, d, 1, R.to_bytes(32, "little"), CAN, 0, ys, ws, aff),   # z >= r
        lib.kzg_eval_form_eval(ctx, blob, 768, 1, z, CAN, 0, ys),
        lib.kzg_eval_form_eval(ctx, blob, 0, 1, z, CAN, 0, ys),
        lib.kzg_eval_form_eval(ctx, blob, d, 1, z, 2, 0, ys),
        lib.kzg_eval_form_eval(ctx, None, d, 1, z, CAN, 0, ys),
        lib.kzg_eval_form_eval(ctx, blob, d, 1, None, CAN, 0, ys),
        lib.kzg_eval_form_eval(ctx, blob, d, 1, z, CAN, 0, None),
        lib.kzg_eval_form_eval(ctx, blob, d, 1, R.to_bytes(32, "little"), CAN, 0, ys),
        lib.kzg_quotient_eval_at(ctx, blob, 768, z, CAN, 0, ys, q),
        lib.kzg_quotient_eval_at(ctx, blob, 0, z, CAN, 0, ys, q),
        lib.kzg_quotient_eval_at(ctx, blob, d, z, 2, 0, ys, q),
        lib.kzg_quotient_eval_at(ctx, None, d, z, CAN, 0, ys, q),
        lib.kzg_quotient_eval_at(ctx, blob, d, None, CAN, 0, ys, q),
        lib.kzg_quotient_eval_at(ctx, blob, d, z, CAN, 0, ys, None),
        lib.kzg_quotient_eval_at(ctx, blob, d, R.to_bytes(32, "little"), CAN, 0, ys, q),
    ]
    assert bad == [SH] * len(bad), bad
    hooks.lib.kzg_test_srs_set_device.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hooks.lib.kzg_test_srs_set_device.restype = ctypes.c_int
    assert hooks.lib.kzg_test_srs_set_device(h, 1) == 0                              # an SRS on another GPU
    try:
        assert lib.kzg_open_eval(ctx, h, blob, d, 1, z, CAN, 0, ys, ws, aff) == SH
        assert "another GPU" in eng.last_error()
    finally:
        hooks.lib.kzg_test_srs_set_device(h, 0)
    assert ys.raw == A5 * 32 and ws.raw == A5 * 144 and q.raw == A5 * (32 * d)
    # batch == 0
    assert lib.kzg_open_eval(ctx, h, blob, d, 0, z, CAN, 0, ys, ws, aff) == 0
    assert lib.kzg_eval_form_eval(ctx, blob, d, 0, z, CAN, 0, ys) == 0
    assert ys.raw == A5 * 32 and ws.raw == A5 * 144
    # and the context is fine afterwards
    assert lib.kzg_open_eval(ctx, h, blob, d, 1, z, CAN, 0, ys, ws, aff) == 0 and ys.raw == le(OM.eval_at(list(range(d)), 7))


# ---- 5. two threads on one context -----------------------------------------------------------------------------------------------
def test_two_threads_alternate_open_eval_and_witness_eval():
    # a context of its own: the evaluation-domain tables (eval_tabs) are built by whichever thread comes first
    rng = random.Random(51)
    d = 1 << 10
    e = kzg_amd.Engine(0)
    lag = kzg_amd.setup_lagrange(e, TAU, d)
    try:
        vecs = [[rng.randrange(R) for _ in range(d)] for _ in range(2)]
        blobs = [pack_scalars(v) for v in vecs]
        w = omega(d)
        jobs = [[(rng.randrange(R), None) if k % 2 == 0 else (None, rng.randrange(d)) for k in range(6)],
                [(None, rng.randrange(d)) if k % 2 == 0 else (pow(w, rng.randrange(d), R), None) for k in range(6)]]

        def run(t, out):
            for z, m in jobs[t]:
                if z is not None:
                    rc, y, wit = open_eval(e, lag, blobs[t], d, [z])
                    out.append((rc, y, wit))
                else:
                    out.append((0, None, witness_eval(e, lag, blobs[t], d, m)))
        got = [[], []]
        threads = [threading.Thread(target=run, args=(t, got[t])) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        serial = [[], []]
        for t in range(2):
            run(t, serial[t])
        assert got == serial and all(rc == 0 for t in got for rc, _, _ in t)
    finally:
        lag.free()
        e.close()


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(eng, srs):
    rng = random.Random(61)
    d = 1 << 10
    params, lag = srs(d)
    prover = kzg_amd.KZGProverEvalForm(params, lag)
    doms = [kzg_amd.EvaluationDomain.from_coeffs([rng.randrange(R) for _ in range(d)]) for _ in range(3)]
    zs = [rng.randrange(R), pow(prover.omega(), 5, R), 0]
    ys, ws = prover.open_at_batch(doms, zs)
    for dom, z, y, w in zip(doms, zs, ys, ws):
        assert (y, w) == prover.open_at(dom, z)
        assert y == M.Polynomial(eng.ntt(dom.coeffs, log2(d), inverse=True), d - 1).eval(z)
    assert ws[1] == prover.create_witness(doms[1], 5)
    verifier = kzg_amd.KZGVerifier(params)
    assert verifier.verify_eval((zs[0], ys[0]), prover.commit(doms[0]), ws[0])
    blob = b"".join(pack_scalars(dom.coeffs) for dom in doms)
    assert prover.open_at_batch(blob, zs) == (ys, ws)
    buf = eng.alloc_scalars(3 * d).upload(blob)
    try:
        assert prover.open_at_batch(buf, zs) == (ys, ws)
        assert eng.eval_form_eval(buf, zs, d) == ys == eng.eval_form_eval(doms, zs)
    finally:
        buf.free()
