"""FK20 (kzg_fk20_setup / kzg_witness_all_coeff / kzg_witness_all_eval, kzg_amd/csrc/g1ntt.hip) and its building blocks on the
GPU.  This file sorts after the tests that release the session's contexts (tests/conftest.py ORDER), so it opens and closes its own
module-scoped Engine and HooksEngine instead of the session fixtures."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import _raise, pack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import fk20_model as F
from tests.gpu_common import HooksEngine, rand_scalars

pytestmark = pytest.mark.gpu

TAU = 0x5EED_F20
SRS_LEN = 1 << 12
VP, SZ, I32, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
FORMATS = [L.G1_AFFINE_MONT, L.G1_JACOBIAN_MONT, L.G1_ZCASH_UNCOMPRESSED, L.G1_ZCASH_COMPRESSED]


@pytest.fixture(scope="module")
def eng():
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks():
    h = HooksEngine(0)
    h.lib.kzg_test_g1_mul_glv.argtypes = [VP, VP, VP, SZ, VP]
    h.lib.kzg_test_g1_mul_glv.restype = I32
    h.lib.kzg_test_g1_ntt.argtypes = [VP, VP, U32, I32, VP]
    h.lib.kzg_test_g1_ntt.restype = I32
    yield h
    h.close()


@pytest.fixture(scope="module")
def params(eng):
    p = kzg_amd.setup(eng, TAU, SRS_LEN, g2_len=2)
    yield p
    p.gs.free()
    if p.hs is not None:
        p.hs.free()


@pytest.fixture(scope="module")
def plans(eng, params):
    cache = {}

    def get(log_n):
        if log_n not in cache:
            cache[log_n] = kzg_amd.FK20Plan(eng, params.gs, log_n)
        return cache[log_n]
    yield get
    for p in cache.values():
        p.free()


def G():
    return C.g1_generator()


def same_point(a, b, fmt):
    """byte equality; the Jacobian form is not canonical, so there the projective coordinates are compared"""
    if fmt != L.G1_JACOBIAN_MONT:
        return a == b
    q = M.Q
    X1, Y1, Z1 = (int.from_bytes(a[i:i + 48], "little") for i in (0, 48, 96))
    X2, Y2, Z2 = (int.from_bytes(b[i:i + 48], "little") for i in (0, 48, 96))
    if Z1 % q == 0 or Z2 % q == 0:
        return Z1 % q == 0 and Z2 % q == 0
    return (X1 * Z2 * Z2 - X2 * Z1 * Z1) % q == 0 and (Y1 * Z2 ** 3 - Y2 * Z1 ** 3) % q == 0


def all_coeff(eng, plan, blob, n, batch, ofmt=L.G1_AFFINE_MONT, sfmt=L.FR_CANONICAL, flags=0, out=None):
    N = plan.domain()
    psz = L.POINT_BYTES[ofmt]
    buf = out if out is not None else ctypes.create_string_buffer(psz * N * batch)
    rc = eng.lib.kzg_witness_all_coeff(eng.ctx, plan.handle, blob, n, batch, sfmt, flags, buf, ofmt)
    if rc:
        _raise(eng, rc)
    return buf


def split(raw, psz, count):
    return [raw[i * psz:(i + 1) * psz] for i in range(count)]


def evals_at_domain(coeffs, N):
    return C.fft(list(coeffs) + [0] * (N - len(coeffs)))


# ---- 1. GLV multiplication --------------------------------------------------------------------------------------------------
def test_glv_mul_hook(hooks):
    rng = random.Random(11)
    lam = F.GLV_LAMBDA
    scalars = [0, 1, lam - 1, lam, lam + 1, M.R - 1, 2, M.R - 2] + [rng.randrange(M.R) for _ in range(56)]
    pts = [bytes(96), G()] + [C.g1_mul(G(), rng.randrange(1, M.R)) for _ in range(6)]
    P, K = [], []
    for p in pts:
        for k in scalars:
            P.append(p)
            K.append(k)
    out = ctypes.create_string_buffer(96 * len(P))
    rc = hooks.lib.kzg_test_g1_mul_glv(hooks.ctx, b"".join(P), pack_scalars(K), len(P), out)
    assert rc == 0, hooks.last_error()
    for i, (p, k) in enumerate(zip(P, K)):
        assert out.raw[96 * i:96 * i + 96] == C.g1_mul(p, k), (i, k)


# ---- 2. G1 DFT ----------------------------------------------------------------------------------------------------------------
@pytest.mark.limit(300)
@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 8, 10])
def test_g1_ntt_hook(hooks, log_n):
    rng = random.Random(100 + log_n)
    d = 1 << log_n
    a = [rng.randrange(M.R) for _ in range(d)]
    a[rng.randrange(d)] = 0  # one identity in the input
    pts = b"".join(C.g1_mul(G(), x) for x in a)
    for inverse in (0, 1):
        out = ctypes.create_string_buffer(96 * d)
        rc = hooks.lib.kzg_test_g1_ntt(hooks.ctx, pts, log_n, inverse, out)
        assert rc == 0, hooks.last_error()
        want = C.fft(a, inverse=bool(inverse))
        if inverse:
            want = [x * d % M.R for x in want]  # the hook's inverse is not scaled
        for m in range(d):
            assert out.raw[96 * m:96 * m + 96] == C.g1_mul(G(), want[m]), (log_n, inverse, m)


# ---- 3. coefficient form ------------------------------------------------------------------------------------------------------
def check_coeff(eng, params, plan, coeffs, ofmts):
    N = plan.domain()
    n = len(coeffs)
    prover = kzg_amd.KZGProver(params)
    w = M.compute_omega(N)[2]
    xs = [pow(w, m, M.R) for m in range(N)]
    ys = evals_at_domain(coeffs, N)
    for ofmt in ofmts:
        psz = L.POINT_BYTES[ofmt]
        got = split(all_coeff(eng, plan, pack_scalars(coeffs), n, 1, ofmt).raw, psz, N)
        want, ok = prover.create_witness_many(kzg_amd.Polynomial(coeffs, n - 1), list(zip(xs, ys)), ofmt)
        assert all(ok)
        for m in range(N):
            assert same_point(got[m], want[m], ofmt), (N, n, ofmt, m)
    return xs, ys


@pytest.mark.limit(600)
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 6, 8, 10])
def test_coeff_form_matches_many(eng, params, plans, log_n):
    rng = random.Random(300 + log_n)
    N = 1 << log_n
    plan = plans(log_n)
    assert plan.domain() == N
    for kind in ("full", "u64"):
        for n in sorted({N, max(1, N // 2 + 1), 1}):
            coeffs = rand_scalars(rng, n, kind)
            ofmts = FORMATS if (kind == "full" and n == N) else [L.G1_AFFINE_MONT]
            xs, ys = check_coeff(eng, params, plan, coeffs, ofmts)
            if N <= 16 and kind == "full":
                gs = M.setup_g1_fast(TAU, max(n, 1))
                mp = M.KZGProver(M.KZGParams(gs))
                got = split(all_coeff(eng, plan, pack_scalars(coeffs), n, 1).raw, 96, N)
                for m in range(N):
                    W = mp.create_witness(M.Polynomial(coeffs, n - 1), (xs[m], ys[m]))
                    assert got[m] == M.g1_to_affine_mont(W), (N, n, m)


def test_python_surface(eng, params, plans):
    rng = random.Random(17)
    plan = plans(4)
    coeffs = rand_scalars(rng, 13)
    poly = kzg_amd.Polynomial(coeffs, 12)
    prover = kzg_amd.KZGProver(params)
    single = prover.create_witness_all_points(poly, plan)
    assert len(single) == 16
    both = prover.create_witness_all_points_batch([poly, kzg_amd.Polynomial(coeffs[:5], 4)], plan)
    assert both[0] == single
    assert both[1] == split(all_coeff(eng, plan, pack_scalars(coeffs[:5] + [0] * 8), 13, 1).raw, 96, 16)


# ---- 4. evaluation form -------------------------------------------------------------------------------------------------------
@pytest.mark.limit(600)
@pytest.mark.parametrize("log_n", [0, 1, 3, 6, 10])
def test_eval_form_matches_many(eng, params, plans, log_n):
    rng = random.Random(400 + log_n)
    N = 1 << log_n
    plan = plans(log_n)
    lag = kzg_amd.setup_lagrange(eng, TAU, N)
    try:
        mono = kzg_amd.KZGParams(kzg_amd.setup(eng, TAU, N, g2_len=0).gs)
        prover = kzg_amd.KZGProverEvalForm(mono, lag)
        for kind in ("full", "u64"):
            ev = kzg_amd.EvaluationDomain(rand_scalars(rng, N, kind), N, log_n, M.compute_omega(N)[2])
            got = prover.create_witness_all_points(ev, plan)
            want = prover.create_witness_many(ev, list(range(N)))
            assert got == want, (N, kind)
        mono.gs.free()
    finally:
        lag.free()


# ---- 5. batch and device buffers ----------------------------------------------------------------------------------------------
@pytest.mark.limit(600)
def test_batch_equals_single_calls_and_device_flags(eng, plans):
    rng = random.Random(5)
    plan = plans(12)
    N, B = 1 << 12, 64
    n = N - 3
    polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
    blob = b"".join(pack_scalars(p) for p in polys)
    batched = all_coeff(eng, plan, blob, n, B).raw
    for b in range(B):
        one = all_coeff(eng, plan, pack_scalars(polys[b]), n, 1).raw
        assert one == batched[b * N * 96:(b + 1) * N * 96], b
    din = eng.alloc_scalars(n * B)
    din.upload(blob)
    dout = ctypes.c_void_p()
    assert eng.lib.kzg_dev_alloc(eng.ctx, N * B * 96, ctypes.byref(dout)) == 0
    try:
        host_out = all_coeff(eng, plan, din.ptr, n, B, flags=L.IN_DEVICE).raw
        assert host_out == batched
        all_coeff(eng, plan, blob, n, B, flags=L.OUT_DEVICE, out=dout)
        back = ctypes.create_string_buffer(N * B * 96)
        assert eng.lib.kzg_dev_download(eng.ctx, back, dout, N * B * 96) == 0
        assert back.raw == batched
    finally:
        eng.lib.kzg_dev_free(eng.ctx, dout)
        din.free()


# ---- 6. pairing check ---------------------------------------------------------------------------------------------------------
@pytest.mark.limit(600)
def test_every_proof_verifies(eng, params, plans):
    rng = random.Random(6)
    plan = plans(12)
    N = 1 << 12
    coeffs = rand_scalars(rng, N)
    proofs = split(all_coeff(eng, plan, pack_scalars(coeffs), N, 1).raw, 96, N)
    prover = kzg_amd.KZGProver(params)
    commitment = prover.commit(kzg_amd.Polynomial(coeffs, N - 1))
    w = M.compute_omega(N)[2]
    ys = evals_at_domain(coeffs, N)
    points = [(pow(w, m, M.R), ys[m]) for m in range(N)]
    ver = kzg_amd.KZGVerifier(params)
    assert all(ver.verify_eval_many(points, [commitment] * N, proofs))
    i, j = 17, 3001
    proofs[i], proofs[j] = proofs[j], proofs[i]
    ok = ver.verify_eval_many(points, [commitment] * N, proofs)
    assert [m for m in range(N) if not ok[m]] == [i, j]


# ---- 7. known-tau random combination at full size -----------------------------------------------------------------------------
@pytest.mark.limit(900)
@pytest.mark.parametrize("log_n", [16, 20])
def test_known_tau_random_combination(eng, log_n):
    rng = random.Random(7 + log_n)
    N = 1 << log_n
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    plan = kzg_amd.FK20Plan(eng, gs, log_n)
    try:
        coeffs = rand_scalars(rng, N)
        proofs = all_coeff(eng, plan, pack_scalars(coeffs), N, 1).raw
    finally:
        plan.free()
        gs.free()
    srs = kzg_amd.Srs.upload(eng, proofs, N)
    try:
        r = [rng.randrange(M.R) for _ in range(N)]
        got = eng.msm(srs, r)
    finally:
        srs.free()
    ys = evals_at_domain(coeffs, N)
    p_tau = C.poly_eval(coeffs, TAU)
    w = M.compute_omega(N)[2]
    # sum r_m (p(tau) - p(w^m)) / (tau - w^m), one batched inversion
    dens, x = [], 1
    for m in range(N):
        dens.append((TAU - x) % M.R)
        x = x * w % M.R
    pref = [1] * (N + 1)
    for m in range(N):
        pref[m + 1] = pref[m] * dens[m] % M.R
    inv = pow(pref[N], M.R - 2, M.R)
    total = 0
    for m in range(N - 1, -1, -1):
        inv_m = inv * pref[m] % M.R
        inv = inv * dens[m] % M.R
        total = (total + r[m] * (p_tau - ys[m]) % M.R * inv_m) % M.R
    assert got == C.g1_mul(G(), total)


# ---- 8. validation and sharing ------------------------------------------------------------------------------------------------
def test_validation(eng, params, plans):
    lib = eng.lib
    plan = plans(3)
    N = 8
    out = ctypes.create_string_buffer(96 * N * 2)
    blob = pack_scalars(list(range(1, 2 * N + 2)))

    def coeff(n, batch=1, p=plan):
        return lib.kzg_witness_all_coeff(eng.ctx, p.handle, blob, n, batch, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)

    def ev(d, p=plan):
        return lib.kzg_witness_all_eval(eng.ctx, p.handle, blob, d, 1, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)

    assert coeff(0) == L.KZG_ERR_SHAPE
    assert coeff(N + 1) == L.KZG_ERR_SHAPE
    assert coeff(N) == 0 and coeff(1) == 0 and coeff(N, 0) == 0
    assert ev(N - 1) == L.KZG_ERR_SHAPE and ev(N + 1) == L.KZG_ERR_SHAPE and ev(N) == 0
    # a short SRS: n - 1 > len(srs) is the reference's slice panic; n - 1 == len(srs) is exact
    short = kzg_amd.setup(eng, TAU, 5, g2_len=0).gs
    sp = kzg_amd.FK20Plan(eng, short, 3)
    try:
        assert coeff(7, p=sp) == L.KZG_ERR_SHAPE
        assert ev(N, p=sp) == L.KZG_ERR_SHAPE
        assert coeff(6, p=sp) == 0
        assert out.raw[:96 * N] == all_coeff(eng, plan, blob, 6, 1).raw[:96 * N]
    finally:
        sp.free()
        short.free()
    h = ctypes.c_void_p()
    assert lib.kzg_fk20_setup(eng.ctx, params.gs.handle, 23, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_fk20_setup(eng.ctx, params.gs.handle, 31, ctypes.byref(h)) == L.KZG_ERR_DEGREE_TOO_LARGE
    assert lib.kzg_fk20_setup(eng.ctx, params.gs.handle, 40, ctypes.byref(h)) == L.KZG_ERR_DEGREE_TOO_LARGE
    with pytest.raises(kzg_amd.ReferencePanic):
        kzg_amd.FK20Plan(eng, params.gs, 23)


def test_plan_of_another_device(eng, hooks, params):
    # a plan pretending to live on GPU 1: built from an SRS the hooks build marks as resident there
    hooks.lib.kzg_test_srs_set_device.argtypes = [VP, I32]
    hooks.lib.kzg_test_srs_set_device.restype = I32
    plan = kzg_amd.FK20Plan(eng, params.gs, 2)
    try:
        # the plan handle is opaque; its first field is the device (struct kzg_fk20 in g1ntt.hip)
        ctypes.cast(plan.handle, ctypes.POINTER(ctypes.c_int))[0] = 1
        out = ctypes.create_string_buffer(96 * 4)
        rc = eng.lib.kzg_witness_all_coeff(eng.ctx, plan.handle, pack_scalars([1, 2, 3]), 3, 1, L.FR_CANONICAL, 0, out,
                                           L.G1_AFFINE_MONT)
        assert rc == L.KZG_ERR_SHAPE
        ctypes.cast(plan.handle, ctypes.POINTER(ctypes.c_int))[0] = 0
        assert hooks.lib.kzg_test_srs_set_device(params.gs.handle, 1) == 0
        h = ctypes.c_void_p()
        assert eng.lib.kzg_fk20_setup(eng.ctx, params.gs.handle, 2, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    finally:
        hooks.lib.kzg_test_srs_set_device(params.gs.handle, 0)
        plan.free()


@pytest.mark.limit(300)
def test_plan_shared_by_two_threads_on_two_contexts(eng, plans):
    rng = random.Random(8)
    plan = plans(10)
    N = 1 << 10
    blob = pack_scalars(rand_scalars(rng, N))
    want = all_coeff(eng, plan, blob, N, 1).raw
    other = [kzg_amd.Engine(0), kzg_amd.Engine(0)]
    results, errors = [None, None], []

    def work(k):
        try:
            results[k] = [all_coeff(other[k], plan, blob, N, 1).raw for _ in range(3)]
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)
    try:
        ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        for e in other:
            e.close()
    assert not errors, errors
    assert all(r == want for rs in results for r in rs)
