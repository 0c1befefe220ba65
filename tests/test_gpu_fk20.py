"""FK20 (kzg_fk20_setup / kzg_witness_all_coeff / kzg_witness_all_eval, kzg_amd/csrc/g1ntt.hip) and its building blocks on the
GPU.  This file sorts after the tests that release the session's contexts (tests/conftest.py ORDER), so it opens and closes its own
module-scoped Engine and HooksEngine instead of the session fixtures."""
import ctypes
import random
import threading
from types import SimpleNamespace

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import _raise, pack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import fk20_model as F
from tests.fk20_common import FORMATS, MONT_R, SIZE_MAX, VP, I32, G, dev_buffer, dev_download, same_point, split
from tests.fk20_common import eng, hooks, params, plans  # noqa: F401 -- this module's fixtures
from tests.gpu_common import rand_scalars

pytestmark = pytest.mark.gpu

TAU = 0x5EED_F20
SRS_LEN = 1 << 12
G2_LEN = 2
PLAN = kzg_amd.FK20Plan


def all_coeff(eng, plan, blob, n, batch, ofmt=L.G1_AFFINE_MONT, sfmt=L.FR_CANONICAL, flags=0, out=None, evals=False):
    """kzg_witness_all_coeff, or kzg_witness_all_eval with evals=True (then n = N)"""
    N = plan.domain()
    psz = L.POINT_BYTES[ofmt]
    buf = out if out is not None else ctypes.create_string_buffer(psz * N * batch)
    fn = eng.lib.kzg_witness_all_eval if evals else eng.lib.kzg_witness_all_coeff
    rc = fn(eng.ctx, plan.handle, blob, n, batch, sfmt, flags, buf, ofmt)
    if rc:
        _raise(eng, rc)
    return buf


def evals_at_domain(coeffs, N):
    return C.fft(list(coeffs) + [0] * (N - len(coeffs)))


def mont(xs):
    return [x * MONT_R % M.R for x in xs]


def known_tau_check(eng, rng, coeffs, N, proofs, ys=None):
    """All N affine proofs of `coeffs` over the size-N domain (an SRS of this file's TAU) at once, by a route that shares
    nothing with how they were computed: the MSM sum_m r_m pi_m against [sum_m r_m (p(tau) - p(w^m)) / (tau - w^m)] G."""
    srs = kzg_amd.Srs.upload(eng, proofs, N)
    try:
        r = [rng.randrange(M.R) for _ in range(N)]
        got = eng.msm(srs, r)
    finally:
        srs.free()
    ys = evals_at_domain(coeffs, N) if ys is None else ys
    p_tau = C.poly_eval(coeffs, TAU)
    w = M.compute_omega(N)[2]
    # one batched inversion of the denominators
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
    assert got == C.g1_mul(G(), total), N


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


@pytest.mark.limit(300)
@pytest.mark.parametrize("log_n", [3, 10])
def test_scalar_forms_and_eval_form_through_the_abi(eng, plans, log_n):
    # Montgomery coefficients, canonical and Montgomery evaluations: the same witnesses as canonical coefficients, in every
    # output format and in a batch of 3
    rng = random.Random(450 + log_n)
    N, B = 1 << log_n, 3
    plan = plans(log_n)
    polys = [rand_scalars(rng, N, kind) for kind in ("full", "u64", "full")]
    coeffs = [c for p in polys for c in p]
    evs = [e for p in polys for e in C.fft(p)]
    inputs = [(pack_scalars(mont(coeffs)), L.FR_MONT, False), (pack_scalars(evs), L.FR_CANONICAL, True),
              (pack_scalars(mont(evs)), L.FR_MONT, True)]
    for ofmt in FORMATS:
        psz = L.POINT_BYTES[ofmt]
        want = all_coeff(eng, plan, pack_scalars(coeffs), N, B, ofmt).raw
        for b in range(B):
            assert all_coeff(eng, plan, pack_scalars(polys[b]), N, 1, ofmt).raw == want[b * N * psz:(b + 1) * N * psz], (ofmt, b)
        want = split(want, psz, B * N)
        for blob, sfmt, evals in inputs:
            got = split(all_coeff(eng, plan, blob, N, B, ofmt, sfmt=sfmt, evals=evals).raw, psz, B * N)
            for i in range(B * N):
                assert same_point(got[i], want[i], ofmt), (N, ofmt, sfmt, evals, i)


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
def run_known_tau(eng, log_n):
    rng = random.Random(7 + log_n)
    N = 1 << log_n
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    try:
        plan = kzg_amd.FK20Plan(eng, gs, log_n)
        try:
            coeffs = rand_scalars(rng, N)
            proofs = all_coeff(eng, plan, pack_scalars(coeffs), N, 1).raw
        finally:
            plan.free()
        # 16 openings through kzg_witness_coeff_many, an MSM route that shares no G1 DFT with FK20
        idx = [0, 1, N // 2, N - 1]
        while len(idx) < 16:
            m = rng.randrange(N)
            if m not in idx:
                idx.append(m)
        ys = evals_at_domain(coeffs, N)
        w = M.compute_omega(N)[2]
        prover = kzg_amd.KZGProver(kzg_amd.KZGParams(gs))
        want, ok = prover.create_witness_many(kzg_amd.Polynomial(coeffs, N - 1), [(pow(w, m, M.R), ys[m]) for m in idx])
        assert all(ok)
        for m, wm in zip(idx, want):
            assert proofs[m * 96:(m + 1) * 96] == wm, (N, m)
    finally:
        gs.free()
    known_tau_check(eng, rng, coeffs, N, proofs, ys)


@pytest.mark.limit(900)
@pytest.mark.parametrize("log_n", [16, 20])
def test_known_tau_random_combination(eng, log_n):
    run_known_tau(eng, log_n)


@pytest.mark.limit(300)  # measured on one MI355X: 22 s, most of it the Python oracle
def test_known_tau_random_combination_at_the_limit(eng):
    # log_n = 22 = FK20_MAX_LOG: 2^22 polynomial coefficients, a plan of 2^23 points, G1 DFTs of 2^23 (inverse) and 2^22 points
    run_known_tau(eng, 22)


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

    # unknown formats, NULL arguments, a batch whose sizes overflow: rejected, in both forms, before any memory is touched
    sentinel = b"\xa5" * len(out)
    ctypes.memmove(out, sentinel, len(sentinel))
    for fn in (lib.kzg_witness_all_coeff, lib.kzg_witness_all_eval):
        def call(fn=fn, ctx=eng.ctx, p=plan.handle, src=blob, batch=1, sfmt=L.FR_CANONICAL, o=out, ofmt=L.G1_AFFINE_MONT):
            return fn(ctx, p, src, N, batch, sfmt, 0, o, ofmt)
        assert call(sfmt=7) == L.KZG_ERR_SHAPE and call(ofmt=99) == L.KZG_ERR_SHAPE
        assert call(src=None) == L.KZG_ERR_SHAPE and call(o=None) == L.KZG_ERR_SHAPE
        assert call(p=None) == L.KZG_ERR_SHAPE and call(ctx=None) == L.KZG_ERR_SHAPE
        assert call(batch=SIZE_MAX // (N * 144) + 1) == L.KZG_ERR_SHAPE and call(batch=SIZE_MAX) == L.KZG_ERR_SHAPE
    assert out.raw == sentinel
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
        # the plan handle is opaque; its first field is the device (struct Fk20Plan in g1ntt.hip)
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


# ---- 9. batches of several chunks ---------------------------------------------------------------------------------------------
# fk20_run works through a batch in chunks of F.chunk_size(N) polynomials, the last one ragged, with n < N so that the input
# (b0 n) and output (b0 N) offsets differ.  Every batched result equals single calls (one chunk each), and the polynomials at
# chunk edges also pass an oracle that shares no code with the batched path.
@pytest.fixture(scope="module")
def batch14(eng):
    """130 = 64 + 64 + 2 polynomials of N - 3 coefficients at N = 2^14 (chunk 64) on a local SRS, and their witnesses from one
    batched coeff-form call"""
    log_n = 14
    N = 1 << log_n
    assert F.chunk_size(N) == 64
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    plan = kzg_amd.FK20Plan(eng, gs, log_n)
    rng = random.Random(90)
    n, B = N - 3, 130
    polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
    blob = b"".join(pack_scalars(p) for p in polys)
    out = all_coeff(eng, plan, blob, n, B).raw
    yield SimpleNamespace(plan=plan, N=N, n=n, B=B, polys=polys, blob=blob, out=out)
    plan.free()
    gs.free()


@pytest.mark.limit(600)
def test_chunked_batch_coeff_form(eng, batch14):
    t = batch14
    N, n, B, sz = t.N, t.n, t.B, t.N * 96
    rng = random.Random(91)
    for b in range(B):
        assert all_coeff(eng, t.plan, pack_scalars(t.polys[b]), n, 1).raw == t.out[b * sz:(b + 1) * sz], b
    for b in (63, 64, 129):  # the last of chunk 0, the first of chunk 1, the last of the ragged chunk 2
        known_tau_check(eng, rng, t.polys[b], N, t.out[b * sz:(b + 1) * sz])
    din = eng.alloc_scalars(n * B)
    din.upload(t.blob)
    dout = dev_buffer(eng, sz * B)
    try:
        assert all_coeff(eng, t.plan, din.ptr, n, B, flags=L.IN_DEVICE).raw == t.out
        for flags, src in ((L.OUT_DEVICE, t.blob), (L.IN_DEVICE | L.OUT_DEVICE, din.ptr)):
            assert eng.lib.kzg_dev_upload(eng.ctx, dout, b"\xa5" * (sz * B), sz * B) == 0
            all_coeff(eng, t.plan, src, n, B, flags=flags, out=dout)
            assert dev_download(eng, dout, sz * B) == t.out, flags
    finally:
        eng.lib.kzg_dev_free(eng.ctx, dout)
        din.free()
    mblob = pack_scalars(mont(c for p in t.polys for c in p))
    assert all_coeff(eng, t.plan, mblob, n, B, sfmt=L.FR_MONT).raw == t.out


@pytest.mark.limit(600)
def test_chunked_batch_eval_form(eng, batch14):
    t = batch14
    N, B = t.N, t.B
    evs = [e for p in t.polys for e in evals_at_domain(p, N)]
    for sfmt, vals in ((L.FR_CANONICAL, evs), (L.FR_MONT, mont(evs))):
        blob = pack_scalars(vals)
        assert all_coeff(eng, t.plan, blob, N, B, sfmt=sfmt, evals=True).raw == t.out, sfmt
        din = eng.alloc_scalars(N * B, sfmt)
        try:
            din.upload(blob)
            assert all_coeff(eng, t.plan, din.ptr, N, B, sfmt=sfmt, flags=L.IN_DEVICE, evals=True).raw == t.out, sfmt
        finally:
            din.free()


@pytest.mark.limit(600)
def test_chunk_cap_branch(eng, params, plans):
    # N = 64: FK20_CHUNK_POINTS / 2N = 16384, so FK20_MAX_CHUNK sets the chunk; 4099 = 4096 + 3
    rng = random.Random(92)
    N, n, B = 64, 61, 4099
    assert F.chunk_size(N) == 4096 < (1 << 21) // (2 * N)
    plan = plans(6)
    polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
    out = all_coeff(eng, plan, b"".join(pack_scalars(p) for p in polys), n, B).raw
    sz = N * 96
    prover = kzg_amd.KZGProver(params)
    w = M.compute_omega(N)[2]
    xs = [pow(w, m, M.R) for m in range(N)]
    for b in (0, 4095, 4096, 4098):
        got = out[b * sz:(b + 1) * sz]
        assert all_coeff(eng, plan, pack_scalars(polys[b]), n, 1).raw == got, b
        want, ok = prover.create_witness_many(kzg_amd.Polynomial(polys[b], n - 1), list(zip(xs, evals_at_domain(polys[b], N))))
        assert all(ok) and b"".join(want) == got, b
    eblob = b"".join(pack_scalars(evals_at_domain(p, N)) for p in polys)
    assert all_coeff(eng, plan, eblob, N, B, evals=True).raw == out


@pytest.mark.limit(600)
def test_chunk_of_one(eng):
    # N = 2^20: one polynomial per chunk; host output in the 48-byte compressed form, device output affine
    rng = random.Random(93)
    log_n = 20
    N = 1 << log_n
    n, B = N - 5, 3
    assert F.chunk_size(N) == 1
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    try:
        plan = kzg_amd.FK20Plan(eng, gs, log_n)
        try:
            polys = [rand_scalars(rng, n, "u64" if b == 1 else "full") for b in range(B)]
            blob = b"".join(pack_scalars(p) for p in polys)
            comp = all_coeff(eng, plan, blob, n, B, ofmt=L.G1_ZCASH_COMPRESSED).raw
            dout = dev_buffer(eng, N * B * 96)
            try:
                all_coeff(eng, plan, blob, n, B, flags=L.OUT_DEVICE, out=dout)
                aff = dev_download(eng, dout, N * B * 96)
            finally:
                eng.lib.kzg_dev_free(eng.ctx, dout)
            for b in range(B):
                one = pack_scalars(polys[b])
                for ofmt, got in ((L.G1_ZCASH_COMPRESSED, comp), (L.G1_AFFINE_MONT, aff)):
                    psz = L.POINT_BYTES[ofmt]
                    assert all_coeff(eng, plan, one, n, 1, ofmt).raw == got[b * N * psz:(b + 1) * N * psz], (b, ofmt)
        finally:
            plan.free()
    finally:
        gs.free()
    known_tau_check(eng, rng, polys[2], N, aff[2 * N * 96:])


def test_domain_of_one(eng, params, plans):
    # N = 1: every quotient is zero; each element is the identity as kzg_witness_coeff_many writes it
    rng = random.Random(94)
    plan = plans(0)
    B = 5
    cs = [rng.randrange(M.R) for _ in range(B)]
    prover = kzg_amd.KZGProver(params)
    for ofmt in FORMATS:
        psz = L.POINT_BYTES[ofmt]
        want, ok = prover.create_witness_many(kzg_amd.Polynomial(cs[:1], 0), [(1, cs[0])], ofmt)
        assert ok == [True]
        host = ctypes.create_string_buffer(b"\xa5" * (psz * B), psz * B)
        all_coeff(eng, plan, pack_scalars(cs), 1, B, ofmt, out=host)
        assert split(host.raw, psz, B) == want * B, ofmt
        dout = dev_buffer(eng, psz * B)
        try:
            all_coeff(eng, plan, pack_scalars(cs), 1, B, ofmt, flags=L.OUT_DEVICE, out=dout)
            assert split(dev_download(eng, dout, psz * B), psz, B) == want * B, ofmt
        finally:
            eng.lib.kzg_dev_free(eng.ctx, dout)
