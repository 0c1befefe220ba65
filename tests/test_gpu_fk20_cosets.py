"""Multi-point FK20 (kzg_fk20_cosets_setup / kzg_witness_cosets_coeff / kzg_witness_cosets_eval, kzg_amd/csrc/g1ntt.hip): every
coset opening of a polynomial in one call, against kzg_witness_coeff_batched at the coset's points, and the combination kernel
alone through its hook.  Like tests/test_gpu_fk20.py this file sorts after the tests that release the session's contexts, so it
opens and closes its own module-scoped Engine and HooksEngine."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import _raise, pack_scalars, unpack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import fk20_model as F
from tests.fk20_common import FORMATS, MONT_R, SIZE_MAX, VP, I32, G, dev_buffer, dev_download, same_point, split
from tests.fk20_common import eng, hooks, params, plans  # noqa: F401 -- this module's fixtures
from tests.gpu_common import rand_scalars

pytestmark = pytest.mark.gpu

TAU = 0x5EED_C05E7
SRS_LEN = 1 << 12
G2_LEN = 17
PLAN = kzg_amd.FK20CosetPlan


def cosets(eng, plan, blob, n, batch, ofmt=L.G1_AFFINE_MONT, sfmt=L.FR_CANONICAL, flags=0, out_w=None, out_r=None, want_r=True,
           evals=False):
    """(witness bytes, interpolant bytes or None)"""
    N, l = plan.domain(), plan.coset_size()
    K = N // l
    w = out_w if out_w is not None else ctypes.create_string_buffer(L.POINT_BYTES[ofmt] * K * batch)
    r = out_r if out_r is not None else (ctypes.create_string_buffer(32 * N * batch) if want_r else None)
    fn = eng.lib.kzg_witness_cosets_eval if evals else eng.lib.kzg_witness_cosets_coeff
    rc = fn(eng.ctx, plan.handle, blob, n, batch, sfmt, flags, w, ofmt, r)
    if rc:
        _raise(eng, rc)
    return w, r


def batched(eng, params, coeffs, xs, ys, ofmt, sfmt=L.FR_CANONICAL):
    """kzg_witness_coeff_batched: (witness bytes, interpolant bytes in sfmt)"""
    conv = (lambda v: v) if sfmt == L.FR_CANONICAL else (lambda v: v * MONT_R % M.R)
    k = len(xs)
    w = ctypes.create_string_buffer(L.POINT_BYTES[ofmt])
    r = ctypes.create_string_buffer(32 * max(k, 2))
    rlen = ctypes.c_size_t()
    rc = eng.lib.kzg_witness_coeff_batched(eng.ctx, params.gs.handle, pack_scalars([conv(c) for c in coeffs]), len(coeffs),
                                           pack_scalars([conv(x) for x in xs]), pack_scalars([conv(y) for y in ys]), k, sfmt, 0, w,
                                           ofmt, r, ctypes.byref(rlen))
    if rc:
        _raise(eng, rc)
    assert rlen.value == k
    return w.raw, r.raw[:32 * k]


def coset_values(coeffs, N, l):
    """(xs, ys) of every coset, in the plan's point order"""
    K = N // l
    ev = C.fft(list(coeffs) + [0] * (N - len(coeffs)))
    w = M.compute_omega(N)[2]
    return [([pow(w, i + t * K, M.R) for t in range(l)], [ev[i + t * K] for t in range(l)]) for i in range(K)]


# ---- 1. byte equality with kzg_witness_coeff_batched --------------------------------------------------------------------------
CASES = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (4, 2), (4, 4), (6, 1), (6, 3), (6, 6), (10, 1), (10, 4), (10, 7), (10, 10)]


@pytest.mark.limit(900)
@pytest.mark.parametrize("log_n,log_l", CASES)
def test_matches_batched_witness(eng, params, plans, log_n, log_l):
    rng = random.Random(100 * log_n + log_l)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    plan = plans(log_n, log_l)
    assert (plan.domain(), plan.coset_size(), plan.num_cosets()) == (N, l, K)
    # at 2^10 with small cosets every coset is still checked for one n; the others take an even spread of cosets
    for n in sorted({N, max(1, N - 3), min(N, l + 1), l, max(1, l - 1), 1}):
        coeffs = rand_scalars(rng, n, "full" if n % 2 else "u64")
        vals = coset_values(coeffs, N, l)
        full = n == N
        check = range(K) if (full or K <= 64) else sorted(set(rng.sample(range(K), 24)) | {0, K - 1})
        for ofmt in (FORMATS if full else [L.G1_AFFINE_MONT]):
            psz = L.POINT_BYTES[ofmt]
            got_w, got_r = cosets(eng, plan, pack_scalars(coeffs), n, 1, ofmt)
            ws = split(got_w.raw, psz, K)
            for i in check:
                assert plan.coset_points(i) == vals[i][0]
                want_w, want_r = batched(eng, params, coeffs, vals[i][0], vals[i][1], ofmt)
                assert same_point(ws[i], want_w, ofmt), (N, l, n, ofmt, i)
                assert got_r.raw[i * l * 32:(i + 1) * l * 32] == want_r, (N, l, n, i)
        if full:  # Montgomery scalars in and out
            mont = pack_scalars([c * MONT_R % M.R for c in coeffs])
            got_w, got_r = cosets(eng, plan, mont, n, 1, sfmt=L.FR_MONT)
            for i in list(check)[:8]:
                want_w, want_r = batched(eng, params, coeffs, vals[i][0], vals[i][1], L.G1_AFFINE_MONT, L.FR_MONT)
                assert got_w.raw[i * 96:(i + 1) * 96] == want_w and got_r.raw[i * l * 32:(i + 1) * l * 32] == want_r, (N, l, i)


def test_python_surface(eng, params, plans):
    rng = random.Random(17)
    plan = plans(4, 2)
    coeffs = rand_scalars(rng, 13)
    poly = kzg_amd.Polynomial(coeffs, 12)
    prover = kzg_amd.KZGProver(params)
    single = prover.create_witness_all_cosets(poly, plan)
    assert len(single) == 4
    vals = coset_values(coeffs, 16, 4)
    for i, wit in enumerate(single):
        ref = prover.create_witness_batched(poly, *vals[i])
        assert wit.elem() == ref.elem() and wit.polynomial().slice_coeffs() == ref.polynomial().slice_coeffs(), i
    both = prover.create_witness_all_cosets_batch([poly, kzg_amd.Polynomial(coeffs[:5], 4)], plan)
    assert [w.elem() for w in both[0]] == [w.elem() for w in single]
    short = prover.create_witness_all_cosets(kzg_amd.Polynomial(coeffs[:5] + [0] * 8, 12), plan)
    assert [w.elem() for w in both[1]] == [w.elem() for w in short]


# ---- 2. evaluation form -------------------------------------------------------------------------------------------------------
@pytest.mark.limit(300)
@pytest.mark.parametrize("log_n,log_l", [(1, 1), (3, 1), (6, 2), (10, 4), (10, 10)])
def test_eval_form_equals_coeff_form(eng, params, plans, log_n, log_l):
    rng = random.Random(200 + log_n)
    N = 1 << log_n
    plan = plans(log_n, log_l)
    for kind in ("full", "u64"):
        coeffs = rand_scalars(rng, N, kind)
        evals = C.fft(coeffs)
        for sfmt, conv in ((L.FR_CANONICAL, lambda v: v), (L.FR_MONT, lambda v: v * MONT_R % M.R)):
            w_c, r_c = cosets(eng, plan, pack_scalars([conv(c) for c in coeffs]), N, 1, sfmt=sfmt)
            w_e, r_e = cosets(eng, plan, pack_scalars([conv(e) for e in evals]), N, 1, sfmt=sfmt, evals=True)
            assert w_c.raw == w_e.raw and r_c.raw == r_e.raw, (N, kind, sfmt)
    ev = kzg_amd.EvaluationDomain(evals, N, log_n, M.compute_omega(N)[2])
    lag = kzg_amd.setup_lagrange(eng, TAU, N)
    try:
        got = kzg_amd.KZGProverEvalForm(params, lag).create_witness_all_cosets(ev, plan)
    finally:
        lag.free()
    assert [g.elem() for g in got] == split(w_c.raw, 96, N >> log_l)


# ---- 3. batch and device buffers ----------------------------------------------------------------------------------------------
@pytest.mark.limit(600)
@pytest.mark.parametrize("log_n,log_l", [(12, 4), (8, 1)])
def test_batch_equals_single_calls_and_device_flags(eng, plans, log_n, log_l):
    rng = random.Random(5 + log_n)
    plan = plans(log_n, log_l)
    N, l, B = 1 << log_n, 1 << log_l, 64
    K = N // l
    n = N - 3
    polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
    blob = b"".join(pack_scalars(p) for p in polys)
    bw, br = cosets(eng, plan, blob, n, B)
    bw, br = bw.raw, br.raw
    for b in range(0, B, 7):
        w1, r1 = cosets(eng, plan, pack_scalars(polys[b]), n, 1)
        assert w1.raw == bw[b * K * 96:(b + 1) * K * 96] and r1.raw == br[b * N * 32:(b + 1) * N * 32], b
    wn, rn = cosets(eng, plan, blob, n, B, want_r=False)
    assert rn is None and wn.raw == bw
    din = eng.alloc_scalars(n * B)
    din.upload(blob)
    dw, dr = ctypes.c_void_p(), ctypes.c_void_p()
    assert eng.lib.kzg_dev_alloc(eng.ctx, K * B * 96, ctypes.byref(dw)) == 0
    assert eng.lib.kzg_dev_alloc(eng.ctx, N * B * 32, ctypes.byref(dr)) == 0
    try:
        for flags in (L.IN_DEVICE, L.OUT_DEVICE, L.IN_DEVICE | L.OUT_DEVICE):
            src = din.ptr if flags & L.IN_DEVICE else blob
            for with_r in (True, False):
                if flags & L.OUT_DEVICE:
                    assert eng.lib.kzg_dev_upload(eng.ctx, dw, bytes(K * B * 96), K * B * 96) == 0
                    assert eng.lib.kzg_dev_upload(eng.ctx, dr, bytes(N * B * 32), N * B * 32) == 0
                    cosets(eng, plan, src, n, B, flags=flags, out_w=dw, out_r=dr if with_r else None, want_r=with_r)
                    back_w = ctypes.create_string_buffer(K * B * 96)
                    assert eng.lib.kzg_dev_download(eng.ctx, back_w, dw, K * B * 96) == 0
                    assert back_w.raw == bw, (flags, with_r)
                    if with_r:
                        back_r = ctypes.create_string_buffer(N * B * 32)
                        assert eng.lib.kzg_dev_download(eng.ctx, back_r, dr, N * B * 32) == 0
                        assert back_r.raw == br, flags
                else:
                    w, r = cosets(eng, plan, src, n, B, flags=flags, want_r=with_r)
                    assert w.raw == bw and (r is None or r.raw == br), (flags, with_r)
    finally:
        eng.lib.kzg_dev_free(eng.ctx, dw)
        eng.lib.kzg_dev_free(eng.ctx, dr)
        din.free()


# ---- 4. pairing checks --------------------------------------------------------------------------------------------------------
@pytest.mark.limit(600)
def test_every_coset_proof_verifies(eng, params, plans):
    rng = random.Random(6)
    plan = plans(12, 4)
    N, l = 1 << 12, 16
    K = N // l
    coeffs = rand_scalars(rng, N)
    poly = kzg_amd.Polynomial(coeffs, N - 1)
    prover = kzg_amd.KZGProver(params)
    wits = prover.create_witness_all_cosets(poly, plan)
    commitment = prover.commit(poly)
    ver = kzg_amd.KZGVerifier(params)
    for i in range(K):
        assert ver.verify_eval_batched(plan.coset_points(i), commitment, wits[i]), i
    a, b = 5, 201
    swapped_a = kzg_amd.KZGBatchWitness(wits[a].r, wits[b].w)
    swapped_b = kzg_amd.KZGBatchWitness(wits[b].r, wits[a].w)
    assert not ver.verify_eval_batched(plan.coset_points(a), commitment, swapped_a)
    assert not ver.verify_eval_batched(plan.coset_points(b), commitment, swapped_b)


# ---- 5. known-tau random combination at full size -----------------------------------------------------------------------------
def run_known_tau(eng, log_n, log_l):
    rng = random.Random(7 + log_n)
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    try:
        plan = kzg_amd.FK20CosetPlan(eng, gs, log_n, log_l)
        try:
            coeffs = rand_scalars(rng, N)
            proofs, interp = cosets(eng, plan, pack_scalars(coeffs), N, 1)
            proofs, interp = proofs.raw, interp.raw
        finally:
            plan.free()
        # the interpolants, independently: coefficient r of I_i is DFT_K(c^(r))_i
        cols = [C.fft(coeffs[r::l]) for r in range(l)]
        # two cosets through kzg_witness_coeff_batched, an MSM route that shares no G1 DFT with the plan (p = I_i on coset i)
        w = M.compute_omega(N)[2]
        params = kzg_amd.KZGParams(gs)
        for i in (K - 1, rng.randrange(K - 1)):
            xs = [pow(w, i + t * K, M.R) for t in range(l)]
            ys = [sum(cols[r][i] * pow(x, r, M.R) for r in range(l)) % M.R for x in xs]
            want_w, want_r = batched(eng, params, coeffs, xs, ys, L.G1_AFFINE_MONT)
            assert proofs[i * 96:(i + 1) * 96] == want_w and interp[i * l * 32:(i + 1) * l * 32] == want_r, (N, l, i)
    finally:
        gs.free()
    I = unpack_scalars(interp)
    sample = [0, 1, K - 1] + rng.sample(range(K), 61)
    for i in sample:
        assert I[i * l:(i + 1) * l] == [cols[r][i] for r in range(l)], i
    srs = kzg_amd.Srs.upload(eng, proofs, K)
    try:
        rho = [rng.randrange(M.R) for _ in range(K)]
        got = eng.msm(srs, rho)
    finally:
        srs.free()
    # sum rho_i (p(tau) - I_i(tau)) / (tau^l - w^(il)), one batched inversion
    p_tau = C.poly_eval(coeffs, TAU)
    tpow = [pow(TAU, r, M.R) for r in range(l)]
    wk = pow(M.compute_omega(N)[2], l, M.R)
    tl = pow(TAU, l, M.R)
    dens, z = [], 1
    for i in range(K):
        dens.append((tl - z) % M.R)
        z = z * wk % M.R
    pref = [1] * (K + 1)
    for i in range(K):
        pref[i + 1] = pref[i] * dens[i] % M.R
    inv = pow(pref[K], M.R - 2, M.R)
    total = 0
    for i in range(K - 1, -1, -1):
        inv_i = inv * pref[i] % M.R
        inv = inv * dens[i] % M.R
        i_tau = sum(cols[r][i] * tpow[r] for r in range(l)) % M.R
        total = (total + rho[i] * (p_tau - i_tau) % M.R * inv_i) % M.R
    assert got == C.g1_mul(G(), total)


@pytest.mark.limit(900)
@pytest.mark.parametrize("log_n,log_l", [(16, 4), (20, 6)])
def test_known_tau_random_combination(eng, log_n, log_l):
    run_known_tau(eng, log_n, log_l)


@pytest.mark.limit(300)  # measured on one MI355X: 17 s (l = 2), 10 s (l = 64)
@pytest.mark.parametrize("log_l", [1, 6])
def test_known_tau_random_combination_at_the_limit(eng, log_l):
    # log_n = 22 = FK20_MAX_LOG.  l = 2 has the largest K: G1 DFTs of 2^22 (inverse) and 2^21 points and a plan of 8.6 GB;
    # l = 64 has a 64-term combination per frequency
    run_known_tau(eng, 22, log_l)


# ---- 6. the combination kernel alone ------------------------------------------------------------------------------------------
def combine(hooks, bases, ks, l, m, route, slices=0):
    out = ctypes.create_string_buffer(96 * m)
    rc = hooks.lib.kzg_test_fk20_cosets_combine(hooks.ctx, b"".join(bases), pack_scalars(ks), l, m, route, slices, out)
    assert rc == 0, hooks.last_error()
    return split(out.raw, 96, m)


@pytest.mark.limit(600)
@pytest.mark.parametrize("route", [0, 1])
def test_combination_hook_edge_cases(hooks, route):
    rng = random.Random(60 + route)
    l, m = 16, 48
    R = M.R
    edge_k = [0, 1, R - 1, 2, R - 2]
    # discrete logs b[r][j] of the bases (0 = the identity) and scalars k[r][j]; column j is one scenario
    b = [[rng.randrange(1, R) for _ in range(m)] for _ in range(l)]
    k = [[rng.randrange(R) for _ in range(m)] for _ in range(l)]
    for j in range(m):
        sc = j % 8
        if sc == 0:                          # identity bases throughout
            for r in range(l):
                b[r][j] = 0
        elif sc == 1:                        # equal bases and equal scalars: the doubling branch of the mixed addition
            for r in range(l):
                b[r][j], k[r][j] = b[0][j], k[0][j]
        elif sc == 2:                        # base and its negation with equal scalars: cancellation to the identity
            for r in range(1, l, 2):
                b[r][j], k[r][j] = (R - b[r - 1][j]) % R, k[r - 1][j]
        elif sc == 3:                        # the edge scalars
            for r in range(l):
                k[r][j] = edge_k[(r + j) % len(edge_k)]
        elif sc == 4:                        # equal bases, scalars summing to zero
            for r in range(l):
                b[r][j] = b[0][j]
            k[l - 1][j] = (-sum(k[r][j] for r in range(l - 1))) % R
        elif sc == 5:                        # one identity base among others, scalars 0 on others
            b[3][j] = 0
            k[5][j] = 0
    for r in range(l):                       # a whole residue class of identity bases (a short SRS)
        for j in range(m):
            if r == 7:
                b[r][j] = 0
    bases = [C.g1_mul(G(), b[r][j]) if b[r][j] else bytes(96) for r in range(l) for j in range(m)]
    ks = [k[r][j] for r in range(l) for j in range(m)]
    want = [C.g1_mul(G(), sum(k[r][j] * b[r][j] for r in range(l)) % R) for j in range(m)]
    for slices in (0, 1, 4, l):
        got = combine(hooks, bases, ks, l, m, route, slices)
        for j in range(m):
            assert got[j] == want[j], (route, slices, j)


@pytest.mark.limit(300)
def test_combination_routes_agree(hooks):
    rng = random.Random(61)
    l, m = 64, 256
    bases = [C.g1_mul(G(), rng.randrange(1, M.R)) for _ in range(l * m)]
    ks = [rng.randrange(M.R) for _ in range(l * m)]
    assert combine(hooks, bases, ks, l, m, 0) == combine(hooks, bases, ks, l, m, 1)


@pytest.mark.limit(300)
def test_routes_agree_end_to_end(eng, plans):
    rng = random.Random(62)
    plan = plans(10, 4)
    blob = pack_scalars(rand_scalars(rng, 2 << 10))
    straus = cosets(eng, plan, blob, 1 << 10, 2)[0].raw
    eng.set_option("fk20_cosets_combine", 1)
    try:
        per_term = cosets(eng, plan, blob, 1 << 10, 2)[0].raw
    finally:
        eng.set_option("fk20_cosets_combine", 0)
    assert straus == per_term


# ---- 7. validation ------------------------------------------------------------------------------------------------------------
def test_validation(eng, params, plans):
    lib = eng.lib
    plan = plans(3, 1)
    N, l = 8, 2
    out = ctypes.create_string_buffer(96 * N * 2)
    rbuf = ctypes.create_string_buffer(32 * N * 2)
    blob = pack_scalars(list(range(1, 2 * N + 2)))
    A, CAN = L.G1_AFFINE_MONT, L.FR_CANONICAL

    def coeff(n, batch=1, p=plan, sfmt=CAN, ofmt=A, src=blob, w=out, r=rbuf):
        return lib.kzg_witness_cosets_coeff(eng.ctx, p.handle if p is not None else None, src, n, batch, sfmt, 0, w, ofmt, r)

    def ev(d, p=plan):
        return lib.kzg_witness_cosets_eval(eng.ctx, p.handle, blob, d, 1, CAN, 0, out, A, rbuf)

    assert coeff(0) == L.KZG_ERR_SHAPE
    assert coeff(N + 1) == L.KZG_ERR_SHAPE
    assert coeff(N) == 0 and coeff(1) == 0 and coeff(N, 0) == 0 and coeff(N, r=None) == 0
    assert coeff(N, sfmt=7) == L.KZG_ERR_SHAPE and coeff(N, ofmt=99) == L.KZG_ERR_SHAPE
    assert coeff(N, src=None) == L.KZG_ERR_SHAPE and coeff(N, w=None) == L.KZG_ERR_SHAPE and coeff(N, p=None) == L.KZG_ERR_SHAPE
    assert lib.kzg_witness_cosets_coeff(None, plan.handle, blob, N, 1, CAN, 0, out, A, rbuf) == L.KZG_ERR_SHAPE
    # a batch whose sizes overflow, in both forms: rejected before any memory is touched
    gw, gr = ctypes.create_string_buffer(b"\xa5" * 96, 96), ctypes.create_string_buffer(b"\xa5" * 32, 32)
    for fn in (lib.kzg_witness_cosets_coeff, lib.kzg_witness_cosets_eval):
        for batch in (SIZE_MAX // (N * 144) + 1, SIZE_MAX):
            assert fn(eng.ctx, plan.handle, blob, N, batch, CAN, 0, gw, A, gr) == L.KZG_ERR_SHAPE, batch
    assert gw.raw == b"\xa5" * 96 and gr.raw == b"\xa5" * 32
    assert ev(N - 1) == L.KZG_ERR_SHAPE and ev(N + 1) == L.KZG_ERR_SHAPE and ev(N) == 0
    assert lib.kzg_fk20_cosets_shape(None, None, None) == L.KZG_ERR_SHAPE
    # a short SRS of 3 points: n - l > len(srs) is the reference's slice panic; n - l == len(srs) is exact; n <= l needs none
    short = kzg_amd.setup(eng, TAU, 3, g2_len=0).gs
    sp = kzg_amd.FK20CosetPlan(eng, short, 3, 1)
    try:
        assert coeff(6, p=sp) == L.KZG_ERR_SHAPE
        assert ev(N, p=sp) == L.KZG_ERR_SHAPE
        assert coeff(5, p=sp) == 0
        got = (out.raw[:96 * 4], rbuf.raw[:32 * N])
        w, r = cosets(eng, plan, blob, 5, 1)
        assert got == (w.raw[:96 * 4], r.raw[:32 * N])
        assert coeff(2, p=sp) == 0
    finally:
        sp.free()
        short.free()
    h = ctypes.c_void_p()
    g = params.gs.handle
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 3, 0, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 3, 4, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 23, 2, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 31, 2, ctypes.byref(h)) == L.KZG_ERR_DEGREE_TOO_LARGE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 40, 2, ctypes.byref(h)) == L.KZG_ERR_DEGREE_TOO_LARGE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, None, 3, 1, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_fk20_cosets_setup(eng.ctx, g, 3, 1, None) == L.KZG_ERR_SHAPE
    with pytest.raises(kzg_amd.ReferencePanic):
        kzg_amd.FK20CosetPlan(eng, params.gs, 4, 0)


def test_plan_of_another_device(eng, hooks, params):
    hooks.lib.kzg_test_srs_set_device.argtypes = [VP, I32]
    hooks.lib.kzg_test_srs_set_device.restype = I32
    plan = kzg_amd.FK20CosetPlan(eng, params.gs, 2, 1)
    try:
        # the plan handle is opaque; its first field is the device (struct Fk20Plan in g1ntt.hip)
        ctypes.cast(plan.handle, ctypes.POINTER(ctypes.c_int))[0] = 1
        out = ctypes.create_string_buffer(96 * 2)
        rc = eng.lib.kzg_witness_cosets_coeff(eng.ctx, plan.handle, pack_scalars([1, 2, 3]), 3, 1, L.FR_CANONICAL, 0, out,
                                              L.G1_AFFINE_MONT, None)
        assert rc == L.KZG_ERR_SHAPE
        ctypes.cast(plan.handle, ctypes.POINTER(ctypes.c_int))[0] = 0
        assert hooks.lib.kzg_test_srs_set_device(params.gs.handle, 1) == 0
        h = ctypes.c_void_p()
        assert eng.lib.kzg_fk20_cosets_setup(eng.ctx, params.gs.handle, 2, 1, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    finally:
        hooks.lib.kzg_test_srs_set_device(params.gs.handle, 0)
        plan.free()


# ---- 8. one plan, two threads, two contexts -----------------------------------------------------------------------------------
@pytest.mark.limit(300)
def test_plan_shared_by_two_threads_on_two_contexts(eng, plans):
    rng = random.Random(8)
    plan = plans(10, 3)
    N = 1 << 10
    blob = pack_scalars(rand_scalars(rng, N))
    ww, wr = cosets(eng, plan, blob, N, 1)
    want = (ww.raw, wr.raw)
    other = [kzg_amd.Engine(0), kzg_amd.Engine(0)]
    results, errors = [None, None], []

    def work(k):
        try:
            results[k] = []
            for _ in range(3):
                w, r = cosets(other[k], plan, blob, N, 1)
                results[k].append((w.raw, r.raw))
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
# fk20_run works through a batch in chunks of F.chunk_size(N) polynomials, the last one ragged, and splits each chunk's
# combination into F.coset_slices residue slices chosen from the FIRST chunk.  n < N, so that the input (b0 n) and output (b0 K,
# b0 N) offsets differ.  Every batch equals single calls, and the polynomials at chunk edges also equal kzg_witness_coeff_batched.
@pytest.fixture(scope="module")
def local_srs(eng):
    """monomial SRSs of this file's TAU past the 2^12 fixture, one per size"""
    cache = {}

    def get(log_n):
        if log_n not in cache:
            cache[log_n] = kzg_amd.setup(eng, TAU, 1 << log_n, g2_len=0).gs
        return cache[log_n]
    yield get
    for gs in cache.values():
        gs.free()


def check_edges(eng, gs, polys, N, l, bw, br, edges, count, rng):
    """`count` cosets (0, K - 1, then random ones) of each polynomial b in `edges` against kzg_witness_coeff_batched"""
    K = N // l
    params = kzg_amd.KZGParams(gs)
    w = M.compute_omega(N)[2]
    for b in edges:
        ev = C.fft(polys[b] + [0] * (N - len(polys[b])))
        for i in ([0, K - 1] + rng.sample(range(1, K - 1), max(0, count - 2)))[:count]:
            xs = [pow(w, i + t * K, M.R) for t in range(l)]
            want_w, want_r = batched(eng, params, polys[b], xs, [ev[i + t * K] for t in range(l)], L.G1_AFFINE_MONT)
            assert bw[(b * K + i) * 96:(b * K + i + 1) * 96] == want_w, (N, l, b, i)
            assert br[(b * N + i * l) * 32:(b * N + (i + 1) * l) * 32] == want_r, (N, l, b, i)


@pytest.mark.limit(600)
@pytest.mark.parametrize("route", [0, 1])
def test_chunked_batch_with_sliced_combination(eng, local_srs, route):
    # (14, 6): chunks of 64, 130 = 64 + 64 + 2; the first chunk's S = 4 residue slices are kept for the last chunk of 2
    rng = random.Random(70 + route)
    log_n, log_l = 14, 6
    N, l = 1 << log_n, 1 << log_l
    K, n, B = N // l, N - 3, 130
    chunk = F.chunk_size(N)
    assert (chunk, B % chunk) == (64, 2)
    assert F.coset_slices(l, 2 * K, chunk) == 4, "the slicing rule changed: (14, 6) no longer splits a chunk's residues"
    gs = local_srs(log_n)
    plan = kzg_amd.FK20CosetPlan(eng, gs, log_n, log_l)
    eng.set_option("fk20_cosets_combine", route)
    try:
        polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
        bw, br = cosets(eng, plan, b"".join(pack_scalars(p) for p in polys), n, B)
        bw, br = bw.raw, br.raw
        for b in range(B):
            w1, r1 = cosets(eng, plan, pack_scalars(polys[b]), n, 1)
            assert w1.raw == bw[b * K * 96:(b + 1) * K * 96] and r1.raw == br[b * N * 32:(b + 1) * N * 32], (route, b)
        check_edges(eng, gs, polys, N, l, bw, br, (63, 64, 129), 4, rng)
    finally:
        eng.set_option("fk20_cosets_combine", 0)
        plan.free()


@pytest.mark.limit(600)
def test_chunked_eval_form_on_the_device(eng, local_srs):
    # (16, 4): chunks of 16, 35 = 16 + 16 + 3.  Montgomery evaluations in device memory, witnesses and interpolants written to
    # device memory (offsets b0 K psz and b0 N 32), against the host canonical coeff-form batch
    rng = random.Random(72)
    log_n, log_l = 16, 4
    N, l = 1 << log_n, 1 << log_l
    K, n, B = N // l, N - 3, 35
    assert (F.chunk_size(N), B % F.chunk_size(N)) == (16, 3)
    gs = local_srs(log_n)
    plan = kzg_amd.FK20CosetPlan(eng, gs, log_n, log_l)
    din = dw = dr = None
    try:
        polys = [rand_scalars(rng, n, "full" if b % 2 else "u64") for b in range(B)]
        want_w, want_r = cosets(eng, plan, b"".join(pack_scalars(p) for p in polys), n, B)
        want_w, want_r = want_w.raw, want_r.raw
        din = eng.alloc_scalars(N * B, L.FR_MONT)
        din.upload(pack_scalars([e * MONT_R % M.R for p in polys for e in C.fft(p + [0] * (N - n))]))
        dw, dr = dev_buffer(eng, K * B * 96), dev_buffer(eng, N * B * 32)
        cosets(eng, plan, din.ptr, N, B, sfmt=L.FR_MONT, flags=L.IN_DEVICE | L.OUT_DEVICE, out_w=dw, out_r=dr, evals=True)
        assert dev_download(eng, dw, K * B * 96) == want_w
        assert dev_download(eng, dr, N * B * 32) == pack_scalars([v * MONT_R % M.R for v in unpack_scalars(want_r)])
        check_edges(eng, gs, polys, N, l, want_w, want_r, (15, 16, 34), 2, rng)
    finally:
        plan.free()
        if din is not None:
            din.free()
        for p in (dw, dr):
            if p is not None:
                eng.lib.kzg_dev_free(eng.ctx, p)


@pytest.mark.limit(600)
def test_chunk_of_one(eng):
    # (20, 6): one polynomial per chunk, batch 2, with and without interpolants
    rng = random.Random(73)
    log_n, log_l = 20, 6
    N, l = 1 << log_n, 1 << log_l
    K, n, B = N // l, N - 5, 2
    assert F.chunk_size(N) == 1
    gs = kzg_amd.setup(eng, TAU, N, g2_len=0).gs
    try:
        plan = kzg_amd.FK20CosetPlan(eng, gs, log_n, log_l)
        try:
            polys = [rand_scalars(rng, n, kind) for kind in ("u64", "full")]
            blob = b"".join(pack_scalars(p) for p in polys)
            bw, br = cosets(eng, plan, blob, n, B)
            bw, br = bw.raw, br.raw
            wn, rn = cosets(eng, plan, blob, n, B, want_r=False)
            assert rn is None and wn.raw == bw
            for b in range(B):
                w1, r1 = cosets(eng, plan, pack_scalars(polys[b]), n, 1)
                assert w1.raw == bw[b * K * 96:(b + 1) * K * 96] and r1.raw == br[b * N * 32:(b + 1) * N * 32], b
        finally:
            plan.free()
        check_edges(eng, gs, polys, N, l, bw, br, (1,), 2, rng)
    finally:
        gs.free()
