"""kzg_ntt_g1 / kzg_ntt_g2 and the G2 Lagrange basis past 1,024 points on the GPU, through the C ABI and the hooks library: the G2
twiddle multiplier value by value (both routes), small transforms against the integer model on inputs that reach the degenerate
additions, 2,048-point transforms with every thread looping over its scratch slot against the known-secret bases,
compute_lagrange_basis_g2 at 2,048 and 4,096, the DFT path against the row-by-row path, batches, chunks and residency, the
evaluation-form verifier end to end, and the refusals."""
import ctypes
import os
import random
import subprocess

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import kzg_model as M
from oracle import pairing_model as PM
from tests import group_ntt_model as G
from tests.fk20_common import dev_buffer, dev_download

pytestmark = pytest.mark.gpu

R, Q = M.R, M.Q
TAU = 0x5EED0F71A5C3
VP, SZ, I32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
G2SZ, G1SZ = L.G2_POINT_BYTES, L.POINT_BYTES
G2ENC = {L.G2_AFFINE_MONT: PM.g2_to_affine_mont, L.G2_JACOBIAN_MONT: PM.g2_to_jacobian_mont, L.G2_UNCOMPRESSED: PM.g2_to_uncompressed,
         L.G2_COMPRESSED: PM.g2_to_compressed}
G1ENC = {L.G1_AFFINE_MONT: M.g1_to_affine_mont, L.G1_ZCASH_UNCOMPRESSED: M.g1_to_uncompressed, L.G1_ZCASH_COMPRESSED: M.g1_to_compressed}


@pytest.fixture(scope="module")
def eng():
    """contexts of this module's own: in the suite's order the file runs behind the tests that close the session's contexts"""
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks():
    from tests.gpu_common import HooksEngine
    h = HooksEngine(0)
    h.lib.kzg_test_g2_mul_gls.argtypes = [VP, VP, VP, SZ, I32, VP]
    h.lib.kzg_test_g2_mul_gls.restype = I32
    yield h
    h.close()


@pytest.fixture
def route(request, eng):
    eng.set_option("g2_ntt_mul", request.param)
    yield request.param
    eng.set_option("g2_ntt_mul", 0)


@pytest.fixture
def looping(eng):
    """256 threads per launch: at 2,048 points every thread loops four times over its scratch slot"""
    eng.set_option("group_ntt_threads", 256)
    yield
    eng.set_option("group_ntt_threads", 0)


def ntt(eng, group, blob, log_n, batch, inverse, pfmt=0, ofmt=0, flags=0, out=None):
    """(rc, bytes): the raw C call, `out` pre-filled with 0xA5 unless given"""
    fn, sizes = (eng.lib.kzg_ntt_g1, G1SZ) if group == 1 else (eng.lib.kzg_ntt_g2, G2SZ)
    n = batch << log_n
    if out is None:
        out = ctypes.create_string_buffer(b"\xa5" * max(n * sizes[ofmt], 1), max(n * sizes[ofmt], 1))
    rc = fn(eng.ctx, blob, log_n, batch, 1 if inverse else 0, pfmt, flags, out, ofmt)
    return rc, out.raw[: n * sizes[ofmt]]


def exp_dft(a, inverse):
    """the transform on exponents: P_j = [a_j] B  ->  out_m = [sum_j a_j w^(+-jm) (/ d)] B"""
    d = len(a)
    w = G.omega(d) if d > 1 else 1
    if inverse:
        w = pow(w, -1, R)
    s = pow(d, -1, R) if inverse else 1
    return [sum(a[j] * pow(w, j * m, R) for j in range(d)) * s % R for m in range(d)]


def inputs(kind, d, rng):
    """exponents of the input points over the generator: random multiples, all points equal, the pattern (P, -P, O, P, ...)"""
    a = rng.randrange(1, R)
    if kind == "random":
        return [rng.randrange(1, R) for _ in range(d)]
    if kind == "equal":
        return [a] * d
    return [(a, R - a, 0, a)[j % 4] for j in range(d)]


class MulCache:
    """[k]B for the model's generator multiples, each computed once for the whole module"""

    def __init__(self, mul, base):
        self.mul, self.base, self.memo = mul, base, {}

    def __call__(self, k):
        k %= R
        if k not in self.memo:
            self.memo[k] = self.mul(self.base, k)
        return self.memo[k]


H_MUL = MulCache(PM.g2_mul, PM.G2)
G_MUL = MulCache(M.g1_mul, M.G1)
SMALL = [(log_n, inverse, kind) for log_n in range(5) for inverse in (False, True) for kind in ("random", "equal", "pattern")]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the multiplier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul_cases():
    rng = random.Random(0x61)
    ks = G.EDGE_SCALARS + [rng.randrange(R) for _ in range(8)]
    s = rng.randrange(2, R)
    cases = [(P, k) for P in (PM.G2, H_MUL(s), None) for k in ks]
    want = b"".join(PM.g2_to_affine_mont(PM.g2_mul(P, k)) for P, k in cases)
    return cases, want


@pytest.mark.parametrize("r", [0, 1])
def test_multiplier_on_edge_scalars(hooks, mul_cases, r):
    cases, want = mul_cases
    pts = b"".join(PM.g2_to_affine_mont(P) for P, _ in cases)
    ks = b"".join(k.to_bytes(32, "little") for _, k in cases)
    out = ctypes.create_string_buffer(192 * len(cases))
    assert hooks.lib.kzg_test_g2_mul_gls(hooks.ctx, pts, ks, len(cases), r, out) == 0, hooks.last_error()
    for i, (P, k) in enumerate(cases):
        assert out.raw[192 * i:192 * (i + 1)] == want[192 * i:192 * (i + 1)], (r, i, hex(k))


# ---------------------------------------------------------------------------------------------------------------------
# 2., 3. small transforms against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1], indirect=True)
@pytest.mark.parametrize("log_n,inverse,kind", SMALL)
def test_g2_small_transforms(eng, route, log_n, inverse, kind):
    a = inputs(kind, 1 << log_n, random.Random(1000 * log_n + 7))  # the same inputs for both routes: one reference
    blob = b"".join(PM.g2_to_affine_mont(H_MUL(k)) for k in a)
    rc, got = ntt(eng, 2, blob, log_n, 1, inverse)
    assert rc == 0, eng.last_error()
    assert got == b"".join(PM.g2_to_affine_mont(H_MUL(k)) for k in exp_dft(a, inverse))


@pytest.mark.parametrize("log_n,inverse,kind", SMALL)
def test_g1_small_transforms(eng, log_n, inverse, kind):
    a = inputs(kind, 1 << log_n, random.Random(1000 * log_n + 9))
    want = [G_MUL(k) for k in exp_dft(a, inverse)]
    for pfmt, ofmt in ((L.G1_AFFINE_MONT, L.G1_AFFINE_MONT), (L.G1_ZCASH_COMPRESSED, L.G1_ZCASH_UNCOMPRESSED)):
        blob = b"".join(G1ENC[pfmt](G_MUL(k)) for k in a)
        rc, got = ntt(eng, 1, blob, log_n, 1, inverse, pfmt, ofmt)
        assert rc == 0, eng.last_error()
        assert got == b"".join(G1ENC[ofmt](P) for P in want), (pfmt, ofmt)


def test_g2_formats_in_and_out(eng):
    a = inputs("pattern", 8, random.Random(3))
    want = [H_MUL(k) for k in exp_dft(a, False)]
    for pfmt, ofmt in ((L.G2_COMPRESSED, L.G2_UNCOMPRESSED), (L.G2_JACOBIAN_MONT, L.G2_COMPRESSED), (L.G2_UNCOMPRESSED, L.G2_JACOBIAN_MONT)):
        rc, got = ntt(eng, 2, b"".join(G2ENC[pfmt](H_MUL(k)) for k in a), 3, 1, False, pfmt, ofmt)
        assert rc == 0, eng.last_error()
        assert got == b"".join(G2ENC[ofmt](P) for P in want), (pfmt, ofmt)


# ---------------------------------------------------------------------------------------------------------------------
# 4. past the old limit, against independent known-secret paths
# ---------------------------------------------------------------------------------------------------------------------
D_BIG = 2048


@pytest.fixture(scope="module")
def known(eng):
    """downloads of setup / setup_lagrange at 2,048 points in both groups"""
    out = {}
    for name, mk in (("hs", kzg_amd.setup_g2), ("lh", kzg_amd.setup_lagrange_g2), ("lg", kzg_amd.setup_lagrange)):
        s = mk(eng, TAU, D_BIG)
        out[name] = s.download()
        s.free()
    p = kzg_amd.setup(eng, TAU, D_BIG, g2_len=0)
    out["gs"] = p.gs.download()
    from_mono = kzg_amd.compute_lagrange_basis(p)
    out["lg_from_mono"] = from_mono.download()
    from_mono.free()
    p.gs.free()
    return out


@pytest.mark.parametrize("route", [0, 1], indirect=True)
def test_g2_2048_points_against_known_secret(eng, looping, known, route):
    rc, inv = ntt(eng, 2, known["hs"], 11, 1, True)
    assert rc == 0, eng.last_error()
    assert inv == known["lh"]
    rc, fwd = ntt(eng, 2, known["lh"], 11, 1, False)
    assert rc == 0 and fwd == known["hs"]
    if route == 0:
        rc, back = ntt(eng, 2, inv, 11, 1, False)
        assert rc == 0 and back == known["hs"]


def test_g1_2048_points_against_known_secret(eng, looping, known):
    rc, inv = ntt(eng, 1, known["gs"], 11, 1, True)
    assert rc == 0, eng.last_error()
    assert inv == known["lg"] and inv == known["lg_from_mono"]
    rc, fwd = ntt(eng, 1, known["lg"], 11, 1, False)
    assert rc == 0 and fwd == known["gs"]
    rc, back = ntt(eng, 1, inv, 11, 1, False)
    assert rc == 0 and back == known["gs"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. compute_lagrange_basis_g2 past 1,024 points (KZG_ERR_SHAPE before this call reached the DFT)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2048, 4096])
def test_lagrange_basis_g2_past_the_old_limit(eng, d):
    params = kzg_amd.setup(eng, TAU, 1, g2_len=d)
    want = kzg_amd.setup_lagrange_g2(eng, TAU, d)
    got = kzg_amd.compute_lagrange_basis_g2(params)
    try:
        assert len(got) == d
        assert got.download() == want.download()
    finally:
        for h in (params.gs, params.hs, want, got):
            h.free()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the DFT path against the row-by-row path
# ---------------------------------------------------------------------------------------------------------------------
def lagrange_at(tau, d):
    """L_i(tau) over the size-d domain: (1/d) sum_j (tau w^-i)^j"""
    w = G.omega(d) if d > 1 else 1
    dinv = pow(d, -1, R)
    return [sum(pow(tau * pow(w, -i, R) % R, j, R) for j in range(d)) * dinv % R for i in range(d)]


@pytest.mark.parametrize("d", [1, 2, 4, 64, 256])
@pytest.mark.parametrize("secret", ["random", "zero", "omega3"])
def test_dft_path_equals_row_path(eng, d, secret):
    w = G.omega(d) if d > 1 else 1
    tau = {"random": TAU, "zero": 0, "omega3": pow(w, 3, R)}[secret]
    want = None
    if secret != "random" and d <= 64:  # what the model expects, computed on the CPU first
        ls = lagrange_at(tau, d)
        assert ls == ([pow(d, -1, R)] * d if secret == "zero" else [1 if i == 3 % d else 0 for i in range(d)])
        want = b"".join(PM.g2_to_affine_mont(H_MUL(k)) for k in ls)
    params = kzg_amd.setup(eng, tau, 1, g2_len=d)
    hs_raw = params.hs.download()
    if secret == "zero" and d > 1:
        assert hs_raw[192:] == bytes(192 * (d - 1))  # hs[1..] are identities
    old = kzg_amd.compute_lagrange_basis_g2(params)
    eng.set_option("g2_lagrange_dft_from", 2)
    try:
        new = kzg_amd.compute_lagrange_basis_g2(params)
    finally:
        eng.set_option("g2_lagrange_dft_from", 2048)
    try:
        a, b = old.download(), new.download()
        assert a == b
        if want is not None:
            assert b == want
        if secret == "omega3" and d >= 4:
            assert b == bytes(192 * 3) + PM.g2_to_affine_mont(PM.G2) + bytes(192 * (d - 4))
        rc, direct = ntt(eng, 2, hs_raw, d.bit_length() - 1, 1, True)
        assert rc == 0 and direct == b
    finally:
        for h in (params.gs, params.hs, old, new):
            h.free()


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch, chunks, residency
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arrays(eng):
    """five arrays of 32 points per group (known-secret powers: valid points without a model)"""
    p = kzg_amd.setup(eng, TAU + 1, 160, g2_len=160)
    out = {1: p.gs.download(), 2: p.hs.download()}
    p.gs.free()
    p.hs.free()
    return out


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("inverse", [False, True])
def test_batch_chunks_and_residency(eng, arrays, group, inverse):
    psz = (G1SZ if group == 1 else G2SZ)[0]
    blob, one = arrays[group], 32 * psz
    singles = []
    for b in range(5):
        rc, got = ntt(eng, group, blob[b * one:(b + 1) * one], 5, 1, inverse)
        assert rc == 0, eng.last_error()
        singles.append(got)
    assert len(set(singles)) == 5
    rc, got = ntt(eng, group, blob[:3 * one], 5, 3, inverse)
    assert rc == 0 and got == b"".join(singles[:3])
    eng.set_option("group_ntt_chunk_points", 64)  # chunks of two arrays: 2 + 2 + 1
    try:
        rc, got = ntt(eng, group, blob, 5, 5, inverse)
        assert rc == 0 and got == b"".join(singles)
        # device in and out, in place, across the same chunks
        dev = dev_buffer(eng, 5 * one)
        assert eng.lib.kzg_dev_upload(eng.ctx, dev, blob, 5 * one) == 0
        fn = eng.lib.kzg_ntt_g1 if group == 1 else eng.lib.kzg_ntt_g2
        assert fn(eng.ctx, dev, 5, 5, 1 if inverse else 0, 0, L.IN_DEVICE | L.OUT_DEVICE, dev, 0) == 0, eng.last_error()
        assert dev_download(eng, dev, 5 * one) == b"".join(singles)
        eng.lib.kzg_dev_free(eng.ctx, dev)
        # a bad point in the LAST chunk: nothing of the first chunks is written
        bad = bytearray(blob)
        bad[4 * one + 5] ^= 1
        rc, got = ntt(eng, group, bytes(bad), 5, 5, inverse)
        assert rc == L.KZG_ERR_BAD_POINT and got == b"\xa5" * (5 * one)
    finally:
        eng.set_option("group_ntt_chunk_points", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 8. end to end: the evaluation-form verifier from a monomial SRS alone
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_form_verifier_from_monomial_srs(eng):
    d = D_BIG
    rng = random.Random(81)
    params = kzg_amd.setup(eng, TAU, d, g2_len=d)
    lag_g, lag_h = kzg_amd.compute_lagrange_basis(params), kzg_amd.compute_lagrange_basis_g2(params)
    ref_g, ref_h = kzg_amd.setup_lagrange(eng, TAU, d), kzg_amd.setup_lagrange_g2(eng, TAU, d)
    try:
        prover = kzg_amd.KZGProverEvalForm(params, lag_g)
        verifier = kzg_amd.KZGVerifierEvalForm(params, lag_g, lag_h)
        known = kzg_amd.KZGVerifierEvalForm(params, ref_g, ref_h)
        evals = kzg_amd.EvaluationDomain.from_coeffs([rng.randrange(R) for _ in range(d)])
        evals.fft(eng)
        c, w = prover.commit(evals), prover.create_witness_all()
        wrong = list(evals.coeffs)
        wrong[d // 3] = (wrong[d // 3] + 1) % R
        assert verifier.verify_eval_all(evals.coeffs, c, w) is True
        assert verifier.verify_eval_all(wrong, c, w) is False
        assert known.verify_eval_all(evals.coeffs, c, w) is True and known.verify_eval_all(wrong, c, w) is False
    finally:
        for h in (params.gs, params.hs, lag_g, lag_h, ref_g, ref_h):
            h.free()


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals: `out` untouched
# ---------------------------------------------------------------------------------------------------------------------
def off_subgroup(group, rng):
    """a point of the curve outside the r-torsion (the cofactor is huge: a random point of the curve is one)"""
    while True:
        if group == 1:
            x = rng.randrange(Q)
            y = pow((x ** 3 + 4) % Q, (Q + 1) // 4, Q)
            if y * y % Q == (x ** 3 + 4) % Q:
                return M.g1_to_affine_mont((x, y))
        else:
            x = (rng.randrange(Q), rng.randrange(Q))
            y = PM.f2_sqrt(PM.f2_add(PM.f2_mul(PM.f2_sqr(x), x), PM.G2_B))
            if y is not None:
                return PM.g2_to_affine_mont((x, y))


@pytest.mark.parametrize("group", [1, 2])
def test_refusals_leave_out_untouched(eng, arrays, group):
    psz = (G1SZ if group == 1 else G2SZ)[0]
    fn = eng.lib.kzg_ntt_g1 if group == 1 else eng.lib.kzg_ntt_g2
    blob = arrays[group][:8 * psz]
    pattern = b"\xa5" * (8 * psz)

    def refused(rc_want, *args, **kw):
        rc, got = ntt(eng, group, *args, **kw)
        assert rc == rc_want, (rc, eng.last_error())
        assert got == pattern[:len(got)]

    out = ctypes.create_string_buffer(pattern, len(pattern))
    assert fn(eng.ctx, blob, 23 if group == 1 else 21, 1, 0, 0, 0, out, 0) == L.KZG_ERR_SHAPE and out.raw == pattern  # over the limit
    refused(L.KZG_ERR_SHAPE, blob, 3, 1, False, pfmt=9)
    assert fn(eng.ctx, blob, 3, 1, 0, 0, 0, out, 9) == L.KZG_ERR_SHAPE and out.raw == pattern  # unknown output format
    assert fn(eng.ctx, None, 3, 1, 0, 0, 0, out, 0) == L.KZG_ERR_SHAPE and out.raw == pattern
    assert fn(eng.ctx, blob, 3, 1, 0, 0, 0, None, 0) == L.KZG_ERR_SHAPE
    assert fn(eng.ctx, None, 3, 0, 0, 0, 0, None, 0) == L.KZG_OK  # batch = 0 is not a refusal
    off_curve = bytearray(blob)
    off_curve[3 * psz + psz // 2] ^= 1  # y of point 3
    refused(L.KZG_ERR_BAD_POINT, bytes(off_curve), 3, 1, False)
    refused(L.KZG_ERR_BAD_POINT, bytes(off_curve), 3, 1, True)
    stray = off_subgroup(group, random.Random(4))
    outside = blob[:5 * psz] + stray + blob[6 * psz:]
    refused(L.KZG_ERR_BAD_POINT, outside, 3, 1, False)
    eng.set_option("trusted_points", 1)  # the curve check alone: the stray point passes, the off-curve one does not
    try:
        refused(L.KZG_ERR_BAD_POINT, bytes(off_curve), 3, 1, False)
        rc, _ = ntt(eng, group, outside, 0, 8, False)  # 8 arrays of one point: a copy, no endomorphism involved
        assert rc == 0
    finally:
        eng.set_option("trusted_points", 0)


def test_srs_conveniences(eng):
    p = kzg_amd.setup(eng, TAU, 16, g2_len=16)
    lg, lh = p.gs.dft(inverse=True), p.hs.dft(inverse=True)
    ref_g, ref_h = kzg_amd.setup_lagrange(eng, TAU, 16), kzg_amd.setup_lagrange_g2(eng, TAU, 16)
    back = lh.dft()
    try:
        assert lg.download() == ref_g.download() and lh.download() == ref_h.download()
        assert back.download() == p.hs.download()
    finally:
        for h in (p.gs, p.hs, lg, lh, ref_g, ref_h, back):
            h.free()


def test_cpp_wrapper(tmp_path):
    """ntt_g1 and ntt_g2 of include/kzg_mi355x.hpp: tests/cpp_group_ntt_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_group_ntt_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_group_ntt_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
