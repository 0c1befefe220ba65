"""-m gpu parity tests of the verifier half through the C ABI: G2 parameters, G2 multi-exponentiation, pairing
checks and KZGVerifier / KZGVerifierEvalForm (src/coeff_form.rs:114-183, src/eval_form.rs:149-218), against the
python oracle (oracle/pairing_model.py).  The scenarios restate the reference's own verifier tests
(src/coeff_form.rs:279-400) with a known tau."""
import ctypes
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M, pairing_model as P

pytestmark = pytest.mark.gpu


def g1b(p):  # affine Montgomery 96 B
    return M.g1_to_affine_mont(p)


def random_polynomial(rng, min_coeffs, max_coeffs):  # src/coeff_form.rs:207-219
    num = rng.randrange(min_coeffs, max_coeffs)
    coeffs = [0] * max_coeffs
    for i in range(num):
        coeffs[i] = rng.getrandbits(64)
    return kzg_amd.Polynomial(coeffs)


def test_setup_g2_matches_oracle_in_every_format(engine):
    tau = 0x1234567
    hs = kzg_amd.setup_g2(engine, tau, 5)
    want = P.setup_g2(tau, 5)
    assert len(hs) == 5
    assert hs.download() == b"".join(P.g2_to_affine_mont(p) for p in want)
    assert hs.download(pfmt=L.G2_JACOBIAN_MONT) == b"".join(P.g2_to_jacobian_mont(p) for p in want)
    assert hs.download(pfmt=L.G2_UNCOMPRESSED) == b"".join(P.g2_to_uncompressed(p) for p in want)
    assert hs.download(1, 3, pfmt=L.G2_COMPRESSED) == b"".join(P.g2_to_compressed(p) for p in want[1:4])
    # upload round trips (incl. the identity) in every format
    pts = want + [None, P.g2_neg(want[2])]
    enc = {L.G2_AFFINE_MONT: P.g2_to_affine_mont, L.G2_JACOBIAN_MONT: P.g2_to_jacobian_mont,
           L.G2_UNCOMPRESSED: P.g2_to_uncompressed, L.G2_COMPRESSED: P.g2_to_compressed}
    for fmt, f in enc.items():
        up = kzg_amd.SrsG2.upload(engine, b"".join(f(p) for p in pts), len(pts), fmt)
        assert up.download(pfmt=L.G2_UNCOMPRESSED) == b"".join(P.g2_to_uncompressed(p) for p in pts), fmt
        up.free()
    # a point off the twist / a non-residue x are rejected
    bad = bytearray(P.g2_to_uncompressed(want[1]))
    bad[-1] ^= 1
    with pytest.raises(kzg_amd.EngineError):
        kzg_amd.SrsG2.upload(engine, bytes(bad), 1, L.G2_UNCOMPRESSED)
    x = (5, 0)
    while P.f2_sqrt(P.f2_add(P.f2_mul(P.f2_sqr(x), x), P.G2_B)) is not None:
        x = (x[0] + 1, 0)
    badc = bytearray(x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    badc[0] |= 0x80
    with pytest.raises(kzg_amd.EngineError):
        kzg_amd.SrsG2.upload(engine, bytes(badc), 1, L.G2_COMPRESSED)
    hs.free()


def test_msm_g2_matches_oracle(engine):
    rng = random.Random(5)
    tau = rng.getrandbits(64)
    hs = kzg_amd.setup_g2(engine, tau, 70)
    want = P.setup_g2(tau, 70)
    for n, off in [(1, 0), (2, 3), (70, 0), (33, 37), (0, 0)]:
        sc = [rng.randrange(M.R) for _ in range(n)]
        if n > 2:
            sc[0], sc[1] = 0, M.R - 1
        got = hs.msm(sc, offset=off, ofmt=L.G2_UNCOMPRESSED)
        assert got == P.g2_to_uncompressed(P.g2_multi_exp(want[off:off + n], sc)), (n, off)
    with pytest.raises(kzg_amd.ReferencePanic):
        hs.msm([1] * 5, offset=68)
    hs.free()


def test_pairing_check_matches_oracle(engine):
    rng = random.Random(6)
    a, b = rng.randrange(M.R), rng.randrange(M.R)
    Pa, Qb = M.g1_mul(M.G1, a), P.g2_mul(P.G2, b)
    neg_ab = M.g1_neg(M.g1_mul(M.G1, a * b % M.R))
    wrong = M.g1_neg(M.g1_mul(M.G1, (a * b + 1) % M.R))
    checks = [[(Pa, Qb), (neg_ab, P.G2)],        # e(aG, bH) e(-abG, H) = 1
              [(Pa, Qb), (wrong, P.G2)],         # off by one
              [(None, Qb), (Pa, None)],          # identity members contribute 1
              [(M.G1, P.G2), (M.g1_neg(M.G1), P.G2)],
              [(M.G1, P.G2), (M.G1, P.G2)]]
    g1 = b"".join(g1b(p) for c in checks for p, _ in c)
    g2 = b"".join(P.g2_to_affine_mont(q) for c in checks for _, q in c)
    ok = ctypes.create_string_buffer(len(checks))
    rc = engine.lib.kzg_pairing_check(engine.ctx, g1, L.G1_AFFINE_MONT, g2, L.G2_AFFINE_MONT, 2, len(checks), ok)
    assert rc == 0, engine.last_error()
    want = [P.pairing_product_is_one(c) for c in checks]
    assert [bool(x) for x in ok.raw] == want == [True, False, True, True, False]
    # three- and four-pair products, zcash encodings
    c3 = [(Pa, Qb), (M.g1_mul(M.G1, 7), P.g2_mul(P.G2, 9)), (M.g1_neg(M.g1_mul(M.G1, (a * b + 63) % M.R)), P.G2)]
    ok = ctypes.create_string_buffer(1)
    rc = engine.lib.kzg_pairing_check(engine.ctx, b"".join(M.g1_to_compressed(p) for p, _ in c3), L.G1_ZCASH_COMPRESSED,
                                      b"".join(P.g2_to_compressed(q) for _, q in c3), L.G2_COMPRESSED, 3, 1, ok)
    assert rc == 0 and ok.raw == b"\x01"


def test_verify_eval_reference_scenarios(engine):  # test_eval_basic (src/coeff_form.rs:317-342)
    rng = random.Random(69)
    tau = rng.getrandbits(64)
    params = kzg_amd.setup(engine, tau, 13)
    prover, verifier = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    p = random_polynomial(rng, 5, 13)
    c = prover.commit(p)
    x = rng.getrandbits(64)
    y = p.eval(engine, x)
    w = prover.create_witness(p, (x, y))
    assert verifier.verify_eval((x, y), c, w)
    assert not verifier.verify_eval((x, (y + 12345) % M.R), c, w)
    assert not verifier.verify_eval(((x + 1) % M.R, y), c, w)
    # the oracle's verifier agrees on both
    op = P.setup(tau, 13)
    ov = P.KZGVerifier(op)
    cP, wP = M.g1_from_uncompressed(prover.commit(p, ofmt=L.G1_ZCASH_UNCOMPRESSED)), \
        M.g1_from_uncompressed(prover.create_witness(p, (x, y), ofmt=L.G1_ZCASH_UNCOMPRESSED))
    assert ov.verify_eval((x, y), cP, wP) and not ov.verify_eval((x, (y + 12345) % M.R), cP, wP)
    # degree-1 edge case: p = 3 + X at (1, 4)
    p1 = kzg_amd.Polynomial([3, 1] + [0] * 11)
    c1 = prover.commit(p1)
    w1 = prover.create_witness(p1, (1, 4))
    assert verifier.verify_eval((1, 4), c1, w1)
    assert not verifier.verify_eval((1, 5), c1, w1)
    # many openings in one launch, mixed verdicts, zcash-compressed inputs; a constant polynomial's witness is the identity
    pc = kzg_amd.Polynomial([42] + [0] * 12)
    cc, wc = prover.commit(pc), prover.create_witness(pc, (9, 42))
    assert wc == bytes(96)
    pts = [(x, y), (x, (y + 1) % M.R), (1, 4), (9, 42), (9, 43)]
    got = verifier.verify_eval_many(pts, [c, c, c1, cc, cc], [w, w, w1, wc, wc])
    assert got == [True, False, True, True, False]
    comp = lambda blob: M.g1_to_compressed(M.g1_from_uncompressed(blob))  # noqa: E731
    cz = prover.commit(p, ofmt=L.G1_ZCASH_UNCOMPRESSED)
    wz = prover.create_witness(p, (x, y), ofmt=L.G1_ZCASH_UNCOMPRESSED)
    assert verifier.verify_eval((x, y), comp(cz), comp(wz), pfmt=L.G1_ZCASH_COMPRESSED)
    params.gs.free()
    params.hs.free()


def test_verify_eval_batched_reference_scenarios(engine):  # test_eval_batched{,_all_points} (:344-399)
    rng = random.Random(70)
    tau = rng.getrandbits(64)
    params = kzg_amd.setup(engine, tau, 15)
    prover, verifier = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    p = random_polynomial(rng, 8, 15)
    c = prover.commit(p)
    xs = [rng.getrandbits(64) for _ in range(8)]
    ys = [p.eval(engine, x) for x in xs]
    w = prover.create_witness_batched(p, xs, ys)
    assert verifier.verify_eval_batched(xs, c, w)
    xs2 = [rng.getrandbits(64) for _ in range(8)]
    assert not verifier.verify_eval_batched(xs2, c, w)
    # oracle verdicts on the same data
    ov = P.KZGVerifier(P.setup(tau, 15))
    cP = M.g1_from_uncompressed(prover.commit(p, ofmt=L.G1_ZCASH_UNCOMPRESSED))
    wP = M.g1_from_uncompressed(prover.create_witness_batched(p, xs, ys, ofmt=L.G1_ZCASH_UNCOMPRESSED).w)
    rP = M.Polynomial.new_from_coeffs(list(w.r.coeffs), w.r.degree)
    assert ov.verify_eval_batched(xs, cP, wP, rP) and not ov.verify_eval_batched(xs2, cP, wP, rP)
    # all points: as many openings as coefficients
    p2 = random_polynomial(rng, 13, 14)
    c2 = prover.commit(p2)
    xs = [rng.getrandbits(64) for _ in range(p2.num_coeffs())]
    ys = [p2.eval(engine, x) for x in xs]
    w2 = prover.create_witness_batched(p2, xs, ys)
    assert verifier.verify_eval_batched(xs, c2, w2)
    # one point: the reference's interpolant quirk (r = X + (y - x)) still verifies, as it does upstream
    w1 = prover.create_witness_batched(p, xs[:1], [p.eval(engine, xs[0])])
    rP1 = M.Polynomial.new_from_coeffs(list(w1.r.coeffs), w1.r.degree)
    got = verifier.verify_eval_batched(xs[:1], c, w1)
    assert got == ov.verify_eval_batched(xs[:1], cP, M.g1_from_uncompressed(
        prover.create_witness_batched(p, xs[:1], [p.eval(engine, xs[0])], ofmt=L.G1_ZCASH_UNCOMPRESSED).w), rP1)
    # more points than hs holds -> the reference's slice panic
    small = kzg_amd.setup(engine, tau, 15, g2_len=4)
    with pytest.raises(kzg_amd.ReferencePanic):
        kzg_amd.KZGVerifier(small).verify_eval_batched(xs2, c, w)
    for prm in (params, small):
        prm.gs.free()
        prm.hs.free()


def test_eval_form_verifier(engine):  # src/eval_form.rs:173-217
    rng = random.Random(71)
    tau = rng.getrandbits(64)
    d = 16
    params = kzg_amd.setup(engine, tau, d)
    lag_g = kzg_amd.setup_lagrange(engine, tau, d)
    lag_h = kzg_amd.setup_lagrange_g2(engine, tau, d)
    want_h = P.lagrange_basis_g2_known_tau(tau, d)
    assert lag_h.download(pfmt=L.G2_UNCOMPRESSED) == b"".join(P.g2_to_uncompressed(p) for p in want_h)
    # compute_lagrange_basis from hs alone (src/eval_form.rs:254-280) yields the same elements
    full = kzg_amd.setup(engine, tau, d, g2_len=d)
    from_hs = kzg_amd.compute_lagrange_basis_g2(full)
    assert from_hs.download() == lag_h.download()
    for h in (full.gs, full.hs, from_hs):
        h.free()
    prover = kzg_amd.KZGProverEvalForm(params, lag_g)
    verifier = kzg_amd.KZGVerifierEvalForm(params, lag_g, lag_h)
    coeffs = [rng.getrandbits(64) for _ in range(d)]
    evals = kzg_amd.EvaluationDomain.from_coeffs(coeffs)
    evals.fft(engine)
    c = prover.commit(evals)
    for i in (0, 5, d - 1):
        w = prover.create_witness(evals, i)
        y = evals.coeffs[i]
        assert verifier.verify_eval((i, y), c, w)
        assert not verifier.verify_eval((i, (y + 1) % M.R), c, w)
        assert not verifier.verify_eval(((i + 1) % d, y), c, w)
    # verify_eval_all exactly as written upstream: the oracle restates the same formula
    ov = P.KZGVerifierEvalForm(P.setup(tau, d), M.lagrange_basis_g1_known_tau(tau, d), want_h)
    cP = M.g1_from_uncompressed(prover.commit(evals, ofmt=L.G1_ZCASH_UNCOMPRESSED))
    for wit in (prover.create_witness_all(), prover.create_witness(evals, 3)):
        wP = None if wit == bytes(96) else \
            M.g1_from_uncompressed(prover.create_witness(evals, 3, ofmt=L.G1_ZCASH_UNCOMPRESSED))
        assert verifier.verify_eval_all(evals.coeffs, c, wit) == ov.verify_eval_all(evals.coeffs, cP, wP)
    for h in (params.gs, params.hs, lag_g, lag_h):
        h.free()


def test_verify_eval_degenerate_secret(engine):
    """tau = 0: hs[1] (and gs[1..]) are the identity -- the stored-lines path must treat the pair as 1, like the oracle."""
    params = kzg_amd.setup(engine, 0, 6)
    assert params.hs.download(1, 1) == bytes(192)
    prover, verifier = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    p = kzg_amd.Polynomial([7, 3, 9, 1, 0, 0])
    c = prover.commit(p)
    assert c == g1b(M.g1_mul(M.G1, 7))
    x, y = 5, p.eval(engine, 5)
    w = prover.create_witness(p, (x, y))
    op = P.setup(0, 6, fast=False)
    ov = P.KZGVerifier(op)
    cP = M.g1_mul(M.G1, 7)
    wP = M.KZGProver(op).create_witness(M.Polynomial([7, 3, 9, 1, 0, 0]), (x, y))
    assert w == g1b(wP)
    for pt in [(x, y), (x, (y + 1) % M.R), (0, 7), (0, 8)]:
        assert verifier.verify_eval(pt, c, w) == ov.verify_eval(pt, cP, wP), pt
    params.gs.free()
    params.hs.free()


def test_batched_opening_5000_points_prover_and_verifier(engine):
    """create_witness_batched + verify_eval_batched (src/coeff_form.rs:83-111, :144-182) with 5000 opening points -- above the 4096 the
    interpolation kernels took until round 4 (limit now 16384).  The witness against the known-tau identity with p(tau), I(tau) by the
    oracle; the interpolant at sampled opening points; the pairing check accepts it and rejects a shifted point set."""
    rng = random.Random(71)
    tau = rng.getrandbits(64)
    n, k = 6000, 5000
    params = kzg_amd.setup(engine, tau, n, g2_len=k + 1)
    prover, verifier = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    coeffs = [rng.randrange(M.R) for _ in range(n)]
    p = kzg_amd.Polynomial(coeffs)
    c = prover.commit(p)
    xs = [rng.randrange(M.R) for _ in range(k)]
    ys = [C.poly_eval(coeffs, x) for x in xs]
    w = prover.create_witness_batched(p, xs, ys)
    I = list(w.r.coeffs)
    assert len(I) == k and all(C.poly_eval(I, xs[i]) == ys[i] for i in range(0, k, 499))
    Z = 1
    for x in xs:
        Z = Z * (tau - x) % M.R
    assert w.w == C.g1_mul(C.g1_generator(), (C.poly_eval(coeffs, tau) - C.poly_eval(I, tau)) * pow(Z, -1, M.R) % M.R)
    assert verifier.verify_eval_batched(xs, c, w)
    assert not verifier.verify_eval_batched([(x + 1) % M.R for x in xs], c, w)
    ys[1234] = (ys[1234] + 1) % M.R
    with pytest.raises(kzg_amd.PointNotOnPolynomial):
        prover.create_witness_batched(p, xs, ys)
    params.gs.free()
    params.hs.free()


# ---------------------------------------------------------------------------------------------------------------------
# Verdicts by the wave.  Every point below is a known multiple of a generator ([a]G, [b]H) under a known tau, so every verdict has an
# exact integer reference that needs no pairing:  prod e([a_i]G, [b_i]H) = 1  <=>  sum a_i b_i = 0 (mod r), the identity being the
# multiple 0.  A handful of records per test (at most 12) also go through the python oracle's verifier, which keeps the integer
# reference honest.  The classes are shuffled with a fixed seed so that every wave of 64 threads mixes them.
# ---------------------------------------------------------------------------------------------------------------------
R = M.R
TAU = 0x5eed0123456789abcdef0fedcba9876543210 % R
_G1 = {}


def g1k(a):
    """[a]G as affine Montgomery 96 B (the identity for a = 0 mod r)"""
    a %= R
    if a not in _G1:
        _G1[a] = bytes(96) if a == 0 else C.g1_mul(C.g1_generator(), a)
    return _G1[a]


def g1_enc(a, pfmt):
    return g1k(a) if pfmt == L.G1_AFFINE_MONT else M.g1_to_compressed(C.blob_to_point(g1k(a)))


def g1_pt(a):
    return C.blob_to_point(g1k(a))


def fr_enc(xs, sfmt):
    return b"".join(((x % R) * (M.FR_MONT_R if sfmt == L.FR_MONT else 1) % R).to_bytes(32, "little") for x in xs)


@pytest.fixture(scope="module")
def g2_pool():
    """[(b, [b]H)]: a few G2 multiples shared by every check (the model's G2 scalar multiplication is the slow part); b = r - 1 last"""
    rng = random.Random(80)
    bs = [1] + [rng.randrange(2, R - 1) for _ in range(4)] + [R - 1]
    return [(b, P.g2_mul(P.G2, b)) for b in bs]


PAIRING_CLASSES = ["balanced", "off by one", "identity P", "identity Q", "all identity", "next to its negation", "b = r - 1"]


def pairing_check_case(rng, cls, np_, pool):
    """-> [(a_i, index into pool or None for the identity Q)] of one check of np_ pairs"""
    nb = len(pool)

    def balance(pairs, free):
        """solves the a of pair `free` so that the live exponents cancel"""
        s = sum(a * pool[j][0] for i, (a, j) in enumerate(pairs) if i != free and j is not None)
        pairs[free] = (-s * pow(pool[pairs[free][1]][0], -1, R) % R, pairs[free][1])

    pairs = [(rng.randrange(1, R), rng.randrange(nb)) for _ in range(np_)]
    if cls == "b = r - 1":
        pairs = [(a, nb - 1) for a, _ in pairs]
    if cls == "next to its negation" and np_ >= 2:
        pairs[1] = (R - pairs[0][0], pairs[0][1])
        if np_ == 4:
            balance(pairs, 3)
        return pairs
    if cls == "all identity":
        return [(0, j) if rng.random() < 0.5 else (a, None) for a, j in pairs]
    if np_ >= 2:
        balance(pairs, np_ - 1)
    if cls == "off by one":
        pairs[-1] = ((pairs[-1][0] + 1) % R, pairs[-1][1])
    if cls in ("identity P", "identity Q"):
        k = rng.randrange(np_)
        pairs[k] = (0, pairs[k][1]) if cls == "identity P" else (pairs[k][0], None)
        live = [i for i in range(np_) if i != k]
        if len(live) >= 2 and rng.random() < 0.5:      # the rest balanced again: a true verdict with a skipped pair
            balance(pairs, live[-1])
    return pairs


@pytest.mark.parametrize("np_", [1, 2, 3, 4])
def test_pairing_check_by_the_wave(engine, g2_pool, np_):
    """kzg_pairing_check with 64 + 9 checks of np_ pairs: one full block and a partial one, the classes mixed inside every wave; in
    affine Montgomery and in zcash compressed form.  For np_ = 1 a check is true exactly when a member is the identity."""
    rng = random.Random(81 + np_)
    checks = 64 + 9
    classes = [PAIRING_CLASSES[i % len(PAIRING_CLASSES)] for i in range(checks)]
    rng.shuffle(classes)
    cases = [pairing_check_case(rng, cls, np_, g2_pool) for cls in classes]
    want = [sum(a * g2_pool[j][0] for a, j in c if j is not None) % R == 0 for c in cases]
    assert True in want and False in want
    if np_ == 1:
        assert want == [a == 0 or j is None for c in cases for a, j in c]
    q = lambda j: None if j is None else g2_pool[j][1]  # noqa: E731
    # the integer reference against the oracle's pairing on a few records of both verdicts
    sample = [want.index(True), want.index(False), checks - 1, 64]
    for i in sample:
        assert P.pairing_product_is_one([(g1_pt(a), q(j)) for a, j in cases[i]]) == want[i], (i, classes[i])
    for pfmt1, pfmt2, enc2 in [(L.G1_AFFINE_MONT, L.G2_AFFINE_MONT, P.g2_to_affine_mont), (L.G1_ZCASH_COMPRESSED, L.G2_COMPRESSED, P.g2_to_compressed)]:
        g1 = b"".join(g1_enc(a, pfmt1) for c in cases for a, _ in c)
        g2 = b"".join(enc2(q(j)) for c in cases for _, j in c)
        ok = ctypes.create_string_buffer(checks)
        rc = engine.lib.kzg_pairing_check(engine.ctx, g1, pfmt1, g2, pfmt2, np_, checks, ok)
        assert rc == 0, engine.last_error()
        got = [bool(x) for x in ok.raw]
        wrong = [(i, classes[i], got[i], want[i]) for i in range(checks) if got[i] != want[i]]
        assert not wrong, (pfmt1, wrong)


def verify_eval_records(rng, tau, count):
    """-> (classes, [(c, v, x, y)]): C = [c]G, w = [v]G; the opening verifies exactly when c - y = v (tau - x) (mod r)"""
    names = ["valid", "c off by one", "v off by one", "x off by one", "y off by one", "c and y off by one", "constant polynomial",
             "zero polynomial", "C = O, v != 0, true", "C = O, v != 0, false", "x = 0", "x = r - 1", "y = 0", "y = r - 1",
             "x = tau, c = y", "x = tau, c != y"]
    classes = [names[i % len(names)] for i in range(count)]
    rng.shuffle(classes)
    recs = []
    for cls in classes:
        v, x, y = rng.randrange(1, R), rng.randrange(R), rng.randrange(R)
        if cls == "x = 0":
            x = 0
        elif cls == "x = r - 1":
            x = R - 1
        elif cls == "y = 0":
            y = 0
        elif cls == "y = r - 1":
            y = R - 1
        elif cls.startswith("x = tau"):
            x = tau
        elif cls in ("constant polynomial", "zero polynomial"):
            v = 0
        c = (y + v * (tau - x)) % R
        if cls == "c off by one":
            c = (c + 1) % R
        elif cls == "v off by one":
            v = (v + 1) % R
        elif cls == "x off by one":
            x = (x + 1) % R
        elif cls == "y off by one":
            y = (y + 1) % R
        elif cls == "c and y off by one":
            c, y = (c + 1) % R, (y + 1) % R
        elif cls == "zero polynomial":
            c, y = 0, 0
        elif cls == "C = O, v != 0, true":
            c, y = 0, (-v * (tau - x)) % R
        elif cls == "C = O, v != 0, false":
            c = 0
        elif cls == "x = tau, c != y":
            c = (y + 1 + rng.randrange(R - 1)) % R
        recs.append((c, v, x, y))
    return classes, recs


@pytest.mark.parametrize("tau,count", [(TAU, 2 * 64 + 7), (0, 64 + 3)])
def test_verify_eval_by_the_wave(engine, tau, count):
    """kzg_verify_eval: two full blocks and a partial one in one call (one and a partial one for tau = 0, where hs[1] is the identity
    and its stored lines must never be read), every class in every wave: lanes that skip an identity pair next to lanes that do not.
    Both scalar formats, affine Montgomery and compressed points."""
    rng = random.Random(82)
    classes, recs = verify_eval_records(rng, tau, count)
    want = [(c - y - v * (tau - x)) % R == 0 for c, v, x, y in recs]
    by_class = {}
    for cls, w in zip(classes, want):
        by_class.setdefault(cls, set()).add(w)
    false_classes = {"c off by one", "v off by one", "x off by one", "y off by one", "C = O, v != 0, false", "x = tau, c != y"}
    assert len(by_class) == 16 and all(by_class[cls] == {cls not in false_classes} for cls in by_class), by_class
    params = kzg_amd.setup(engine, tau, 4)
    if tau == 0:
        assert params.hs.download(1, 1) == bytes(192)
    ov = P.KZGVerifier(P.setup(tau, 2, fast=bool(tau)))
    for i in [want.index(True), want.index(False)] + [classes.index(n) for n in ("constant polynomial", "x = tau, c = y", "C = O, v != 0, true", "y off by one")]:
        c, v, x, y = recs[i]
        assert ov.verify_eval((x, y), g1_pt(c), g1_pt(v)) == want[i], (i, classes[i])
    for sfmt in (L.FR_CANONICAL, L.FR_MONT):
        for pfmt in (L.G1_AFFINE_MONT, L.G1_ZCASH_COMPRESSED):
            ok = ctypes.create_string_buffer(count)
            rc = engine.lib.kzg_verify_eval(engine.ctx, params.gs.handle, params.hs.handle, fr_enc([r[2] for r in recs], sfmt),
                                            fr_enc([r[3] for r in recs], sfmt), sfmt, b"".join(g1_enc(r[0], pfmt) for r in recs),
                                            b"".join(g1_enc(r[1], pfmt) for r in recs), pfmt, count, ok)
            assert rc == 0, engine.last_error()
            got = [bool(b) for b in ok.raw]
            wrong = [(i, classes[i], got[i], want[i]) for i in range(count) if got[i] != want[i]]
            assert not wrong, (sfmt, pfmt, wrong)
    params.gs.free()
    params.hs.free()


@pytest.fixture(scope="module")
def batched_params(engine):
    params = kzg_amd.setup(engine, TAU, 16)
    yield params
    params.gs.free()
    params.hs.free()


@pytest.mark.parametrize("sfmt", [L.FR_CANONICAL, L.FR_MONT])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_verify_eval_batched_integer_reference(engine, batched_params, k, sfmt):
    """kzg_verify_eval_batched (k_verify_finish: hz on the fly next to the stored lines of h0): C = [c]G, w = [v]G, any r; true exactly
    when v z(tau) = c - r(tau) with z = prod (X - x_i)."""
    rng = random.Random(83 + k)

    def poly_at_tau(coeffs):
        return sum(a * pow(TAU, j, R) for j, a in enumerate(coeffs)) % R

    def z_at_tau(xs):
        z = 1
        for x in xs:
            z = z * (TAU - x) % R
        return z

    records = []   # (label, c, v, xs, r)
    xs = [rng.randrange(R) for _ in range(k)]
    v = rng.randrange(1, R)
    for r_len in sorted({0, 1, k}):
        r = [rng.randrange(1, R) for _ in range(r_len)]
        records.append(("valid, r_len %d" % r_len, (v * z_at_tau(xs) + poly_at_tau(r)) % R, v, xs, r))
    _, c, v, xs, r = records[-1]                                    # r_len = k
    i = rng.randrange(k)
    records += [("c off by one", (c + 1) % R, v, xs, r), ("v off by one", c, (v + 1) % R, xs, r),
                ("x_%d off by one" % i, c, v, xs[:i] + [(xs[i] + 1) % R] + xs[i + 1:], r),
                ("r_%d off by one" % i, c, v, xs, r[:i] + [(r[i] + 1) % R] + r[i + 1:])]
    xt = xs[:i] + [TAU] + xs[i + 1:]                                # z(tau) = 0: hz is the identity
    records += [("x_%d = tau, c = r(tau)" % i, poly_at_tau(r), v, xt, r), ("x_%d = tau, c != r(tau)" % i, (poly_at_tau(r) + 1) % R, v, xt, r)]
    records += [("w = O, c = r(tau)", poly_at_tau(r), 0, xs, r), ("w = O, c != r(tau)", c, 0, xs, r)]
    want = [(v_ * z_at_tau(x_) - c_ + poly_at_tau(r_)) % R == 0 for _, c_, v_, x_, r_ in records]
    n_valid = len({0, 1, k})
    assert want == [True] * n_valid + [False] * 4 + [True, False, True, False]
    if sfmt == L.FR_CANONICAL:      # the integer reference against the oracle's verifier (one true and one false record)
        ov = P.KZGVerifier(P.setup(TAU, k + 1))
        for j in (n_valid - 1, n_valid + 2):
            _, c_, v_, x_, r_ = records[j]
            assert ov.verify_eval_batched(x_, g1_pt(c_), g1_pt(v_), M.Polynomial.new_from_coeffs(list(r_), len(r_) - 1)) == want[j], records[j][0]
    for (label, c_, v_, x_, r_), w in zip(records, want):
        ok = ctypes.c_int(-1)
        rc = engine.lib.kzg_verify_eval_batched(engine.ctx, batched_params.gs.handle, batched_params.hs.handle, fr_enc(x_, sfmt), k,
                                                fr_enc(r_, sfmt), len(r_), sfmt, g1k(c_), g1k(v_), L.G1_AFFINE_MONT, ctypes.byref(ok))
        assert rc == 0, engine.last_error()
        assert ok.value == int(w), (label, k, sfmt)


@pytest.mark.parametrize("d", [1, 2, 16])
def test_verify_eval_all_integer_reference(engine, d):
    """kzg_verify_eval_all with the formula exactly as written upstream (z has -1 at index 0 and +1 at index d - 1; for d = 1 the later
    write wins): true exactly when v (L_{d-1}(tau) - L_0(tau)) = c - sum_{i < ys_len} y_i L_i(tau).  Expected from the oracle's
    KZGVerifierEvalForm.verify_eval_all and from the integer identity."""
    rng = random.Random(84 + d)
    _, _, omega = M.compute_omega(d)
    lag = [(pow(TAU, d, R) - 1) * pow(omega, i, R) % R * pow(d * (TAU - pow(omega, i, R)), -1, R) % R for i in range(d)]
    assert sum(lag) % R == 1
    zs = 1 if d == 1 else (lag[d - 1] - lag[0]) % R
    gr = lambda ys: sum(y * l for y, l in zip(ys, lag)) % R  # noqa: E731
    v = rng.randrange(1, R)
    ys = [rng.randrange(1, R) for _ in range(d)]
    c = (v * zs + gr(ys)) % R
    i = rng.randrange(d)
    records = [("valid, ys_len 0", v * zs % R, v, []), ("valid, ys_len d", c, v, ys), ("c off by one", (c + 1) % R, v, ys),
               ("v off by one", c, (v + 1) % R, ys), ("y_%d off by one" % i, c, v, ys[:i] + [(ys[i] + 1) % R] + ys[i + 1:]),
               ("w = O, c = gr", gr(ys), 0, ys), ("w = O, c != gr", c, 0, ys), ("w = O, ys_len 0, C = O", 0, 0, [])]
    want = [(v_ * zs - c_ + gr(y_)) % R == 0 for _, c_, v_, y_ in records]
    assert want == [True, True, False, False, False, True, False, True]
    params = kzg_amd.setup(engine, TAU, d)
    lag_g = kzg_amd.setup_lagrange(engine, TAU, d)
    lag_h = kzg_amd.setup_lagrange_g2(engine, TAU, d)
    ov = P.KZGVerifierEvalForm(P.setup(TAU, d), M.lagrange_basis_g1_known_tau(TAU, d), P.lagrange_basis_g2_known_tau(TAU, d))
    for j in (1, 3, 5):
        _, c_, v_, y_ = records[j]
        assert ov.verify_eval_all(y_, g1_pt(c_), g1_pt(v_)) == want[j], records[j][0]
    for sfmt in (L.FR_CANONICAL, L.FR_MONT):
        for (label, c_, v_, y_), w in zip(records, want):
            ok = ctypes.c_int(-1)
            rc = engine.lib.kzg_verify_eval_all(engine.ctx, lag_g.handle, lag_h.handle, params.hs.handle, fr_enc(y_, sfmt), len(y_), sfmt,
                                                g1k(c_), g1k(v_), L.G1_AFFINE_MONT, ctypes.byref(ok))
            assert rc == 0, engine.last_error()
            assert ok.value == int(w), (label, d, sfmt)
    for h in (params.gs, params.hs, lag_g, lag_h):
        h.free()
