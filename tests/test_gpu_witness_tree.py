"""kzg_verify_eval_tree (kzg_amd/csrc/witness_tree.hip) on the GPU: the verifier of a batched opening at the points of a kzg_point_tree.
Openings are made two ways: by KZGProver.create_witness_batched where that call applies, and under the known secret tau as
C = [s M(tau) + r(tau)]G, w = [s]G for any remainder r and any s -- the equation e(w, [M(tau)]H) == e(C - [r(tau)]G, H) by construction,
through the C oracle's G1 arithmetic, which needs no division and reaches past 16,384 points.
kzg_witness_coeff_tree, the prover on a plan, is checked byte for byte against kzg_witness_coeff_batched where that call applies and
everywhere by the known-tau identity w = [(p(tau) - r(tau)) / M(tau)]G through the C oracle."""
import ctypes
import os
import random
import subprocess
import threading
import time

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import KZGBatchWitness, Polynomial, ReferencePanic
from oracle import c_oracle as C
from oracle import kzg_model as M

pytestmark = pytest.mark.gpu

R = M.R
TAU = 0x7A11_5EED_0123
G = None


def gen():
    global G
    if G is None:
        G = C.g1_generator()
    return G


@pytest.fixture(scope="module")
def engine():  # noqa: F811
    """a context of this module's own: in the suite's order (tests/conftest.py ORDER) the file runs behind the tests that close the
    session's contexts"""
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def params(engine):
    p = kzg_amd.setup(engine, TAU, (1 << 16) + 8, g2_len=(1 << 16) + 2)
    yield p
    p.gs.free()
    p.hs.free()


def horner(cs, x):
    acc = 0
    for c in reversed(cs):
        acc = (acc * x + c) % R
    return acc


def m_at_tau(xs):
    acc = 1
    for x in xs:
        acc = acc * (TAU - x) % R
    return acc


def known_tau_opening(rng, xs, r=None):
    """(commitment, KZGBatchWitness) that verify at xs: r random of len(xs) coefficients unless given"""
    k = len(xs)
    r = [rng.randrange(R) for _ in range(k)] if r is None else r
    s = rng.randrange(1, R)
    c = C.g1_mul(gen(), (s * m_at_tau(xs) + horner(r, TAU)) % R)
    return c, KZGBatchWitness(Polynomial.new_from_coeffs(list(r), k - 1), C.g1_mul(gen(), s))


def bent(w, j=0):
    cs = list(w.r.slice_coeffs())
    cs += [0] * (j + 1 - len(cs))
    cs[j] = (cs[j] + 1) % R
    return KZGBatchWitness(Polynomial.new_from_coeffs(cs, len(cs) - 1), w.w)


@pytest.mark.parametrize("leaf", [0, 4])
@pytest.mark.parametrize("k", [1, 2, 3, 16, 17, 1024, 1025, 5000])
def test_verdicts_at_small_and_medium_k(engine, params, k, leaf):
    rng = random.Random(100 * k + leaf)
    xs = rng.sample(range(1, 1 << 40), k)
    engine.set_option("point_tree_leaf", leaf)
    try:
        tree, shifted = engine.point_tree(xs), engine.point_tree([x + 1 for x in xs])
    finally:
        engine.set_option("point_tree_leaf", 0)
    ver = kzg_amd.KZGVerifier(params)
    try:
        c, w = known_tau_opening(rng, xs)
        c2, w2 = known_tau_opening(rng, xs)
        assert ver.verify_eval_batched_with_tree(tree, c, w)
        tampered_w = KZGBatchWitness(w.r, C.g1_add(w.w, gen()))
        cases = [(c, w), (c, bent(w)), (c, bent(w, k - 1)), (c, tampered_w), (c2, w), (c2, w2)]
        want = [True, False, False, False, False, True]
        got = ver.verify_eval_batched_with_tree_many(tree, [a for a, _ in cases], [b for _, b in cases])
        assert got == want
        assert not ver.verify_eval_batched_with_tree(shifted, c, w)  # a point set shifted by one
        if k >= 2:  # the same verdicts as the reference call, tuple by tuple
            assert [ver.verify_eval_batched(xs, a, b) for a, b in cases] == want
        if 2 <= k <= 1025:  # an opening the engine's own prover made
            n = 2 * k + 1
            p = Polynomial([rng.randrange(R) for _ in range(n)])
            ys = tree.eval(p)
            pw = kzg_amd.KZGProver(params).create_witness_batched(p, xs, ys)
            pc = kzg_amd.KZGProver(params).commit(p)
            assert ver.verify_eval_batched_with_tree(tree, pc, pw)
            assert not ver.verify_eval_batched_with_tree(tree, pc, bent(pw, 1))
            assert not ver.verify_eval_batched_with_tree(tree, c, pw)  # a swapped commitment
    finally:
        tree.close()
        shifted.close()


@pytest.mark.parametrize("k", [16385, (1 << 16) + 1])
def test_past_the_old_limit(engine, params, k):
    rng = random.Random(k)
    xs = rng.sample(range(1, 1 << 48), k)
    tree = engine.point_tree(xs)
    ver = kzg_amd.KZGVerifier(params)
    try:
        c, w = known_tau_opening(rng, xs)
        got = ver.verify_eval_batched_with_tree_many(tree, [c, c, c], [w, bent(w, k // 2), KZGBatchWitness(w.r, C.g1_add(w.w, gen()))])
        assert got == [True, False, False]
        with pytest.raises(ReferencePanic):  # the reference call stops at 16384 points
            ver.verify_eval_batched(xs, c, w)
    finally:
        tree.close()


def raw_call(engine, params, tree, r, c, w, count=1, sfmt=L.FR_CANONICAL, pfmt=L.G1_AFFINE_MONT, ok=None, gs=None, hs=None, plan=True):
    ok = ctypes.create_string_buffer(b"\x77" * max(count, 1), max(count, 1)) if ok is None else ok
    rc = engine.lib.kzg_verify_eval_tree(engine.ctx, (gs or params.gs).handle, (hs or params.hs).handle, tree.handle if plan else None, r, sfmt, c, w,
                                         pfmt, count, ok)
    return rc, ok.raw


def test_formats_count_zero_and_errors_leave_ok_untouched(engine, params):
    rng = random.Random(7)
    k = 9
    xs = rng.sample(range(1, 1 << 30), k)
    tree = engine.point_tree(xs)
    c, w = known_tau_opening(rng, xs)
    r_can = b"".join(v.to_bytes(32, "little") for v in w.r.slice_coeffs()).ljust(32 * k, b"\0")
    r_mont = b"".join((v * (1 << 256) % R).to_bytes(32, "little") for v in w.r.slice_coeffs()).ljust(32 * k, b"\0")
    r_lift = b"".join((v + R).to_bytes(32, "little") for v in w.r.slice_coeffs()).ljust(32 * k, b"\0")  # canonical values >= r count as their residues
    small_hs = kzg_amd.setup_g2(engine, TAU, k)
    small = kzg_amd.setup(engine, TAU, k - 1, g2_len=0)
    twice = engine.point_tree(xs[:-1] + xs[:1])
    try:
        assert raw_call(engine, params, tree, r_can, c, w.w) == (0, b"\x01")
        assert raw_call(engine, params, tree, r_mont, c, w.w, sfmt=L.FR_MONT) == (0, b"\x01")
        assert raw_call(engine, params, tree, r_lift, c, w.w) == (0, b"\x01")
        assert raw_call(engine, params, tree, r_can * 2, c + c, w.w + c, count=2) == (0, b"\x01\x00")
        for pfmt, enc in ((L.G1_ZCASH_UNCOMPRESSED, M.g1_to_uncompressed), (L.G1_ZCASH_COMPRESSED, M.g1_to_compressed)):  # the wire formats
            assert raw_call(engine, params, tree, r_can, enc(model_point(c)), enc(model_point(w.w)), pfmt=pfmt) == (0, b"\x01")
            assert raw_call(engine, params, tree, r_can, enc(model_point(c)), enc(model_point(c)), pfmt=pfmt) == (0, b"\x00")
        assert raw_call(engine, params, tree, r_can, c, w.w, count=0) == (0, b"\x77")
        shape = [dict(sfmt=2), dict(pfmt=L.G1_JACOBIAN_MONT), dict(pfmt=9), dict(hs=small_hs), dict(gs=small.gs), dict(plan=False)]
        for kw in shape:
            assert raw_call(engine, params, tree, r_can, c, w.w, **kw) == (3, b"\x77"), kw
        assert raw_call(engine, params, twice, r_can, c, w.w) == (3, b"\x77")  # repeated points
        for args in [(None, c, w.w), (r_can, None, w.w), (r_can, c, None)]:
            assert raw_call(engine, params, tree, *args) == (3, b"\x77")
            assert raw_call(engine, params, tree, *args, count=0) == (3, b"\x77")  # a NULL buffer is refused at count == 0 too
        assert engine.lib.kzg_verify_eval_tree(engine.ctx, params.gs.handle, params.hs.handle, tree.handle, r_can, L.FR_CANONICAL, c, w.w,
                                               L.G1_AFFINE_MONT, 1, None) == 3
        off = bytearray(c)
        off[0] ^= 1  # not on the curve
        assert raw_call(engine, params, tree, r_can * 2, c + bytes(off), w.w * 2, count=2) == (4, b"\x77\x77")
        assert raw_call(engine, params, tree, r_can * 2, c * 2, w.w + bytes(off), count=2) == (4, b"\x77\x77")
    finally:
        tree.close()
        twice.close()
        small_hs.free()
        small.gs.free()


def model_point(blob):
    """affine Montgomery bytes -> the oracle's (x, y)"""
    inv = pow(M.FQ_MONT_R, -1, M.Q)
    return (int.from_bytes(blob[:48], "little") * inv % M.Q, int.from_bytes(blob[48:], "little") * inv % M.Q)


def test_four_threads_on_one_plan(engine, params):
    rng = random.Random(17)
    xs = rng.sample(range(1, 1 << 30), 300)
    tree = engine.point_tree(xs)
    ver = kzg_amd.KZGVerifier(params)
    c, w = known_tau_opening(rng, xs)
    bad = bent(w, 5)
    errs = []

    def work(i):
        try:
            for _ in range(3):
                assert ver.verify_eval_batched_with_tree_many(tree, [c, c], [w, bad] if i % 2 else [bad, w]) == ([True, False] if i % 2 else [False, True])
        except Exception as e:  # noqa: BLE001
            errs.append((i, repr(e)))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    try:
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs
    finally:
        tree.close()


def test_cpp_wrapper(tmp_path):
    """msm_g2_bucket and PointTree::verify of include/kzg_mi355x.hpp: tests/cpp_witness_tree_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_witness_tree_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_witness_tree_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


@pytest.mark.limit(300)
def test_two_to_the_18_plus_one_points(engine):
    """k = 2^18 + 1 under a known secret: the verifier's verdicts for an honest and a tampered opening.  Measured on an MI355X: see
    DESIGN.md section 3.6b (the whole test, set-up of 2^18 + 2 G2 points and of the plan included)."""
    k = (1 << 18) + 1
    rng = random.Random(18)
    t0 = time.time()
    p = kzg_amd.setup(engine, TAU, k, g2_len=k + 1)
    xs = rng.sample(range(1, 1 << 48), k)
    tree = engine.point_tree(xs)
    try:
        c, w = known_tau_opening(rng, xs)
        t1 = time.time()
        got = kzg_amd.KZGVerifier(p).verify_eval_batched_with_tree_many(tree, [c, c], [w, bent(w, k - 1)])
        t2 = time.time()
        print("k = 2^18 + 1: set-up %.1f s, kzg_verify_eval_tree of two openings %.2f s" % (t1 - t0, t2 - t1))
        assert got == [True, False]
    finally:
        tree.close()
        p.gs.free()
        p.hs.free()


# ---------------------------------------------------------------------------------------------------------------------
# the prover on a plan: kzg_witness_coeff_tree
# ---------------------------------------------------------------------------------------------------------------------
def identity_w(coeffs, r, xs):
    """[(p(tau) - r(tau)) / M(tau)]G by the C oracle (the identity for a zero quotient)"""
    q_tau = (C.poly_eval(coeffs, TAU) - horner(r, TAU)) * M.fr_inv(m_at_tau(xs)) % R
    return C.g1_mul(gen(), q_tau) if q_tau else bytes(96)


@pytest.mark.parametrize("leaf", [0, 4])
@pytest.mark.parametrize("k", [1, 2, 3, 16, 17, 1024, 1025, 5000])
def test_prover_bytes_identity_and_verdicts(engine, params, k, leaf):
    rng = random.Random(7000 * k + leaf)
    xs = rng.sample(range(1, 1 << 40), k)
    engine.set_option("point_tree_leaf", leaf)
    try:
        tree = engine.point_tree(xs)
    finally:
        engine.set_option("point_tree_leaf", 0)
    prover, ver = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    past_pow2 = (1 << (2 * k + 1).bit_length()) + 3  # a size past the next power of two
    try:
        for n in [1, k, k + 1, 2 * k + 1, past_pow2]:
            polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
            polys[1][-1] = 0 if n > 1 else polys[1][-1]  # a polynomial whose top coefficient is zero
            flat = [c for p in polys for c in p]
            ws, rs = tree.create_witness_batch(params.gs, flat, batch=3)
            for b in range(3):
                assert len(rs[b]) == k
                assert ws[b] == identity_w(polys[b], rs[b], xs), (n, b)
                for x in (xs[0], xs[-1]):  # r is the interpolant through the values
                    assert horner(rs[b], x) == horner(polys[b], x), (n, b)
                if n <= k:
                    assert ws[b] == bytes(96) and rs[b] == polys[b] + [0] * (k - n)
            commits = [C.g1_mul(gen(), C.poly_eval(p, TAU)) if C.poly_eval(p, TAU) else bytes(96) for p in polys]
            wits = [KZGBatchWitness(Polynomial(list(rs[b])), ws[b]) for b in range(3)]
            assert ver.verify_eval_batched_with_tree_many(tree, commits, wits) == [True] * 3, n
            if k >= 2 and n > k:  # where the reference call applies: the same bytes, the same verdicts
                for b in (0, 2):
                    poly = Polynomial(list(polys[b]))
                    old = prover.create_witness_batched(poly, xs, tree.eval_batch(polys[b]))
                    assert old.w == ws[b], (n, b)
                    assert (list(old.r.slice_coeffs()) + [0] * k)[:k] == rs[b], (n, b)
                    assert ver.verify_eval_batched(xs, commits[b], wits[b]) is True
    finally:
        tree.close()


def test_claims_status_and_return_code(engine, params):
    rng = random.Random(41)
    k, n = 17, 40
    xs = rng.sample(range(1, 1 << 40), k)
    tree = engine.point_tree(xs)
    try:
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
        flat = [c for p in polys for c in p]
        ys = [v for p in polys for v in tree.eval_batch(p)]
        ws, rs, st = tree.create_witness_batch(params.gs, flat, batch=3, ys=ys, with_status=True)
        assert st == [0, 0, 0]
        assert (ws, rs) == tree.create_witness_batch(params.gs, flat, batch=3, ys=ys) == tree.create_witness_batch(params.gs, flat, batch=3)
        bad = list(ys)
        bad[k + 5] = (bad[k + 5] + 1) % R  # one wrong value in polynomial 1 of 3
        ws2, rs2, st2 = tree.create_witness_batch(params.gs, flat, batch=3, ys=bad, with_status=True)
        assert st2 == [0, L.KZG_ERR_POINT_NOT_ON_POLY, 0] and (ws2, rs2) == (ws, rs)
        with pytest.raises(kzg_amd.api.PointNotOnPolynomial):
            tree.create_witness_batch(params.gs, flat, batch=3, ys=bad)
        # without status: the return code, and every witness and remainder is still written
        out_w, out_r = ctypes.create_string_buffer(b"\x11" * (96 * 3), 96 * 3), ctypes.create_string_buffer(b"\x11" * (32 * 3 * k), 32 * 3 * k)
        rc = engine.lib.kzg_witness_coeff_tree(engine.ctx, params.gs.handle, tree.handle, kzg_amd.api.pack_scalars(flat), n, 3, kzg_amd.api.pack_scalars(bad),
                                               L.FR_CANONICAL, 0, out_w, L.G1_AFFINE_MONT, out_r, None)
        assert rc == L.KZG_ERR_POINT_NOT_ON_POLY
        assert out_w.raw == b"".join(ws) and kzg_amd.api.unpack_scalars(out_r.raw) == [c for r in rs for c in r]
    finally:
        tree.close()


@pytest.mark.parametrize("k", [16385, (1 << 16) + 1])
def test_prover_past_the_old_limit(engine, params, k):
    rng = random.Random(3 * k)
    n = k + 1000
    xs = rng.sample(range(1, 1 << 48), k)
    tree = engine.point_tree(xs)
    try:
        coeffs = [rng.randrange(R) for _ in range(n)]
        ws, rs = tree.create_witness_batch(params.gs, coeffs)
        assert ws[0] == identity_w(coeffs, rs[0], xs)
        wit = KZGBatchWitness(Polynomial(list(rs[0])), ws[0])
        commit = C.g1_mul(gen(), C.poly_eval(coeffs, TAU))
        ver = kzg_amd.KZGVerifier(params)
        assert ver.verify_eval_batched_with_tree_many(tree, [commit, commit], [wit, bent(wit, 7)]) == [True, False]
    finally:
        tree.close()


def test_prover_formats_residency_chunks_and_prefilled_buffers(engine, params):
    rng = random.Random(43)
    k, n, batch = 5, 12, 20  # 20 polynomials: more than one chunk of 16
    xs = rng.sample(range(1, 1 << 40), k)
    tree = engine.point_tree(xs)
    try:
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(batch)]
        flat = [c for p in polys for c in p]
        ws, rs = tree.create_witness_batch(params.gs, flat, batch=batch)
        for b in (0, 15, 16, 19):  # a batch across chunks equals single calls
            w1, r1 = tree.create_witness_batch(params.gs, polys[b])
            assert (w1[0], r1[0]) == (ws[b], rs[b]), b
        can = kzg_amd.api.pack_scalars(flat)
        mont = b"".join((c * (1 << 256) % R).to_bytes(32, "little") for c in flat)
        PAD = 64
        for sfmt, blob in [(L.FR_CANONICAL, can), (L.FR_MONT, mont)]:
            want_r = b"".join((c if sfmt == L.FR_CANONICAL else c * (1 << 256) % R).to_bytes(32, "little") for r in rs for c in r)
            for ofmt, enc in [(L.G1_AFFINE_MONT, lambda w: w), (L.G1_ZCASH_COMPRESSED, lambda w: M.g1_to_compressed(model_point(w)))]:
                psz = L.POINT_BYTES[ofmt]
                want_w = b"".join(enc(w) for w in ws)
                for in_dev in (False, True):
                    for out_dev in (False, True):
                        flags = (L.IN_DEVICE if in_dev else 0) | (L.OUT_DEVICE if out_dev else 0)
                        src = engine.alloc_scalars(batch * n, sfmt).upload(blob) if in_dev else None
                        if out_dev:
                            dw, dr = engine.alloc_scalars(batch * 3 + 2), engine.alloc_scalars(batch * k + 2)
                            dw.upload(b"\xa5" * dw.n * 32)
                            dr.upload(b"\xa5" * dr.n * 32)
                            ow, orr = dw.ptr, dr.ptr
                        else:
                            ow = ctypes.create_string_buffer(b"\xa5" * (psz * batch + PAD), psz * batch + PAD)
                            orr = ctypes.create_string_buffer(b"\xa5" * (32 * batch * k + PAD), 32 * batch * k + PAD)
                        rc = engine.lib.kzg_witness_coeff_tree(engine.ctx, params.gs.handle, tree.handle, src.ptr if in_dev else blob, n, batch, None, sfmt,
                                                               flags, ow, ofmt, orr, None)
                        assert rc == 0, (sfmt, ofmt, flags, engine.last_error())
                        gw = dw.download()[:psz * batch + PAD] if out_dev else ow.raw
                        gr = dr.download()[:32 * batch * k + PAD] if out_dev else orr.raw
                        assert gw[:psz * batch] == want_w and gr[:32 * batch * k] == want_r, (sfmt, ofmt, flags)
                        assert gw[psz * batch:] == b"\xa5" * PAD and gr[32 * batch * k:] == b"\xa5" * PAD, (sfmt, ofmt, flags)
                        for buf in ([src] if in_dev else []) + ([dw, dr] if out_dev else []):
                            buf.free()
    finally:
        tree.close()


def test_prover_refusals_leave_the_outputs_untouched(engine, params):
    rng = random.Random(47)
    k, n = 6, 15
    xs = rng.sample(range(1, 1 << 40), k)
    tree, twice = engine.point_tree(xs), engine.point_tree(xs[:-1] + xs[:1])
    small = kzg_amd.setup(engine, TAU, 8, g2_len=0)
    blob = kzg_amd.api.pack_scalars([rng.randrange(R) for _ in range(2 * n)])
    fill_w, fill_r = b"\x3c" * 192, b"\x3c" * (64 * k)

    def call(plan=tree, gs=params.gs, coeffs=blob, n_=n, batch=2, sfmt=L.FR_CANONICAL, ofmt=L.G1_AFFINE_MONT, w=True):
        ow, orr = ctypes.create_string_buffer(fill_w, 192), ctypes.create_string_buffer(fill_r, 64 * k)
        st = (ctypes.c_int * 2)(9, 9)
        rc = engine.lib.kzg_witness_coeff_tree(engine.ctx, gs.handle if gs else None, plan.handle if plan else None, coeffs, n_, batch, None, sfmt, 0,
                                               ow if w else None, ofmt, orr, st)
        return rc, ow.raw == fill_w and orr.raw == fill_r and list(st) == [9, 9]
    try:
        assert call()[0] == 0
        for kw in [dict(plan=twice), dict(n_=0), dict(n_=(1 << 27) + 1), dict(sfmt=2), dict(ofmt=9), dict(coeffs=None), dict(w=False), dict(plan=None),
                   dict(gs=None), dict(gs=small.gs)]:  # (small: 15 - 6 = 9 quotient coefficients against 8 points)
            assert call(**kw) == (3, True), kw
        assert call(batch=0) == (0, True)
    finally:
        tree.close()
        twice.close()
        small.gs.free()


def test_prover_four_threads_on_one_plan(engine, params):
    rng = random.Random(53)
    k, n = 33, 100
    xs = rng.sample(range(1, 1 << 40), k)
    tree = engine.point_tree(xs)
    polys = [[rng.randrange(R) for _ in range(2 * n)] for _ in range(4)]
    want = [tree.create_witness_batch(params.gs, p, batch=2) for p in polys]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                assert tree.create_witness_batch(params.gs, polys[i], batch=2) == want[i]
        except Exception as e:  # noqa: BLE001
            errs.append((i, repr(e)))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    try:
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs
    finally:
        tree.close()


def test_prover_python_mirrors(engine, params):
    rng = random.Random(59)
    prover, ver = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    poly = Polynomial([rng.randrange(R) for _ in range(9)])
    for k in (3, 1):
        xs = rng.sample(range(1, 1 << 40), k)
        tree = engine.point_tree(xs)
        try:
            ys = [poly.eval(engine, x) for x in xs]
            got, old = prover.create_witness_batched_with_tree(poly, tree, ys), prover.create_witness_batched(poly, xs, ys)
            assert got.w == old.w and got.r.slice_coeffs() == old.r.slice_coeffs() and got.r.degree == old.r.degree, k
            if k > 1:
                assert ver.verify_eval_batched_with_tree(tree, prover.commit(poly), got)
            with pytest.raises(kzg_amd.api.PointNotOnPolynomial):
                prover.create_witness_batched_with_tree(poly, tree, [(ys[0] + 1) % R] + ys[1:])
            with pytest.raises(ReferencePanic):
                prover.create_witness_batched_with_tree(poly, tree, ys + [1])
        finally:
            tree.close()


@pytest.mark.limit(300)
def test_prover_and_verifier_at_two_to_the_18_plus_one_points_of_a_2_20_polynomial(engine):
    """k = 2^18 + 1, n = 2^20, known secret: the prover's identity w = [(p(tau) - r(tau)) / M(tau)]G by the C oracle and the verifier's
    verdict on the prover's output.  Measured on an MI355X: DESIGN.md section 3.6b."""
    k, n = (1 << 18) + 1, 1 << 20
    rng = random.Random(20)
    t0 = time.time()
    p = kzg_amd.setup(engine, TAU, n, g2_len=k + 1)
    xs = rng.sample(range(1, 1 << 48), k)
    tree = engine.point_tree(xs)
    buf = engine.alloc_scalars(n).fill_random(2020)
    try:
        blob = buf.download()
        t1 = time.time()
        ws, rs = tree.create_witness_batch(p.gs, buf)
        t2 = time.time()
        p_tau = C.poly_eval_bytes(blob, n, TAU)
        q_tau = (p_tau - horner(rs[0], TAU)) * M.fr_inv(m_at_tau(xs)) % R
        assert ws[0] == C.g1_mul(gen(), q_tau)
        wit = KZGBatchWitness(Polynomial(list(rs[0])), ws[0])
        commit = C.g1_mul(gen(), p_tau)
        t3 = time.time()
        got = kzg_amd.KZGVerifier(p).verify_eval_batched_with_tree_many(tree, [commit, commit], [wit, bent(wit, k - 1)])
        t4 = time.time()
        print("k = 2^18 + 1, n = 2^20: set-up %.1f s, kzg_witness_coeff_tree %.2f s (r to host lists), kzg_verify_eval_tree of two %.2f s"
              % (t1 - t0, t2 - t1, t4 - t3))
        assert got == [True, False]
    finally:
        buf.free()
        tree.close()
        p.gs.free()
        p.hs.free()
