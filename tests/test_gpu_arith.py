"""Device field / curve arithmetic (kzg_amd/csrc/field.h, curve.h as compiled for gfx950) vs the oracle; and kzg_test_arith: every
arithmetic shim of tests/host_math.cpp that has an inline-asm branch on the device, run on the GPU at its limb bounds, compared with
the host build record by record and with big-integer arithmetic."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import arith_vectors as AV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(hooks_engine):  # noqa: F811  the unit-test hooks live in the -DKZG_TEST_HOOKS build of the library, not in the product
    return hooks_engine


def _call(engine, fname, n, *bufs, out_elem):
    out = ctypes.create_string_buffer(n * out_elem)
    f = getattr(engine.lib, fname)
    rc = f(engine.ctx, *bufs, n, out)
    assert rc == 0, engine.last_error()
    return out.raw


def test_fr_fq_mul(engine):
    rng = random.Random(11)
    n = 1000
    Rr, Rq = M.FR_MONT_R, M.FQ_MONT_R
    a = [rng.randrange(M.R) for _ in range(n)]
    b = [rng.randrange(M.R) for _ in range(n)]
    a[:4], b[:4] = [0, M.R - 1, 1, M.R - 1], [5, M.R - 1, 0, 1]
    out = _call(engine, "kzg_test_fr_mul", n, b"".join(x.to_bytes(32, "little") for x in a),
                b"".join(x.to_bytes(32, "little") for x in b), out_elem=32)
    rinv = pow(Rr, -1, M.R)
    for i in range(n):
        assert int.from_bytes(out[32 * i:32 * i + 32], "little") == a[i] * b[i] * rinv % M.R
    a = [rng.randrange(M.Q) for _ in range(n)]
    b = [rng.randrange(M.Q) for _ in range(n)]
    a[:4], b[:4] = [0, M.Q - 1, 1, M.Q - 1], [5, M.Q - 1, 0, 1]
    out = _call(engine, "kzg_test_fq_mul", n, b"".join(x.to_bytes(48, "little") for x in a),
                b"".join(x.to_bytes(48, "little") for x in b), out_elem=48)
    rinv = pow(Rq, -1, M.Q)
    for i in range(n):
        assert int.from_bytes(out[48 * i:48 * i + 48], "little") == a[i] * b[i] * rinv % M.Q


def test_fr_inv(engine):
    rng = random.Random(12)
    n = 300
    Rr = M.FR_MONT_R
    a = [rng.randrange(1, M.R) for _ in range(n)]
    a[0], a[1], a[2] = 1, M.R - 1, 0
    out = ctypes.create_string_buffer(n * 32)
    rc = engine.lib.kzg_test_fr_inv(engine.ctx, b"".join((x * Rr % M.R).to_bytes(32, "little") for x in a), n, out)
    assert rc == 0, engine.last_error()
    for i in range(n):
        want = 0 if a[i] == 0 else pow(a[i], -1, M.R) * Rr % M.R
        assert int.from_bytes(out.raw[32 * i:32 * i + 32], "little") == want


def test_g1_add_edge_cases(engine):
    """P+Q, P+P (doubling branch), P+(-P), inf+P, P+inf, inf+inf -- mixed and general addition."""
    rng = random.Random(13)
    G, INF = C.g1_generator(), bytes(96)
    pts = [C.g1_mul(G, rng.randrange(1, M.R)) for _ in range(20)]
    A, B = [], []
    for i in range(0, 20, 2):
        A.append(pts[i]); B.append(pts[i + 1])
    P = pts[0]
    nP = C.point_to_blob(M.g1_neg(C.blob_to_point(P)))
    A += [P, P, INF, P, INF]
    B += [P, nP, P, INF, INF]
    n = len(A)
    out = _call(engine, "kzg_test_g1_add", n, b"".join(A), b"".join(B), out_elem=96)
    for i in range(n):
        assert out[96 * i:96 * i + 96] == C.g1_add(A[i], B[i]), f"case {i}"


def test_g1_scalar_mul(engine):
    rng = random.Random(14)
    G = C.g1_generator()
    ks = [0, 1, 2, M.R - 1] + [rng.randrange(M.R) for _ in range(28)]
    P = C.g1_mul(G, 123456789)
    n = len(ks)
    out = _call(engine, "kzg_test_g1_mul", n, P * n, b"".join(k.to_bytes(32, "little") for k in ks), out_elem=96)
    for i, k in enumerate(ks):
        assert out[96 * i:96 * i + 96] == C.g1_mul(P, k)


# ---------------------------------------------------------------------------------------------------------------------------------
# kzg_test_arith: the generated inline asm of the three field layers against the portable C of the host build, record by record
# ---------------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREC = 4096 + 45          # records per launch: not a multiple of 64 or 256, so the last wave and the last block are partial
SHAPES = {  # op: (in_rec, out_rec) -- include/kzg_mi355x_test.h
    0: (96, 48), 1: (96, 48), 2: (96, 48), 3: (64, 32), 4: (64, 32), 5: (64, 32),
    6: (104, 52), 7: (52, 52), 8: (208, 52), 9: (156, 52), 10: (104, 52), 11: (156, 52), 12: (156, 52), 13: (52, 52), 14: (52, 48),
    15: (1552, 96), 16: (192, 96), 17: (128, 96),
    18: (64, 32), 19: (100, 64), 20: (68, 108), 21: (1192, 32), 22: (716, 68), 23: (136, 72), 24: (132, 144)}
OPS = ["FQ_MUL", "FQ_ADD", "FQ_SUB", "FR_MUL", "FR_ADD", "FR_SUB", "MUL30", "SQR30", "MULADD30", "MUL30_SUB", "MUL30U", "SQR30_SUB2",
       "SQR30_SUB2U", "NORMALIZE30", "FROM30", "MADD30_CHAIN", "ADD30", "MUL30_SCALAR", "FR29_MUL", "FR29_BUTTERFLIES",
       "FR29_SHOUP_RAW", "FR29_RADIX4_CHAIN", "FR29_QUOTIENT_THREAD", "MULSHOUP29X2", "EMIT"]
INF = bytes(96)


@pytest.fixture(scope="module")
def HL(tmp_path_factory):
    """The host build of tests/host_math.cpp: the portable C branch of the same headers."""
    so = str(tmp_path_factory.mktemp("hm_gpu") / "libhostmath.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "host_math.cpp")])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def pool():
    """Curve points: 12 random multiples of G, their negatives, the identity."""
    rng = random.Random(7070)
    G = C.g1_generator()
    pts = [C.g1_mul(G, rng.randrange(1, M.R)) for _ in range(12)]
    return pts, [C.point_to_blob(M.g1_neg(C.blob_to_point(p))) for p in pts]


def b(x, n):
    return x.to_bytes(n, "little")


def u32s(xs):
    return struct.pack("<%dI" % len(xs), *xs)


def spread(rng, cases):
    """Fills to NREC records by cycling through `cases` (a list of generator functions of one record each: every one recurs, with
    fresh random parts) and shuffles, so that every extreme sits in many lanes, waves and blocks, next to other kinds."""
    recs = [cases[i % len(cases)]() for i in range(NREC)]
    rng.shuffle(recs)
    return recs


def run_op(engine, op, recs):
    """recs: (input bytes, meta) -> device output records."""
    in_rec, out_rec = SHAPES[op]
    assert all(len(r) == in_rec for r, _ in recs)
    out = ctypes.create_string_buffer(len(recs) * out_rec)
    rc = engine.lib.kzg_test_arith(engine.ctx, op, b"".join(r for r, _ in recs), in_rec, len(recs), out, out_rec)
    assert rc == 0, engine.last_error()
    return [out.raw[i * out_rec:(i + 1) * out_rec] for i in range(len(recs))]


def host_op(HL, op, rec):
    """The host shim of `op` on one record: the same bytes the device twin must produce."""
    in_rec, out_rec = SHAPES[op]
    o = ctypes.create_string_buffer(out_rec)
    w = lambda k, n: rec[4 * k: 4 * k + 4 * n]          # noqa: E731  n words from word k
    i32 = lambda k: struct.unpack_from("<i", rec, 4 * k)[0]   # noqa: E731
    sat = {0: (HL.hm_fq_mul, 12), 1: (HL.hm_fq_add, 12), 2: (HL.hm_fq_sub, 12), 3: (HL.hm_fr_mul, 8), 4: (HL.hm_fr_add, 8),
           5: (HL.hm_fr_sub, 8)}
    if op in sat:
        f, n = sat[op]
        f(w(0, n), w(n, n), o)
    elif op in (6, 10):
        (HL.hm_mul30_raw if op == 6 else HL.hm_mul30u_raw)(w(0, 13), w(13, 13), o)
    elif op == 7:
        HL.hm_sqr30_raw(w(0, 13), o)
    elif op == 8:
        HL.hm_muladd30_raw(w(0, 13), w(13, 13), w(26, 13), w(39, 13), o)
    elif op in (9, 11, 12):
        {9: HL.hm_mul30_sub_raw, 11: HL.hm_sqr30_sub2_raw, 12: HL.hm_sqr30_sub2u_raw}[op](w(0, 13), w(13, 13), w(26, 13), o)
    elif op in (13, 14):
        (HL.hm_normalize30_raw if op == 13 else HL.hm_from30_raw)(w(0, 13), o)
    elif op == 15:
        signs = struct.unpack_from("<Q", rec, 8)[0]
        HL.hm_madd30_chain_kernel_form(w(4, 16 * 24), i32(0), ctypes.c_uint64(signs), o)
    elif op == 16:
        HL.hm_add30(w(0, 24), w(24, 24), o)
    elif op == 17:
        HL.hm_mul30_scalar(w(0, 24), w(24, 8), o)
    elif op == 18:
        HL.hm_fr29_mul(w(0, 8), w(8, 8), o)
    elif op == 19:
        ou, ov = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        HL.hm_fr29_butterflies(w(0, 8), w(8, 8), w(16, 8), i32(24), ou, ov)
        return ou.raw + ov.raw
    elif op == 20:
        r, wl, wpl = (ctypes.create_string_buffer(36) for _ in range(3))
        HL.hm_fr29_shoup_raw(w(0, 9), w(9, 8), r, wl, wpl)
        return r.raw + wl.raw + wpl.raw
    elif op == 21:
        HL.hm_fr29_radix4_chain(w(0, 8), w(8, 144), w(152, 144), i32(296), i32(297), o)
    elif op == 22:
        os_, on, top = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), ctypes.c_uint32()
        HL.hm_fr29_quotient_thread(w(0, 64), w(64, 8), w(72, 8), w(80, 90), i32(170), w(171, 8), os_, on, ctypes.byref(top))
        return os_.raw + on.raw + struct.pack("<I", top.value)
    elif op == 23:      # no host twin of the interleaved pair: each half is the host's single Shoup product
        return host_op(HL, 20, rec[:68])[:36] + host_op(HL, 20, rec[68:])[:36]
    elif op == 24:
        HL.hm_emit(w(0, 24), w(24, 8), i32(32), o)
    return o.raw


def check_op(engine, HL, op, recs, invariant):
    """(a) every device record equals the host build's record byte for byte; (b) `invariant(dev_out, meta)` on the device output."""
    dev = run_op(engine, op, recs)
    bad = [i for i, (r, _) in enumerate(recs) if dev[i] != host_op(HL, op, r)]
    assert not bad, "%s: %d of %d device records differ from the host build (first: record %d, meta %r)" % (
        OPS[op], len(bad), len(recs), bad[0], recs[bad[0]][1])
    for i, (_, meta) in enumerate(recs):
        try:
            invariant(dev[i], meta)
        except AssertionError as e:
            raise AssertionError("%s record %d (meta %r): %s" % (OPS[op], i, meta, e)) from None


# ---- saturated Fq / Fr: field.h's add / sub / mul_gfx950 (reduce_once_gfx950 behind add and mul) ---------------------------------
@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5], ids=OPS[:6])
def test_arith_saturated(engine, HL, op):
    rng = random.Random(900 + op)
    p, nl = (M.Q, 12) if op < 3 else (M.R, 8)
    R = 1 << (32 * nl)
    edges = AV.saturated_edges(p, nl)
    pairs = edges + [(rng.randrange(p), rng.randrange(p)) for _ in range(max(0, NREC - len(edges)))]
    rng.shuffle(pairs)
    f = [lambda a, c: a * c * pow(R, -1, p) % p, lambda a, c: (a + c) % p, lambda a, c: (a - c) % p][op % 3]
    recs = [(b(a, 4 * nl) + b(c, 4 * nl), (a, c)) for a, c in pairs]
    assert len(recs) >= 4096 and len(recs) % 64

    def inv(out, meta):
        assert int.from_bytes(out, "little") == f(*meta)
    check_op(engine, HL, op, recs, inv)


# ---- signed 13 x 30-bit Fq: mul30_gfx950.inc ---------------------------------------------------------------------------------------
def _recs30(op, rng):
    K, UK = AV.KINDS30, AV.UKINDS30
    lim, ulim = (lambda k: AV.limbs30(rng, k)), (lambda k: AV.ulimbs30(rng, k))
    raw = lambda *ls: b"".join(AV.raw30(l) for l in ls)    # noqa: E731
    sq = [k for k in K if k != "neg_of_min"]                 # sqr30 doubles its operand: needs the normalised range
    cases = []
    if op == 6:      # balanced x balanced (kind x kind), balanced x unsigned
        for ka in K:
            for kb in K:
                cases.append(lambda ka=ka, kb=kb: (lambda a, c: (raw(a, c), ("bal", a, c)))(lim(ka), lim(kb)))
            for ku in UK:
                cases.append(lambda ka=ka, ku=ku: (lambda a, c: (raw(a, c), ("uns", a, c)))(lim(ka), ulim(ku)))
    elif op == 10:
        cases = [lambda ka=ka, ku=ku: (lambda a, c: (raw(a, c), ("uns", a, c)))(lim(ka), ulim(ku)) for ka in K for ku in UK]
    elif op == 7:
        cases = [lambda ka=ka: (lambda a: (raw(a), a))(lim(ka)) for ka in sq]
    elif op == 8:
        cases = [lambda ka=ka, kb=kb: (lambda a, c, e, f: (raw(a, c, e, f), (a, c, e, f)))(lim(ka), lim(kb), lim(kb), lim(ka))
                 for ka in K for kb in K]
        top = [AV.H30] * 12 + [1 << 20], [-AV.H30] * 12 + [-(1 << 20)]   # same-sign worst case for every column at once
        cases += [lambda: (raw(top[0], top[0], top[0], top[0]), (top[0],) * 4), lambda: (raw(top[0], top[1], top[0], top[1]),
                                                                                         (top[0], top[1], top[0], top[1]))]
    elif op == 9:
        for ka in K:
            for kb in K:
                cases.append(lambda ka=ka, kb=kb: (lambda a, c, u: (raw(a, c, u), ("bal", a, c, u)))(
                    lim(ka), lim(kb), lim(kb if ka == "rnd" else ka)))
            for ku in UK:       # unsigned operand and unsigned subtrahend
                cases.append(lambda ka=ka, ku=ku: (lambda a, c, u: (raw(a, c, u), ("uns", a, c, u)))(lim(ka), ulim(ku), ulim("umax")))
    elif op == 11:
        cases = [lambda ka=ka, kb=kb: (lambda a, u, e: (raw(a, u, e), (a, u, e)))(lim(ka), lim(kb if ka == "rnd" else ka), lim(kb))
                 for ka in sq for kb in K]
    elif op == 12:
        cases = [lambda ka=ka, ku=ku: (lambda a, c, e: (raw(a, c, e), (a, c, e)))(lim(ka), lim(ka), ulim(ku)) for ka in sq for ku in UK]
    elif op == 13:
        # every limb at the largest magnitude whose carry-in keeps it below 3 * 2^29 (normalize30's entry condition)
        edge = [[3 * AV.H30 - 2] * 12 + [(1 << 20) - 1], [-3 * AV.H30 + 2] * 12 + [-(1 << 20)],
                [(3 * AV.H30 - 2) * (1 - 2 * (i & 1)) for i in range(12)] + [0]]
        cases = [lambda: (lambda l: (raw(l), l))(AV.normalize30_input(rng))] * 3 + [lambda e=e: (raw(e), e) for e in edge]
    elif op == 14:
        edge = [0, 1, -1, M.Q - 1, -(M.Q - 1), 255 * M.Q - 1, -(255 * M.Q - 1), 128 * M.Q, -128 * M.Q]
        cases = [lambda: (lambda lx: (raw(lx[0]), lx[1]))(AV.from30_input(rng))] * 3 + \
                [lambda x=x: (raw(AV.balanced30(x)), x) for x in edge]
    return cases


def _inv30(op):
    def inv(out, meta):
        r = AV.unraw30(out) if op != 14 else None
        if op == 6 and meta[0] == "bal":
            a, c = meta[1:]
            AV.check_mont30(r, AV.val30(a) * AV.val30(c), AV.mont30_bound(abs(AV.val30(a) * AV.val30(c))))
        elif op in (6, 10):
            AV.check_mul30_any(r, meta[1], meta[2], unsigned=op == 10)
        elif op == 7:
            AV.check_mont30(r, AV.val30(meta) ** 2, AV.mont30_bound(AV.val30(meta) ** 2))
        elif op == 8:
            a, c, e, f = (AV.val30(x) for x in meta)
            AV.check_mont30(r, a * c + e * f, AV.mont30_bound(abs(a * c) + abs(e * f)))
        elif op == 9:
            kind, a, c, u = meta
            if kind == "bal":
                AV.check_mul30_sub(r, a, c, u)
            else:
                assert AV.is_normalised30(r)
                assert ((AV.val30(r) + AV.val30(u)) * AV.R30 - AV.val30(a) * AV.val30(c)) % M.Q == 0
        elif op in (11, 12):
            AV.check_sqr30_sub2(r, *meta, unsigned=op == 12)
        elif op == 13:
            assert AV.val30(r) == AV.val30(meta) and AV.is_normalised30(r)
        elif op == 14:
            assert int.from_bytes(out, "little") == AV.from30_want(meta)
    return inv


@pytest.mark.parametrize("op", list(range(6, 15)), ids=OPS[6:15])
def test_arith_fq30(engine, HL, op):
    rng = random.Random(3000 + op)
    recs = spread(rng, _recs30(op, rng))
    check_op(engine, HL, op, recs, _inv30(op))


# ---- 30-bit curve chains: k_accum_affine's accumulator form, g1_add30 / g1_dbl30 -------------------------------------------------
def _chain_ref(ps, signs):
    acc = INF
    for i, p in enumerate(ps):
        q = C.point_to_blob(M.g1_neg(C.blob_to_point(p))) if (signs >> i) & 1 and p != INF else p
        acc = C.g1_add(acc, q)
    return acc


def test_arith_madd30_chain(engine, HL, pool):
    """Chains of 1..16 mixed additions, n and the sign mask per record: random chains, doublings (P + P), restarts (P + (-P) makes
    the accumulator the identity, the next point restarts it), identity points anywhere, chains that start at the identity --
    shuffled, so the branches diverge inside every wave."""
    rng = random.Random(1515)
    pts, negs = pool

    def rec(ps, signs):
        body = b"".join(ps) + INF * (16 - len(ps))
        return struct.pack("<IIQ", len(ps), 0, signs) + body, (ps, signs)

    def rnd():
        n = rng.randrange(1, 17)
        ps = [INF if rng.random() < 0.1 else rng.choice(pts) for _ in range(n)]
        return rec(ps, rng.getrandbits(n))

    def dbl():
        P = rng.choice(pts)
        n = rng.randrange(2, 17)
        return rec([P] * n, 0)

    def restart():
        i = rng.randrange(12)
        tail = [rng.choice(pts) for _ in range(rng.randrange(0, 13))]
        return rec([pts[i], pts[i]] + tail, 0b10 | (rng.getrandbits(len(tail)) << 2))   # P + (-P), then a fresh start

    def restart_neg():
        i = rng.randrange(12)
        return rec([pts[i], negs[i], pts[(i + 1) % 12], pts[(i + 1) % 12]], 0)

    def from_inf():
        return rec([INF] * rng.randrange(1, 4) + [rng.choice(pts) for _ in range(rng.randrange(0, 8))], rng.getrandbits(16))

    recs = spread(rng, [rnd, rnd, rnd, dbl, restart, restart_neg, from_inf, lambda: rec([INF], 1), lambda: rec([pts[0]], 1)])
    recs = [(r, (ps, s & ((1 << len(ps)) - 1))) for r, (ps, s) in recs]

    def inv(out, meta):
        assert out == _chain_ref(*meta)
    check_op(engine, HL, 15, recs, inv)


def test_arith_add30_and_mul30_scalar(engine, HL, pool):
    rng = random.Random(1616)
    pts, negs = pool

    def add_case():
        i, j = rng.randrange(12), rng.randrange(12)
        P, Q = pts[i], [pts[j], pts[i], negs[i], INF][rng.randrange(4)]
        if rng.random() < 0.1:
            P = INF
        return P + Q, (P, Q)
    recs = spread(rng, [add_case])

    def inv_add(out, m):
        assert out == C.g1_add(*m)
    check_op(engine, HL, 16, recs, inv_add)

    ks = [0, 1, 2, 3, M.R - 1, M.R - 2, (M.R - 1) // 2, 1 << 254, (1 << 254) - 1]

    def mul_case():
        P = rng.choice(pts)
        k = rng.choice(ks) if rng.random() < 0.2 else rng.randrange(M.R)
        return P + b(k, 32), (P, k)
    recs = spread(rng, [mul_case])

    def inv(out, m):
        assert out == C.g1_mul(*m)
    check_op(engine, HL, 17, recs, inv)


# ---- 9 x 29-bit Fr: mul29r_gfx950.inc (mul29r, mulshoup29, mulshoup29x2) ----------------------------------------------------------
def test_arith_fr29_mul_and_butterflies(engine, HL):
    rng = random.Random(2929)
    R = M.R
    edge = [(0, 5), (AV.R256 - 1, R - 1), (R - 1, R - 1), (1, 0), (AV.R256 - 1, 1), (R, R - 1)]

    def mul_case():
        x = rng.randrange(AV.R256) if rng.random() < 0.6 else rng.randrange(R)
        w = rng.randrange(R)
        if rng.random() < 0.1:
            x, w = rng.choice(edge)
        return b(x, 32) + b(AV.mont_r(w), 32), (x, w)
    recs = spread(rng, [mul_case])

    def inv(out, m):
        assert int.from_bytes(out, "little") == m[0] * m[1] % R
    check_op(engine, HL, 18, recs, inv)

    def bf_case(stages):
        u, v, w = rng.randrange(R), rng.randrange(R), rng.randrange(R)
        if rng.random() < 0.1:
            u, v, w = R - 1, R - 1, R - 1
        return b(u, 32) + b(v, 32) + b(AV.mont_r(w), 32) + struct.pack("<i", stages), (u, v, w, stages)
    recs = spread(rng, [lambda s=s: bf_case(s) for s in range(13)])

    def inv_bf(out, m):
        U, V, w, stages = m
        for _s in range(stages):
            t = V * w % R
            U, V = (U + t) % R, (U - t) % R
        assert (int.from_bytes(out[:32], "little"), int.from_bytes(out[32:], "little")) == (U, V)
    check_op(engine, HL, 19, recs, inv_bf)


def _shoup_in(rng, it):
    w = AV.shoup_twiddle(rng, it)
    raw, x = AV.shoup_operand(rng, it)
    return u32s(raw) + b(AV.mont_r(w), 32), (x, w)


def test_arith_shoup_single_and_interleaved(engine, HL):
    """mulshoup29 on the four operand kinds (every limb at 1.5 * 2^30, values up to 2^261 - 1 ...), and the interleaved
    mulshoup29x2 on two independent pairs with different operands: each half equals the single product of the host build."""
    rng = random.Random(2020)
    it = iter(range(10 ** 9))
    recs = spread(rng, [lambda: _shoup_in(rng, next(it) % 400)])

    def inv(out, m):
        x, w = m
        lim = struct.unpack("<27I", out)
        assert (AV.val29(lim[9:18]), AV.val29(lim[18:])) == AV.shoup_pair(w)
        AV.check_shoup(lim[:9], x, w)
    check_op(engine, HL, 20, recs, inv)

    def pair():
        (r1, m1), (r2, m2) = _shoup_in(rng, next(it) % 400), _shoup_in(rng, next(it) % 400)
        return r1 + r2, (m1, m2)
    recs = spread(rng, [pair])

    def inv2(out, m):
        lim = struct.unpack("<18I", out)
        AV.check_shoup(lim[:9], *m[0])
        AV.check_shoup(lim[9:], *m[1])
    check_op(engine, HL, 23, recs, inv2)


def test_arith_radix4_chain(engine, HL):
    """lds_ntt_stages29's register code, with its mulshoup29x2, along the never-multiplied chain: 0..6 stage pairs, every output."""
    rng = random.Random(4444)

    def case(pairs, which):
        x0, xs, ws = AV.radix4_chain_case(rng, pairs)
        xs_b = b"".join(b(v, 32) for v in xs) + bytes(32 * (18 - len(xs)))
        ws_b = b"".join(b(AV.mont_r(v), 32) for v in ws) + bytes(32 * (18 - len(ws)))
        return b(x0, 32) + xs_b + ws_b + struct.pack("<ii", pairs, which), (x0, xs, ws, pairs, which)
    recs = spread(rng, [lambda p=p, w=w: case(p, w) for p in range(7) for w in range(4)])

    def inv(out, m):
        assert int.from_bytes(out, "little") == AV.radix4_chain_ref(*m)
    check_op(engine, HL, 21, recs, inv)


def test_arith_quotient_thread(engine, HL):
    rng = random.Random(2912)
    it = iter(range(10 ** 9))

    def case():
        a, x, p, m, nbv, a_next = AV.quotient_case(rng, next(it) % 300)
        nb = []
        for v in nbv:
            nb += AV.nb_limbs(v)
        nb += [0] * (90 - len(nb))
        rec = b"".join(b(v, 32) for v in a) + b(AV.mont_r(x), 32) + b(AV.mont_r(p), 32) + u32s(nb) + struct.pack("<i", m) + b(a_next, 32)
        return rec, (a, x, p, nbv, a_next)
    recs = spread(rng, [case])

    def inv(out, m):
        want = AV.quotient_want(*m)
        assert (int.from_bytes(out[:32], "little"), int.from_bytes(out[32:64], "little")) == want
        assert struct.unpack_from("<I", out, 64)[0] < AV.QUOTIENT_TOP_MAX
    check_op(engine, HL, 22, recs, inv)


# ---- emit.h's emit_one on the device, every output format ------------------------------------------------------------------------
def test_arith_emit(engine, HL, pool):
    rng = random.Random(2424)
    pts, _ = pool
    fmts = [(0, 96), (1, 144), (2, 96), (3, 48)]   # affine Montgomery, Jacobian Montgomery, zcash uncompressed / compressed

    def case(fmt):
        P = rng.choice(pts)
        k = rng.choice([0, 1, M.R - 1]) if rng.random() < 0.1 else rng.randrange(M.R)
        return P + b(k, 32) + struct.pack("<i", fmt), (P, k, fmt)
    recs = spread(rng, [lambda f=f: case(f) for f, _ in fmts])
    rinv = pow(M.FQ_MONT_R, -1, M.Q)

    def inv(out, m):
        P, k, fmt = m
        nb = dict(fmts)[fmt]
        assert out[nb:] == bytes(144 - nb)
        want_blob = C.g1_mul(P, k)
        want = C.blob_to_point(want_blob)
        if fmt == 0:
            assert out[:96] == want_blob
        elif fmt == 2:
            assert out[:96] == M.g1_to_uncompressed(want)
        elif fmt == 3:
            assert out[:48] == M.g1_to_compressed(want)
        else:
            X, Y, Z = (int.from_bytes(out[48 * i:48 * i + 48], "little") * rinv % M.Q for i in range(3))
            if want is None:
                assert Z == 0
            else:
                zi = pow(Z, -1, M.Q)
                assert (X * zi * zi % M.Q, Y * zi * zi * zi % M.Q) == want
    check_op(engine, HL, 24, recs, inv)


def test_arith_rejects_bad_shapes(engine):
    """Unknown ops, record sizes of another op, and loop counts outside the documented contract: KZG_ERR_SHAPE, nothing launched."""
    shape_err = 3     # KZG_ERR_SHAPE
    rec = bytes(1552)
    out = ctypes.create_string_buffer(1552)
    for op, in_rec, out_rec in [(-1, 96, 48), (25, 96, 48), (0, 64, 48), (0, 96, 32), (15, 1552, 48), (24, 132, 96)]:
        assert engine.lib.kzg_test_arith(engine.ctx, op, rec, in_rec, 1, out, out_rec) == shape_err, (op, in_rec, out_rec)
    for op, bad in [(15, struct.pack("<I", 0)), (15, struct.pack("<I", 17)), (19, bytes(96) + struct.pack("<i", 13)),
                    (21, bytes(1184) + struct.pack("<ii", 7, 0)), (21, bytes(1184) + struct.pack("<ii", 1, 4)),
                    (22, bytes(680) + struct.pack("<i", 11)), (24, bytes(128) + struct.pack("<i", 9))]:
        r = (bad + bytes(SHAPES[op][0]))[:SHAPES[op][0]]
        assert engine.lib.kzg_test_arith(engine.ctx, op, r, SHAPES[op][0], 1, out, SHAPES[op][1]) == shape_err, op
    assert engine.lib.kzg_test_arith(engine.ctx, 0, rec, 96, 0, out, 48) == shape_err
