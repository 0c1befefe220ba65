"""kzg_poly_divide on the GPU, through the C ABI via kzg_amd.  Every expected value comes from oracle.kzg_model
(Polynomial.long_division), from oracle.c_oracle.long_division above a few hundred coefficients, or from kzg_quotient_linear /
kzg_poly_eval (the parity and identity tests), never from the call under test, and every comparison is equality of integers or
bytes."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import ReferencePanic, pack_scalars, unpack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import poly_divide_model as PD
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
SH = L.KZG_ERR_SHAPE
A5 = b"\xa5"
PAD = 64  # bytes behind every output that must stay 0xA5
B0 = PD.DEFAULT_BASE
SHAPES = [(1, 1), (5, 1), (1, 2), (2, 2), (3, 2), (9, 2), (4, 5), (8, 8), (9, 8), (10, 8), (17, 9), (33, 17), (40, 33), (300, 200),
          (257, 2), (256, 129), (520, 257), (521, 258), (1000, 3)]
# m = na - nb + 1 one below, at and one above the default base precision; nb - 1 one below, at and one above a power of two;
# (10, 2): m = 9, four and two Newton levels with a truncated last one under base 1 and 4
SHAPES += [(B0 + 1, 3), (B0 + 2, 3), (B0 + 3, 3), (2 * B0 + 9, 10), (10, 2), (40, 16), (40, 17), (40, 18), (90, 64), (90, 65), (90, 66)]
BASES = [0, 1, 4]


def le(v):
    return int(v).to_bytes(32, "little")


def encode(vals, sfmt):
    """ints below 2^256 as the call reads them: canonical bytes as they are (a value >= r counts as its residue); Montgomery: the
    representative of the residue, plus r where the value was given as >= r and that still fits 256 bits"""
    if sfmt == CAN:
        return b"".join(le(v) for v in vals)
    out = []
    for v in vals:
        x = (v % R) * MONT_R % R
        out.append(le(x + R if v >= R and x + R < 1 << 256 else x))
    return b"".join(out)


def decode(raw, sfmt):
    vals = unpack_scalars(raw)
    assert all(v < R for v in vals), "an output is not the residue below r"
    return [v * pow(MONT_R, -1, R) % R for v in vals] if sfmt == MONT else vals


def reference(a, b):
    """the reference's quotient and remainder zero-padded to na - nb + 1 and nb - 1 coefficients, and its None"""
    na, nb = len(a), len(b)
    if na < nb:
        r = [x % R for x in a] + [0] * (nb - 1 - na)
        return [], r, not any(r)
    q, r = M.Polynomial(a).long_division(M.Polynomial(b))
    qc = q.coeffs[: q.degree + 1]
    rc = [] if r is None else r.coeffs[: r.degree + 1]
    return qc + [0] * (na - nb + 1 - len(qc)), rc + [0] * (nb - 1 - len(rc)), r is None


def case(na, nb, seed=0):
    rng = random.Random(1000 * na + nb + seed)
    return [rng.randrange(R) for _ in range(na)], [rng.randrange(R) for _ in range(nb - 1)] + [rng.randrange(1, R)]


def divide(eng, a, na, batch, b, sfmt=CAN, in_dev=False, out_dev=False, want_q=True, want_r=True, want_exact=True):
    """the C call with host / device inputs in `sfmt` and host / device outputs prefilled with 0xA5 -> (q, r, exact) as flat lists of
    ints (None for an output that was not asked for); nothing may be written behind the batch x m and batch x (nb - 1) scalars"""
    nb = len(b)
    m, nr = (na - nb + 1 if na >= nb else 0), nb - 1
    ab, bb = encode(a, sfmt), encode(b, sfmt)
    assert len(ab) == 32 * na * batch
    flags, srcs = 0, []
    pa, pb = ab, bb
    if in_dev:
        pa, pb = dev_buffer(eng, len(ab)), dev_buffer(eng, len(bb))
        assert eng.lib.kzg_dev_upload(eng.ctx, pa, ab, len(ab)) == 0 and eng.lib.kzg_dev_upload(eng.ctx, pb, bb, len(bb)) == 0
        srcs = [pa, pb]
        flags |= L.IN_DEVICE
    qn, rn = 32 * batch * m + PAD, 32 * batch * nr + PAD
    if out_dev:
        pq, pr = dev_buffer(eng, qn), dev_buffer(eng, rn)
        flags |= L.OUT_DEVICE
    else:
        pq, pr = ctypes.create_string_buffer(A5 * qn, qn), ctypes.create_string_buffer(A5 * rn, rn)
    ex = (ctypes.c_int * (batch + 1))(*([-7] * (batch + 1)))
    rc = eng.lib.kzg_poly_divide(eng.ctx, pa, na, batch, pb, nb, sfmt, flags, pq if want_q else None, pr if want_r else None,
                                 ex if want_exact else None)
    assert rc == 0, eng.last_error()
    qraw = dev_download(eng, pq, qn) if out_dev else pq.raw
    rraw = dev_download(eng, pr, rn) if out_dev else pr.raw
    for p in srcs + ([pq, pr] if out_dev else []):
        eng.lib.kzg_dev_free(eng.ctx, p)
    assert qraw[qn - PAD:] == A5 * PAD and rraw[rn - PAD:] == A5 * PAD
    if not want_q:
        assert qraw == A5 * qn
    if not want_r:
        assert rraw == A5 * rn
    assert ex[batch] == -7 and (want_exact or list(ex) == [-7] * (batch + 1))
    return (decode(qraw[: qn - PAD], sfmt) if want_q else None, decode(rraw[: rn - PAD], sfmt) if want_r else None,
            [bool(v) for v in ex[:batch]] if want_exact else None)


def with_base(eng, base, fn):
    eng.set_option("poly_divide_base", base)
    try:
        return fn()
    finally:
        eng.set_option("poly_divide_base", 0)


_REF = {}


def shape_case(na, nb):
    if (na, nb) not in _REF:
        a, b = case(na, nb)
        _REF[(na, nb)] = (a, b, reference(a, b))
    return _REF[(na, nb)]


@pytest.mark.parametrize("sfmt", [CAN, MONT])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("na,nb", SHAPES)
def test_shapes_against_the_oracle(eng, na, nb, base, sfmt):
    a, b, want = shape_case(na, nb)
    assert with_base(eng, base, lambda: divide(eng, a, na, 1, b, sfmt)) == (want[0], want[1], [want[2]])


@pytest.mark.parametrize("sfmt", [CAN, MONT])
@pytest.mark.parametrize("na,nb", [(40, 9), (20, 14)])  # m > nb and nb > m
def test_divisor_and_dividend_patterns(eng, na, nb, sfmt):
    rng = random.Random(na * nb)
    a, b = case(na, nb, 7)
    divisors = {
        "b0_zero": [0] + b[1:],
        "sparse": [(-5) % R] + [0] * (nb - 2) + [1],            # X^k - c
        "monic": b[:-1] + [1],
        "non_monic": b[:-1] + [R - 2],
        "above_r": [x + R if x + R < 1 << 256 else x for x in b],
    }
    dividends = {
        "random": a,
        "top_two_zero": a[:-2] + [0, 0],
        "zero": [0] * na,
        "above_r": [x + R if x + R < 1 << 256 else x for x in a],
        "all_ones_256": [(1 << 256) - 1] * na,
        "tiny": [rng.randrange(3) for _ in range(na)],
    }
    for dn, d in divisors.items():
        for an, x in dividends.items():
            want = reference(x, d)
            for base in BASES:
                got = with_base(eng, base, lambda: divide(eng, x, na, 1, d, sfmt))
                assert got == (want[0], want[1], [want[2]]), (dn, an, base)
    assert divide(eng, [0] * na, na, 1, b, sfmt)[2] == [True]   # the zero dividend: the reference's None


@pytest.mark.parametrize("nq,nb", [(23, 12), (5, 30), (100, 2)])
def test_exact_divisions_and_one_perturbed_coefficient(eng, nq, nb):
    q0, b = case(nq, nb, 3)
    a = M.Polynomial(q0).mul_naive(M.Polynomial(b)).coeffs
    na = len(a)
    assert PD.divide(a, b)[0] == q0
    for sfmt in (CAN, MONT):
        assert divide(eng, a, na, 1, b, sfmt) == (q0, [0] * (nb - 1), [True])
        assert divide(eng, a, na, 1, b, sfmt, want_r=False) == (q0, None, [True])       # exact does not need r_out
    for pos in (0, nb - 2, na - 1):
        a2 = list(a)
        a2[pos] = (a2[pos] + 1) % R
        want = reference(a2, b)
        assert not want[2]
        assert divide(eng, a2, na, 1, b) == (want[0], want[1], [False])
        assert divide(eng, a2, na, 1, b, want_r=False) == (want[0], None, [False])
        assert divide(eng, a2, na, 1, b, want_q=False) == (None, want[1], [False])


@pytest.mark.parametrize("n", [2, 9, 257, 5000])
def test_linear_divisors_equal_quotient_linear_and_poly_eval(eng, n):
    rng = random.Random(n)
    p, x = [rng.randrange(R) for _ in range(n)], rng.randrange(R)
    blob = pack_scalars(p)
    y = ctypes.create_string_buffer(32)
    assert eng.lib.kzg_poly_eval(eng.ctx, blob, n, le(x), CAN, 0, y) == 0
    ql = ctypes.create_string_buffer(32 * (n - 1))
    assert eng.lib.kzg_quotient_linear(eng.ctx, blob, n, le(x), y.raw, CAN, 0, ql) == 0, eng.last_error()
    q, r = ctypes.create_string_buffer(32 * (n - 1)), ctypes.create_string_buffer(32)
    ex = (ctypes.c_int * 1)(-7)
    assert eng.lib.kzg_poly_divide(eng.ctx, blob, n, 1, pack_scalars([-x, 1]), 2, CAN, 0, q, r, ex) == 0, eng.last_error()
    assert q.raw == ql.raw and r.raw == y.raw
    assert ex[0] == (1 if y.raw == bytes(32) else 0)


def test_a_batch_of_three_equals_three_lone_calls(eng):
    na, nb = 70, 9
    a, b = case(3 * na, nb, 11)
    a[na - 1] = 0                                 # dividend 0: top coefficient zero
    a[2 * na - 5:2 * na] = [0] * 5                # dividend 1: the top five
    a[2 * na:3 * na] = [0] * na                   # dividend 2: zero
    lone = [divide(eng, a[i * na:(i + 1) * na], na, 1, b) for i in range(3)]
    for i in range(3):
        want = reference(a[i * na:(i + 1) * na], b)
        assert lone[i] == (want[0], want[1], [want[2]])
    for sfmt in (CAN, MONT):
        for in_dev in (False, True):
            for out_dev in (False, True):
                got = divide(eng, a, na, 3, b, sfmt, in_dev, out_dev)
                assert got[0] == sum((l[0] for l in lone), []) and got[1] == sum((l[1] for l in lone), []), (sfmt, in_dev, out_dev)
                assert got[2] == [False, False, True]


@pytest.mark.parametrize("na,nb,batch", [(9, 4, 260), (3, 5, 258), (1 << 13, 100, 130)])  # chunks of 256, 256 and 128 dividends
def test_a_batch_that_spans_two_chunks(eng, na, nb, batch):
    rng = random.Random(batch)
    a, b = [rng.randrange(R) for _ in range(na * batch)], case(na, nb)[1]
    for in_dev, out_dev in ((False, False), (True, True)):
        q, r, ex = divide(eng, a, na, batch, b, CAN, in_dev, out_dev)
        m, nr = max(na - nb + 1, 0), nb - 1
        for i in (0, 1, batch // 2 - 1, batch // 2, batch - 2, batch - 1) if na > 100 else range(batch):
            ai = a[i * na:(i + 1) * na]
            want = (C.long_division(ai, b) + (False,)) if na > 100 else reference(ai, b)
            assert (q[i * m:(i + 1) * m], r[i * nr:(i + 1) * nr], ex[i]) == (want[0], want[1], want[2]), i
        lone = divide(eng, a[(batch - 1) * na:], na, 1, b)
        assert (q[(batch - 1) * m:], r[(batch - 1) * nr:], ex[batch - 1:]) == lone


@pytest.mark.parametrize("sfmt", [CAN, MONT])
@pytest.mark.parametrize("na,nb", [(33, 17), (300, 20), (5, 8)])
def test_flag_combinations_and_single_outputs(eng, na, nb, sfmt):
    a, b = case(na, nb, 5)
    want = reference(a, b)
    for in_dev in (False, True):
        for out_dev in (False, True):
            assert divide(eng, a, na, 1, b, sfmt, in_dev, out_dev) == (want[0], want[1], [want[2]])
            assert divide(eng, a, na, 1, b, sfmt, in_dev, out_dev, want_exact=False) == (want[0], want[1], None)
            if na >= nb:
                assert divide(eng, a, na, 1, b, sfmt, in_dev, out_dev, want_r=False) == (want[0], None, [want[2]])
            assert divide(eng, a, na, 1, b, sfmt, in_dev, out_dev, want_q=False) == (None, want[1], [want[2]])


def test_python_surface(eng):
    a, b = case(50, 7, 9)
    want = reference(a, b)
    assert eng.poly_divide(a, b) == (want[0], want[1], [want[2]])
    a3 = a + case(50, 7, 10)[0] + [0] * 50
    q, r, ex = eng.poly_divide(a3, b, batch=3)
    assert (q[0], r[0], ex[0]) == want and q[2] == [0] * 44 and r[2] == [0] * 6 and ex == [False, False, True]
    for sfmt in (CAN, MONT):
        buf = kzg_amd.DeviceBuffer(eng, 150, sfmt).upload(encode(a3, sfmt))
        qo, ro = kzg_amd.DeviceBuffer(eng, 132, sfmt), kzg_amd.DeviceBuffer(eng, 18, sfmt)
        try:
            assert eng.poly_divide(buf, b, batch=3) == (q, r, ex)
            got = eng.poly_divide(buf, b, batch=3, q_out=qo, r_out=ro)
            assert got[0] is qo and got[1] is ro and got[2] == ex
            assert decode(qo.download(), sfmt) == sum(q, []) and decode(ro.download(), sfmt) == sum(r, [])
            with pytest.raises(ReferencePanic):
                eng.poly_divide(buf, b, batch=4)
        finally:
            for d in (buf, qo, ro):
                d.free()
    P = kzg_amd.api.Polynomial
    quo, rem = P(a).long_division(eng, P(b))
    assert (quo.coeffs, quo.degree) == (want[0], 43) and (rem.coeffs, rem.degree) == (want[1], 5)
    prod = M.Polynomial(a).mul_naive(M.Polynomial(b)).coeffs
    quo, rem = P(prod + [0, 0]).long_division(eng, P(b + [0]))           # slice_coeffs on both sides
    assert (quo.coeffs, quo.degree, rem) == (a, 49, None)
    quo, rem = P([5] + prod[1:]).long_division(eng, P(b))                # a remainder of degree 0: its degree is fixed up
    assert rem.degree == 0 and rem.coeffs == [(5 - prod[0]) % R] + [0] * 5


def larger_case(na, nb):
    """(2^16 + 3, 257): random coefficients.  (2^16, 2^15 + 1): the oracle's loop takes 2^30 field products on random coefficients
    (most of a minute); it skips the quotient coefficients that are zero, so the dividend there is a = q0 b + r0 with a random divisor and
    remainder and 32 non-zero quotient coefficients, the lowest and the highest among them -- every coefficient of a is still a
    random-looking residue, and the call under test does the same work whatever the values."""
    if nb <= 257:
        return case(na, nb)
    rng = random.Random(na + nb)
    b = case(na, nb)[1]
    m = na - nb + 1
    a = [rng.randrange(R) for _ in range(nb - 1)] + [0] * m
    for p in [0, m - 1] + rng.sample(range(1, m - 1), 30):
        c = rng.randrange(1, R)
        for j, x in enumerate(b):
            a[p + j] += c * x
    return [x % R for x in a], b


def test_cpp_wrapper(tmp_path):
    """poly_divide and Polynomial::long_division of include/kzg_mi355x.hpp: tests/cpp_poly_divide_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_poly_divide_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_poly_divide_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("na,nb", [((1 << 16) + 3, 257), (1 << 16, (1 << 15) + 1)])
def test_larger_cases_against_the_c_oracle(eng, na, nb):
    a, b = larger_case(na, nb)
    wq, wr = C.long_division(a, b)
    assert wr is not None
    assert divide(eng, a, na, 1, b) == (wq, wr, [False])
    assert divide(eng, a, na, 1, b, MONT, True, True) == (wq, wr, [False])


def test_full_size_identity_at_two_points(eng):
    """na = 2^20, nb = 2^10 + 1, device buffers: a(z) = q(z) b(z) + r(z) at two fixed points through kzg_poly_eval"""
    na, nb = 1 << 20, (1 << 10) + 1
    m, nr = na - nb + 1, nb - 1
    a = kzg_amd.DeviceBuffer(eng, na).fill_random(20)
    b = kzg_amd.DeviceBuffer(eng, nb).fill_random(21)
    q, r = kzg_amd.DeviceBuffer(eng, m), kzg_amd.DeviceBuffer(eng, nr)
    try:
        assert any(b.download(1, nb - 1))
        _, _, ex = eng.poly_divide(a, b, q_out=q, r_out=r)
        assert ex == [False]
        assert all(v < R for v in unpack_scalars(q.download(64)) + unpack_scalars(r.download(64)))
        for z in (0x1234567, R - 0xABCDEF):
            az, qz, bz, rz = (eng.poly_eval(d, z, n=n) for d, n in ((a, na), (q, m), (b, nb), (r, nr)))
            assert az == (qz * bz + rz) % R
    finally:
        for d in (a, b, q, r):
            d.free()


def test_two_threads_on_one_context(eng):
    cases = [case(3000, 200, 1), case(2500, 1300, 2)]
    want = [C.long_division(a, b) for a, b in cases]
    got, errs = [None, None], []

    def work(i):
        try:
            for _ in range(4):
                res = divide(eng, cases[i][0], len(cases[i][0]), 1, cases[i][1])
                if got[i] is not None and res != got[i]:
                    errs.append("thread %d: two calls disagree" % i)
                got[i] = res
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert got[i] == (want[i][0], want[i][1], [False])


def test_shape_errors_leave_the_outputs_untouched(eng):
    lib, ctx = eng.lib, eng.ctx
    na, nb = 12, 5
    a, b = case(na, nb)
    ab, bb = pack_scalars(a), pack_scalars(b)
    q, r = ctypes.create_string_buffer(A5 * 512, 512), ctypes.create_string_buffer(A5 * 512, 512)
    ex = (ctypes.c_int * 2)(-7, -7)
    zero_top, r_top = pack_scalars(b[:-1]) + bytes(32), pack_scalars(b[:-1]) + le(R)
    mont_r_top = pack_scalars(b[:-1]) + le(R)   # Montgomery bytes equal to r: the residue 0 as well
    codes = [
        lib.kzg_poly_divide(None, ab, na, 1, bb, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, None, na, 1, bb, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, None, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, bb, nb, CAN, 0, None, None, ex),
        lib.kzg_poly_divide(ctx, ab, 0, 1, bb, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, bb, 0, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, bb, nb, 2, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, zero_top, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, zero_top, nb, MONT, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, r_top, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, mont_r_top, nb, MONT, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1, bytes(32 * nb), nb, CAN, 0, q, r, ex),          # the zero divisor
        lib.kzg_poly_divide(ctx, ab, na, 1, bytes(32), 1, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, (1 << 27) + 1, 1, bb, nb, CAN, 0, q, r, ex),
        lib.kzg_poly_divide(ctx, ab, na, 1 << 62, bb, nb, CAN, 0, q, r, ex),                # batch x na x 32 beyond size_t
        lib.kzg_poly_divide(ctx, ab, 3, 1, bb, nb, CAN, 0, None, None, ex),                 # na < nb: r would not be empty
        lib.kzg_poly_divide(ctx, ab, na, 1, pack_scalars([3]), 1, CAN, 0, None, None, ex),  # nb == 1: q would not be empty
    ]
    assert codes == [SH] * len(codes), codes
    # the same for a device-resident divisor: the check reads its top coefficient
    da, dq, dr = dev_buffer(eng, len(ab)), dev_buffer(eng, 512), dev_buffer(eng, 512)
    assert lib.kzg_dev_upload(ctx, da, ab, len(ab)) == 0
    for bad in (zero_top, r_top):
        db = dev_buffer(eng, len(bad))
        assert lib.kzg_dev_upload(ctx, db, bad, len(bad)) == 0
        for sfmt in (CAN, MONT):
            assert lib.kzg_poly_divide(ctx, da, na, 1, db, nb, sfmt, L.IN_DEVICE | L.OUT_DEVICE, dq, dr, ex) == SH
            assert lib.kzg_poly_divide(ctx, da, na, 1, db, nb, sfmt, L.IN_DEVICE, q, r, ex) == SH
        lib.kzg_dev_free(ctx, db)
    assert dev_download(eng, dq, 512) == A5 * 512 and dev_download(eng, dr, 512) == A5 * 512
    for p in (da, dq, dr):
        lib.kzg_dev_free(ctx, p)
    assert q.raw == A5 * 512 and r.raw == A5 * 512 and list(ex) == [-7, -7]
    assert lib.kzg_poly_divide(ctx, ab, na, 0, bb, nb, CAN, 0, q, r, ex) == 0               # batch == 0
    assert lib.kzg_poly_divide(ctx, None, na, 0, None, nb, CAN, 0, None, None, None) == 0
    assert q.raw == A5 * 512 and r.raw == A5 * 512 and list(ex) == [-7, -7]
    for bad in (3, 128, -1):
        assert lib.kzg_ctx_set_option(ctx, b"poly_divide_base", bad) == SH
    # one NULL output beside one that is empty anyway: nothing is written but `exact`
    assert lib.kzg_poly_divide(ctx, ab, 3, 2, bb, nb, CAN, 0, q, None, ex) == 0 and list(ex) == [0, 0]
    assert lib.kzg_poly_divide(ctx, bytes(32 * 3) + ab[:96], 3, 2, bb, nb, CAN, 0, q, None, ex) == 0 and list(ex) == [1, 0]
    assert lib.kzg_poly_divide(ctx, ab, na, 1, pack_scalars([3]), 1, CAN, 0, None, r, ex) == 0 and list(ex) == [1, 0]
    assert q.raw == A5 * 512 and r.raw == A5 * 512
    assert lib.kzg_poly_divide(ctx, ab, na, 1, bb, nb, CAN, 0, q, r, None) == 0
    assert unpack_scalars(q.raw[: 32 * 8]) == reference(a, b)[0] and q.raw[32 * 8:] == A5 * (512 - 256)
