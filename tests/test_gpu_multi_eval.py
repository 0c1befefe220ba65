"""kzg_poly_multi_eval and kzg_interpolate on the GPU, through the C ABI via kzg_amd.  Every expected value comes from oracle.kzg_model
(Polynomial.eval, multi_eval, lagrange_interpolation) or from kzg_poly_eval (the parity tests), never from the calls under test, and
every comparison is equality of integers or bytes."""
import ctypes
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import ReferencePanic, pack_scalars, unpack_scalars
from oracle import kzg_model as M
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
SH = L.KZG_ERR_SHAPE
A5 = b"\xa5"
TAU = 0x1F2E3D4C5B6A7988
NS = [1, 2, 7, 8, 9, 255, 256, 257, 2049, 4097]
KS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 300]
ROOT32 = M.FR_ROOT_OF_UNITY  # of order 2^32


def le(v):
    return int(v).to_bytes(32, "little")


def scalars(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(count)]


def expect(coeffs, xs):
    p = M.Polynomial([c % R for c in coeffs])
    return [p.eval(x) for x in xs]


def forced(eng, segment, chunk):
    eng.set_option("multi_eval_segment", segment)
    eng.set_option("multi_eval_points_chunk", chunk)


@pytest.fixture
def plans(eng):
    """calls fn once under automatic planning and once with 8-coefficient segments and 64 points per pass"""
    def run(fn):
        out = []
        for seg, chunk in ((0, 0), (8, 64)):
            forced(eng, seg, chunk)
            try:
                out.append(fn())
            finally:
                forced(eng, 0, 0)
        return out
    return run


_REF = {}


def shape_case(n, k):
    """(coefficients, points, values) of the shape, computed once for both plans"""
    if (n, k) not in _REF:
        coeffs, xs = scalars(1000 * n + k, n), scalars(7000 * n + k, k)
        _REF[(n, k)] = (coeffs, xs, expect(coeffs, xs))
    return _REF[(n, k)]


@pytest.mark.parametrize("mode", ["auto", "segment8_chunk64"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_small_shapes_against_the_oracle(eng, n, k, mode):
    coeffs, xs, want = shape_case(n, k)
    if mode != "auto":  # 257 coefficients: 33 segments, the last of one coefficient; 300 points: five passes
        forced(eng, 8, 64)
    try:
        got = eng.poly_multi_eval(coeffs, xs)
    finally:
        forced(eng, 0, 0)
    assert got == want


def raw_call(eng, coeffs, n, batch, xs, sfmt, in_dev, out_dev):
    """the C call with host / device coefficients in `sfmt` and a host / device output -> the values as ints"""
    k = len(xs)
    enc = (lambda v: le(v * MONT_R % R)) if sfmt == MONT else le
    cb = b"".join(enc(c) for c in coeffs)
    xb = b"".join(enc(x) for x in xs)
    flags, src = 0, cb
    if in_dev:
        src = dev_buffer(eng, len(cb))
        assert eng.lib.kzg_dev_upload(eng.ctx, src, cb, len(cb)) == 0
        flags |= L.IN_DEVICE
    if out_dev:
        dst = dev_buffer(eng, 32 * batch * k + 64)
        flags |= L.OUT_DEVICE
    else:
        dst = ctypes.create_string_buffer(A5 * (32 * batch * k + 64), 32 * batch * k + 64)
    assert eng.lib.kzg_poly_multi_eval(eng.ctx, src, n, batch, xb, k, sfmt, flags, dst) == 0, eng.last_error()
    raw = dev_download(eng, dst, 32 * batch * k + 64) if out_dev else dst.raw
    if in_dev:
        eng.lib.kzg_dev_free(eng.ctx, src)
    if out_dev:
        eng.lib.kzg_dev_free(eng.ctx, dst)
    assert raw[32 * batch * k:] == A5 * 64  # nothing written past the batch x k values
    vals = unpack_scalars(raw[: 32 * batch * k])
    assert all(v < R for v in vals)
    return [v * pow(MONT_R, -1, R) % R for v in vals] if sfmt == MONT else vals


@pytest.mark.parametrize("k", [3, 65])  # both lane layouts
@pytest.mark.parametrize("sfmt", [CAN, MONT])
def test_formats_buffers_and_a_batch_of_three(eng, plans, sfmt, k):
    n, batch = 257, 3
    coeffs, xs = scalars(31 + k, n * batch), scalars(32 + k, k)
    want = [y for b in range(batch) for y in expect(coeffs[b * n:(b + 1) * n], xs)]
    for in_dev in (False, True):
        for out_dev in (False, True):
            for got in plans(lambda: raw_call(eng, coeffs, n, batch, xs, sfmt, in_dev, out_dev)):
                assert got == want, (in_dev, out_dev)


def test_python_surface_batch_and_device_buffers(eng):
    n, batch, k = 100, 3, 70
    coeffs, xs = scalars(41, n * batch), scalars(42, k)
    want = [expect(coeffs[b * n:(b + 1) * n], xs) for b in range(batch)]
    assert eng.poly_multi_eval(coeffs, xs, batch=batch) == want
    buf = eng.alloc_scalars(n * batch).upload(pack_scalars(coeffs))
    out = eng.alloc_scalars(batch * k)
    try:
        assert eng.poly_multi_eval(buf, xs, n=n, batch=batch) == want
        assert eng.poly_multi_eval(buf, xs, n=n, batch=batch, out=out) is out
        assert unpack_scalars(out.download()) == [y for row in want for y in row]
        assert eng.poly_multi_eval(buf, xs[:5], n=n) == want[0][:5]  # the first polynomial alone
        with pytest.raises(ReferencePanic):
            eng.poly_multi_eval(buf, xs, n=n, batch=batch + 1)
    finally:
        buf.free()
        out.free()


EXTREME_XS = [0, 1, R - 1, 2, ROOT32, 5, 5, 5]


@pytest.mark.parametrize("name", ["zeros", "all_r_minus_1", "leading_zero"])
@pytest.mark.parametrize("k", [len(EXTREME_XS), 64 + len(EXTREME_XS)])
def test_extreme_points_and_coefficients(eng, plans, name, k):
    n = 300
    coeffs = {"zeros": [0] * n, "all_r_minus_1": [R - 1] * n, "leading_zero": scalars(51, n - 2) + [0, 0]}[name]
    xs = EXTREME_XS + scalars(52, k - len(EXTREME_XS))
    want = expect(coeffs, xs)
    assert want[5] == want[6] == want[7] and want[0] == coeffs[0]
    for got in plans(lambda: eng.poly_multi_eval(coeffs, xs)):
        assert got == want


@pytest.mark.parametrize("k", [len(EXTREME_XS), 64 + len(EXTREME_XS)])
def test_canonical_coefficients_of_any_256_bit_value_count_as_their_residue(eng, plans, k):
    n = 300
    rawc = [(1 << 256) - 1, R, R + 1, (1 << 256) - 2] * (n // 4)
    xs = EXTREME_XS + scalars(53, k - len(EXTREME_XS))
    want = expect(rawc, xs)
    blob = b"".join(le(c) for c in rawc)
    for got in plans(lambda: eng.poly_multi_eval(blob, xs)):
        assert got == want


def poly_eval_bytes(eng, ptr, n, x, sfmt, flags):
    out = ctypes.create_string_buffer(32)
    assert eng.lib.kzg_poly_eval(eng.ctx, ptr, n, le(x), sfmt, flags, out) == 0
    return out.raw


def test_the_bytes_of_k_poly_eval_calls(eng, plans):
    n, k = 5000, 70
    blob, xs = pack_scalars(scalars(61, n)), scalars(62, k)
    want = b"".join(poly_eval_bytes(eng, blob, n, x, CAN, 0) for x in xs)

    def call():
        out = ctypes.create_string_buffer(32 * k)
        assert eng.lib.kzg_poly_multi_eval(eng.ctx, blob, n, 1, pack_scalars(xs), k, CAN, 0, out) == 0
        return out.raw
    for got in plans(call):
        assert got == want


def test_2_20_coefficients_at_1024_points_against_poly_eval(eng):
    n, k = 1 << 20, 1024
    buf = eng.alloc_scalars(n).fill_random(0x20)
    xs = scalars(63, k)
    try:
        want = b"".join(poly_eval_bytes(eng, buf.ptr, n, x, CAN, L.IN_DEVICE) for x in xs)
        out = ctypes.create_string_buffer(32 * k)
        assert eng.lib.kzg_poly_multi_eval(eng.ctx, buf.ptr, n, 1, pack_scalars(xs), k, CAN, L.IN_DEVICE, out) == 0
        assert out.raw == want
    finally:
        buf.free()


@pytest.mark.parametrize("n", [1, 2, 17, 64])
def test_the_reference_shape_against_the_oracle_tree(eng, n):
    coeffs = scalars(71 + n, n - 1) + [1 + scalars(72, 1)[0] % (R - 1)]  # degree n - 1
    xs = scalars(73 + n, n + 1)
    want = M.Polynomial(coeffs).multi_eval(xs)
    assert kzg_amd.Polynomial(coeffs).multi_eval(eng, xs) == want
    if n >= 2:
        with pytest.raises(ReferencePanic):  # assert!(xs.len() > self.degree())
            kzg_amd.Polynomial(coeffs).multi_eval(eng, xs[: n - 1])


def test_shape_errors_leave_the_output_untouched(eng):
    lib, ctx = eng.lib, eng.ctx
    n, k = 16, 3
    blob, xs = pack_scalars(scalars(81, n)), pack_scalars([1, 2, 3])
    big = pack_scalars([1, 2]) + le(R)
    out = ctypes.create_string_buffer(A5 * (32 * k), 32 * k)
    bad = [
        lib.kzg_poly_multi_eval(ctx, blob, 0, 1, xs, k, CAN, 0, out),            # n == 0
        lib.kzg_poly_multi_eval(ctx, blob, (1 << 28) + 1, 1, xs, k, CAN, 0, out),  # n above the limit
        lib.kzg_poly_multi_eval(ctx, blob, n, 1, big, k, CAN, 0, out),           # x == r
        lib.kzg_poly_multi_eval(ctx, blob, n, 1, big, k, MONT, 0, out),
        lib.kzg_poly_multi_eval(ctx, blob, n, 1, xs, k, 2, 0, out),              # unknown format
        lib.kzg_poly_multi_eval(ctx, None, n, 1, xs, k, CAN, 0, out),            # NULL buffers
        lib.kzg_poly_multi_eval(ctx, blob, n, 1, None, k, CAN, 0, out),
        lib.kzg_poly_multi_eval(ctx, blob, n, 1, xs, k, CAN, 0, None),
        lib.kzg_poly_multi_eval(None, blob, n, 1, xs, k, CAN, 0, out),
        lib.kzg_poly_multi_eval(ctx, blob, n, 1 << 62, xs, k, CAN, 0, out),      # size overflow
    ]
    assert bad == [SH] * len(bad), bad
    assert lib.kzg_poly_multi_eval(ctx, blob, n, 1, xs, 0, CAN, 0, out) == 0     # k == 0
    assert lib.kzg_poly_multi_eval(ctx, blob, n, 0, xs, k, CAN, 0, out) == 0     # batch == 0
    assert out.raw == A5 * (32 * k)
    for key, value in (("multi_eval_segment", 4), ("multi_eval_segment", 24), ("multi_eval_points_chunk", -1)):
        with pytest.raises(ReferencePanic):
            eng.set_option(key, value)


# ---- interpolation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 64, 65, 257])
def test_interpolation_against_the_oracle(eng, k):
    xs, ys = scalars(91 + k, k), scalars(92 + k, k)
    assert len(set(xs)) == k
    want = M.Polynomial.lagrange_interpolation(xs, ys)
    got = kzg_amd.Polynomial.lagrange_interpolation(eng, xs, ys)
    assert got.coeffs == want.coeffs[:k] + [0] * (k - len(want.coeffs[:k])) and got.degree == want.degree
    assert eng.interpolate(xs, ys) == got.coeffs


def test_interpolation_of_one_point_the_mirror_quirk_and_the_constant(eng):
    x, y = scalars(93, 2)
    want = M.Polynomial.lagrange_interpolation([x], [y])  # X + (y - x), src/polynomial.rs:269-272
    got = kzg_amd.Polynomial.lagrange_interpolation(eng, [x], [y])
    assert got.coeffs == want.coeffs == [(y - x) % R, 1] and got.degree == 1
    assert eng.interpolate([x], [y]) == [y]
    assert eng.interpolate([x], [[y], [0], [R - 1]]) == [[y], [0], [R - 1]]
    out = ctypes.create_string_buffer(32)
    assert eng.lib.kzg_interpolate(eng.ctx, le(x), le((1 << 256) - 1), 1, 1, CAN, 0, out) == 0  # a raw value: its residue
    assert unpack_scalars(out.raw) == [((1 << 256) - 1) % R]


def test_interpolation_of_three_value_vectors_both_formats_and_a_device_output(eng):
    k, batch = 65, 3
    xs, ys = scalars(94, k), [scalars(95 + b, k) for b in range(batch)]
    want = [M.Polynomial.lagrange_interpolation(xs, v).coeffs[:k] for v in ys]
    want = [c + [0] * (k - len(c)) for c in want]
    assert eng.interpolate(xs, ys) == want
    flat = [y for v in ys for y in v]
    dst = dev_buffer(eng, 32 * batch * k + 64)
    try:
        xb, yb = (b"".join(le(v * MONT_R % R) for v in vec) for vec in (xs, flat))
        assert eng.lib.kzg_interpolate(eng.ctx, xb, yb, k, batch, MONT, L.OUT_DEVICE, dst) == 0, eng.last_error()
        raw = dev_download(eng, dst, 32 * batch * k + 64)
    finally:
        eng.lib.kzg_dev_free(eng.ctx, dst)
    assert raw[32 * batch * k:] == A5 * 64
    assert [v * pow(MONT_R, -1, R) % R for v in unpack_scalars(raw[: 32 * batch * k])] == [c for row in want for c in row]


def test_interpolate_round_trip_at_300(eng):
    k = 300
    coeffs, xs = scalars(96, k), scalars(97, k)
    assert eng.interpolate(xs, eng.poly_multi_eval(coeffs, xs)) == coeffs


def test_interpolation_shape_errors(eng):
    lib, ctx = eng.lib, eng.ctx
    k = 4
    xs, ys = pack_scalars([1, 2, 3, 4]), pack_scalars([5, 6, 7, 8])
    out = ctypes.create_string_buffer(A5 * (32 * k), 32 * k)
    bad = [
        lib.kzg_interpolate(ctx, pack_scalars([1, 2, 3, 2]), ys, k, 1, CAN, 0, out),  # two equal xs
        lib.kzg_interpolate(ctx, pack_scalars([1, 2, 3]) + le(R), ys, k, 1, CAN, 0, out),
        lib.kzg_interpolate(ctx, xs, ys, 0, 1, CAN, 0, out),
        lib.kzg_interpolate(ctx, xs, ys, 16385, 1, CAN, 0, out),
        lib.kzg_interpolate(ctx, xs, ys, k, 1, 2, 0, out),
        lib.kzg_interpolate(ctx, None, ys, k, 1, CAN, 0, out),
        lib.kzg_interpolate(ctx, xs, None, k, 1, CAN, 0, out),
        lib.kzg_interpolate(ctx, xs, ys, k, 1, CAN, 0, None),
        lib.kzg_interpolate(None, xs, ys, k, 1, CAN, 0, out),
    ]
    assert bad == [SH] * len(bad), bad
    assert lib.kzg_interpolate(ctx, xs, ys, k, 0, CAN, 0, out) == 0  # batch == 0
    assert out.raw == A5 * (32 * k)
    with pytest.raises(ReferencePanic):
        eng.interpolate([7, 8, 7], [1, 2, 3])


# ---- open_at_points --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params(eng):
    p = kzg_amd.setup(eng, TAU, 300, g2_len=8)
    yield p
    p.gs.free()
    p.hs.free()


@pytest.mark.parametrize("k", [5, 1])
def test_open_at_points(eng, params, k):
    n = 300
    poly = kzg_amd.Polynomial(scalars(101, n))
    xs = scalars(102 + k, k)
    want = expect(poly.coeffs, xs)
    prover, verifier = kzg_amd.KZGProver(params), kzg_amd.KZGVerifier(params)
    ys, witness = prover.open_at_points(poly, xs)
    assert ys == want
    ref = prover.create_witness_batched(poly, xs, want)
    assert witness.w == ref.w and witness.r.coeffs == ref.r.coeffs
    assert verifier.verify_eval_batched(xs, prover.commit(poly), witness) is True


# ---- concurrency -----------------------------------------------------------------------------------------------------------------
def test_four_threads_on_one_context(eng):
    n, k, calls = 2049, 65, 50
    cases = []
    for t in range(4):
        coeffs, xs = scalars(111 + t, n), scalars(121 + t, k)
        cases.append((pack_scalars(coeffs), xs, expect(coeffs, xs)))
    wrong = []

    def work(blob, xs, want):
        try:
            for _ in range(calls):
                if eng.poly_multi_eval(blob, xs) != want:
                    wrong.append("values")
        except Exception as e:  # noqa: BLE001 -- reported below, on the main thread
            wrong.append(repr(e))
    threads = [threading.Thread(target=work, args=c) for c in cases]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not wrong, wrong[:3]
