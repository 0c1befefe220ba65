"""kzg_point_tree_* on the GPU, through the C ABI via kzg_amd.  Expected values come from oracle.kzg_model (SubProductTree,
Polynomial) at the small shapes, from tests/point_tree_model.py (checked against the oracle in tests/test_point_tree_model.py) and from
kzg_poly_multi_eval / kzg_interpolate / kzg_poly_eval -- independent code paths -- at the large ones, never from the calls under
test; every comparison is equality of integers or bytes."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import Polynomial, ReferencePanic, pack_scalars, unpack_scalars
from oracle import kzg_model as M
from tests import point_tree_model as PT
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
SH = L.KZG_ERR_SHAPE
PAD = 64  # bytes behind every output that must stay 0xA5
LEAF, SMALL = PT.LEAF, PT.SMALL
# one below, at and one above the leaf and the in-LDS transform bound (the transforms above it add global stages: the one other path)
KS = [1, 2, 3, LEAF - 1, LEAF, LEAF + 1, 2 * LEAF + 1, SMALL - 1, SMALL, SMALL + 1, 5000]
LEAVES = [0, 1, 4]
ORACLE_K = 2 * LEAF + 1  # up to here the expected values are the oracle's


def le(v):
    return int(v).to_bytes(32, "little")


def encode(vals, sfmt):
    """ints below 2^256 as the calls read them: canonical bytes as they are (a value >= r counts as its residue); Montgomery: the
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


def points(k, seed=0):
    rng = random.Random(7000 + k + seed)
    xs = [rng.randrange(R) for _ in range(k)]
    for pos, v in ((1, 0), (2, 1), (3, R - 1)):
        if k > pos + 1:
            xs[pos] = v
    return xs


def values(count, seed, big=True):
    """random residues; with `big`, the first and every 97th are given as residue + r"""
    rng = random.Random(seed)
    return [rng.randrange(R) + (R if big and i % 97 == 0 and i % 2 == 0 else 0) for i in range(count)]


class Plan:
    def __init__(self, eng, xs, sfmt=CAN, leaf=0):
        self.eng, self.k, self.h = eng, len(xs), ctypes.c_void_p()
        eng.set_option("point_tree_leaf", leaf)
        try:
            rc = eng.lib.kzg_point_tree_setup(eng.ctx, encode(xs, sfmt), len(xs), sfmt, ctypes.byref(self.h))
        finally:
            eng.set_option("point_tree_leaf", 0)
        assert rc == 0, (rc, eng.last_error())

    def shape(self):
        k, padded, nbytes, distinct = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(-1)
        assert self.eng.lib.kzg_point_tree_shape(self.h, ctypes.byref(k), ctypes.byref(padded), ctypes.byref(nbytes), ctypes.byref(distinct)) == 0
        return k.value, padded.value, nbytes.value, distinct.value

    def free(self):
        self.eng.lib.kzg_point_tree_free(self.eng.ctx, self.h)


def run(eng, name, plan, blob, out_count, sfmt=CAN, in_dev=False, out_dev=False, n=None, batch=1, expect=0, handle="plan"):
    """one call of kzg_point_tree_<name> on an output prefilled with 0xA5: (rc, the out_count output scalars as bytes).  The PAD bytes
    behind the output must be untouched; a failing call must leave all of it untouched."""
    fn = getattr(eng.lib, "kzg_point_tree_" + name)
    nbytes = 32 * out_count + PAD
    flags = (L.IN_DEVICE if in_dev else 0) | (L.OUT_DEVICE if out_dev else 0)
    src = None
    if blob is not None and in_dev:
        src = ctypes.c_void_p()
        assert eng.lib.kzg_dev_alloc(eng.ctx, max(len(blob), 32), ctypes.byref(src)) == 0
        assert eng.lib.kzg_dev_upload(eng.ctx, src, blob, len(blob)) == 0
    out = dev_buffer(eng, nbytes) if out_dev else ctypes.create_string_buffer(b"\xa5" * nbytes, nbytes)
    h = plan.h if handle == "plan" else handle
    inp = src if src is not None else blob
    try:
        if name == "product":
            rc = fn(eng.ctx, h, sfmt, flags, out)
        elif name == "eval":
            rc = fn(eng.ctx, h, inp, n, batch, sfmt, flags, out)
        else:
            rc = fn(eng.ctx, h, inp, batch, sfmt, flags, out)
        raw = dev_download(eng, out, nbytes) if out_dev else out.raw
    finally:
        if src is not None:
            eng.lib.kzg_dev_free(eng.ctx, src)
        if out_dev:
            eng.lib.kzg_dev_free(eng.ctx, out)
    assert rc == expect, (name, rc)
    assert raw[32 * out_count:] == b"\xa5" * PAD, "the call wrote behind its output"
    if rc:
        assert raw == b"\xa5" * nbytes, "a failing call wrote to its output"
    return raw[: 32 * out_count]


def multi_eval_bytes(eng, coeffs_blob, n, batch, xs, sfmt=CAN):
    k = len(xs)
    out = ctypes.create_string_buffer(32 * batch * k)
    assert eng.lib.kzg_poly_multi_eval(eng.ctx, coeffs_blob, n, batch, encode(xs, sfmt), k, sfmt, 0, out) == 0
    return out.raw


def interpolate_bytes(eng, xs, ys_blob, batch, sfmt=CAN):
    k = len(xs)
    out = ctypes.create_string_buffer(32 * batch * k)
    assert eng.lib.kzg_interpolate(eng.ctx, encode(xs, sfmt), ys_blob, k, batch, sfmt, 0, out) == 0
    return out.raw


_MODEL = {}


def model(k):
    """the big-int model's tree of points(k) at the default leaf: built once per k"""
    if k not in _MODEL:
        _MODEL[k] = PT.Tree(points(k))
    return _MODEL[k]


def ns_for(k):
    K = PT.next_pow2(k)
    return sorted({1, k, K, K + 1, 2 * K + 1})


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("k", KS)
def test_every_call_at_every_shape(eng, k, leaf):
    xs, B = points(k), 3
    plan = Plan(eng, xs, leaf=leaf)
    try:
        kk, K, nbytes, distinct = plan.shape()
        assert (kk, K, distinct) == (k, PT.next_pow2(k), 1)
        assert nbytes == PT.plan_bytes(k, leaf if leaf else LEAF)
        # the product
        want_m = M.SubProductTree.new_from_points(xs).product.coeffs[: k + 1] if k <= ORACLE_K else model(k).M
        assert decode(run(eng, "product", plan, None, k + 1), CAN) == want_m
        # values: kzg_poly_multi_eval's bytes, and the oracle's integers at the small shapes
        for n in ns_for(k):
            coeffs = values(B * n, 31 * k + n)
            blob = encode(coeffs, CAN)
            got = run(eng, "eval", plan, blob, B * k, n=n, batch=B)
            assert got == multi_eval_bytes(eng, blob, n, B, xs), (k, n)
            if k <= ORACLE_K:
                assert decode(got, CAN) == [M.Polynomial(coeffs[b * n:(b + 1) * n]).eval(x) for b in range(B) for x in xs]
        # the combination
        cs = values(B * k, 77 * k)
        got = decode(run(eng, "combine", plan, encode(cs, CAN), B * k, batch=B), CAN)
        for b in range(B):
            row = cs[b * k:(b + 1) * k]
            if k == 1:
                want = [row[0] % R]
            elif k <= ORACLE_K:
                want = (M.SubProductTree.new_from_points(xs).linear_mod_combination([c % R for c in row]).coeffs + [0] * k)[:k]
            else:
                want = model(k).combine(row)
            assert got[b * k:(b + 1) * k] == want, (k, b)
        # interpolation: kzg_interpolate's bytes
        ys = encode(values(B * k, 91 * k), CAN)
        assert run(eng, "interpolate", plan, ys, B * k, batch=B) == interpolate_bytes(eng, xs, ys, B), k
    finally:
        plan.free()


@pytest.mark.parametrize("sfmt", [CAN, MONT])
@pytest.mark.parametrize("in_dev,out_dev", [(False, False), (True, False), (False, True), (True, True)])
def test_formats_and_residency(eng, sfmt, in_dev, out_dev):
    k, n, B = 37, 150, 2  # K = 64: two levels of transforms above the leaf, three blocks
    xs = points(k)
    plan = Plan(eng, xs, sfmt)
    try:
        coeffs, cs, ys = values(B * n, 1), values(B * k, 2), values(B * k, 3)
        got = decode(run(eng, "eval", plan, encode(coeffs, sfmt), B * k, sfmt, in_dev, out_dev, n=n, batch=B), sfmt)
        assert got == [M.Polynomial(coeffs[b * n:(b + 1) * n]).eval(x) for b in range(B) for x in xs]
        ot = M.SubProductTree.new_from_points(xs)
        assert decode(run(eng, "product", plan, None, k + 1, sfmt, False, out_dev), sfmt) == ot.product.coeffs[: k + 1]
        got = decode(run(eng, "combine", plan, encode(cs, sfmt), B * k, sfmt, in_dev, out_dev, batch=B), sfmt)
        assert got == sum(((ot.linear_mod_combination([c % R for c in cs[b * k:(b + 1) * k]]).coeffs + [0] * k)[:k] for b in range(B)), [])
        got = decode(run(eng, "interpolate", plan, encode(ys, sfmt), B * k, sfmt, in_dev, out_dev, batch=B), sfmt)
        want = [M.Polynomial.lagrange_interpolation(xs, [y % R for y in ys[b * k:(b + 1) * k]]) for b in range(B)]
        assert got == sum(((w.coeffs + [0] * k)[:k] for w in want), [])
    finally:
        plan.free()


def test_repeated_points(eng):
    xs = [5, 9, 5, 0, 0, R - 1, 7]
    for leaf in (0, 1):
        plan = Plan(eng, xs, leaf=leaf)
        try:
            assert plan.shape()[3] == 0
            p = values(19, 5)
            assert decode(run(eng, "eval", plan, encode(p, CAN), 7, n=19), CAN) == [M.Polynomial(p).eval(x) for x in xs]
            ot = M.SubProductTree.new_from_points(xs)
            assert decode(run(eng, "product", plan, None, 8), CAN) == ot.product.coeffs[:8]
            cs = values(7, 6, big=False)
            assert decode(run(eng, "combine", plan, encode(cs, CAN), 7), CAN) == (ot.linear_mod_combination(cs).coeffs + [0] * 7)[:7]
            run(eng, "interpolate", plan, encode(values(7, 8), CAN), 7, expect=SH)
            run(eng, "interpolate", plan, encode(values(7, 8), CAN), 7, out_dev=True, expect=SH)
        finally:
            plan.free()


def test_shape_errors_leave_outputs_untouched(eng):
    lib, h = eng.lib, ctypes.c_void_p()
    one = le(1)
    assert lib.kzg_point_tree_setup(eng.ctx, one, 0, CAN, ctypes.byref(h)) == SH                 # k == 0
    assert lib.kzg_point_tree_setup(eng.ctx, one, (1 << 22) + 1, CAN, ctypes.byref(h)) == SH     # k out of range: xs is not read
    assert lib.kzg_point_tree_setup(eng.ctx, None, 1, CAN, ctypes.byref(h)) == SH
    assert lib.kzg_point_tree_setup(eng.ctx, one, 1, CAN, None) == SH
    assert lib.kzg_point_tree_setup(eng.ctx, one, 1, 7, ctypes.byref(h)) == SH
    assert lib.kzg_point_tree_setup(eng.ctx, le(R), 1, CAN, ctypes.byref(h)) == SH               # a point that is not below r
    assert lib.kzg_point_tree_setup(eng.ctx, le(3) + le(R + 1), 2, MONT, ctypes.byref(h)) == SH
    assert h.value is None
    assert lib.kzg_point_tree_shape(None, None, None, None, None) == SH
    lib.kzg_point_tree_free(eng.ctx, None)
    for bad in (-1, 3, 32):
        with pytest.raises(ReferencePanic):
            eng.set_option("point_tree_leaf", bad)
    plan = Plan(eng, [3, 4, 5])
    try:
        blob = encode([1, 2, 3], CAN)
        for name in ("eval", "combine", "interpolate"):
            kw = {"n": 3} if name == "eval" else {}
            run(eng, name, plan, blob, 3, handle=None, expect=SH, **kw)      # a NULL plan
            run(eng, name, plan, None, 3, expect=SH, **kw)                   # a NULL input
            run(eng, name, plan, blob, 3, sfmt=7, expect=SH, **kw)           # an unknown format
            run(eng, name, plan, blob, 3, out_dev=True, sfmt=7, expect=SH, **kw)
            assert run(eng, name, plan, blob, 3, batch=0, **kw) == b"\xa5" * 96  # batch == 0: KZG_OK, nothing written
            fn = getattr(lib, "kzg_point_tree_" + name)
            args = (eng.ctx, plan.h, blob) + ((3,) if name == "eval" else ()) + (1, CAN, 0, None)
            assert fn(*args) == SH                                           # a NULL output
        run(eng, "eval", plan, blob, 3, n=0, expect=SH)                      # an empty polynomial
        run(eng, "product", plan, None, 4, handle=None, expect=SH)
        run(eng, "product", plan, None, 4, sfmt=7, expect=SH)
        assert lib.kzg_point_tree_product(eng.ctx, plan.h, CAN, 0, None) == SH
        assert run(eng, "eval", plan, blob, 3, batch=0, n=3) == b"\xa5" * 96
    finally:
        plan.free()


def random_blob(count, seed):
    """count scalars below 2^254 < r"""
    b = bytearray(random.Random(seed).randbytes(32 * count))
    b[31::32] = bytes(v & 0x3F for v in b[31::32])
    return bytes(b)


@pytest.mark.parametrize("k", [16385, (1 << 16) + 1])
def test_past_the_old_limit(eng, k):
    n = (1 << 16) + 3
    xs_blob, coeffs, ys = random_blob(k, k), random_blob(n, k + 1), random_blob(k, k + 2)
    xs = unpack_scalars(xs_blob)
    assert len(set(xs)) == k
    plan = Plan(eng, xs)
    try:
        assert plan.shape() == (k, PT.next_pow2(k), PT.plan_bytes(k), 1)
        want = multi_eval_bytes(eng, coeffs, n, 1, xs)
        assert run(eng, "eval", plan, coeffs, k, n=n) == want
        f = run(eng, "interpolate", plan, ys, k)
        assert multi_eval_bytes(eng, f, k, 1, xs) == ys  # the interpolant takes the values
    finally:
        plan.free()


@pytest.mark.limit(300)
def test_full_size(eng):
    """k = n = 2^20, device buffers: 64 sampled values against kzg_poly_eval"""
    k = n = 1 << 20
    xs_blob = random_blob(k, 20)
    h = ctypes.c_void_p()
    assert eng.lib.kzg_point_tree_setup(eng.ctx, xs_blob, k, CAN, ctypes.byref(h)) == 0
    coeffs, ys = kzg_amd.DeviceBuffer(eng, n).fill_random(21), kzg_amd.DeviceBuffer(eng, k)
    try:
        assert eng.lib.kzg_point_tree_eval(eng.ctx, h, coeffs.ptr, n, 1, CAN, L.IN_DEVICE | L.OUT_DEVICE, ys.ptr) == 0
        got = ys.download()
        for i in random.Random(22).sample(range(k), 62) + [0, k - 1]:
            x = int.from_bytes(xs_blob[32 * i:32 * i + 32], "little")
            assert int.from_bytes(got[32 * i:32 * i + 32], "little") == eng.poly_eval(coeffs, x, n=n), i
    finally:
        eng.lib.kzg_point_tree_free(eng.ctx, h)
        coeffs.free()
        ys.free()


def test_a_batch_across_chunks_equals_single_calls(eng):
    k, n = 5000, 100
    K = PT.next_pow2(k)
    C = PT.chunk_units(K)
    B = C + 1
    xs = points(k)
    plan = Plan(eng, xs)
    try:
        coeffs = random_blob(B * n, 1)
        got = run(eng, "eval", plan, coeffs, B * k, n=n, batch=B)
        for b in (0, C - 1, C):
            assert got[32 * b * k:32 * (b + 1) * k] == multi_eval_bytes(eng, coeffs[32 * b * n:32 * (b + 1) * n], n, 1, xs), b
        # a polynomial longer than a chunk of blocks: its blocks go in several passes, highest first
        n2 = (C + 2) * K + 5
        long = kzg_amd.DeviceBuffer(eng, n2).fill_random(3)
        try:
            want = ctypes.create_string_buffer(32 * k)
            assert eng.lib.kzg_poly_multi_eval(eng.ctx, long.ptr, n2, 1, encode(xs, CAN), k, CAN, L.IN_DEVICE, want) == 0
            out = ctypes.create_string_buffer(32 * k)
            assert eng.lib.kzg_point_tree_eval(eng.ctx, plan.h, long.ptr, n2, 1, CAN, L.IN_DEVICE, out) == 0
            assert out.raw == want.raw
            host = long.download()
            assert eng.lib.kzg_point_tree_eval(eng.ctx, plan.h, host, n2, 1, CAN, 0, out) == 0
            assert out.raw == want.raw
        finally:
            long.free()
        ys = random_blob(B * k, 2)
        got = run(eng, "interpolate", plan, ys, B * k, batch=B)
        for b in (0, C - 1, C):
            assert got[32 * b * k:32 * (b + 1) * k] == run(eng, "interpolate", plan, ys[32 * b * k:32 * (b + 1) * k], k), b
        assert got[: 32 * k] == interpolate_bytes(eng, xs, ys[: 32 * k], 1)
    finally:
        plan.free()


def test_four_threads_share_one_plan(eng):
    k, n = 1500, 4000
    xs = points(k)
    plan = Plan(eng, xs)
    try:
        jobs = [(encode(values(n, 40 + t), CAN), encode(values(k, 50 + t), CAN)) for t in range(4)]
        want = [(multi_eval_bytes(eng, c, n, 1, xs), interpolate_bytes(eng, xs, y, 1)) for c, y in jobs]
        got, errs = [None] * 4, []

        def work(t):
            try:
                for _ in range(3):
                    got[t] = (run(eng, "eval", plan, jobs[t][0], k, n=n), run(eng, "interpolate", plan, jobs[t][1], k))
                    assert got[t] == want[t]
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errs.append(e)
        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errs, errs
        assert got == want
    finally:
        plan.free()


def test_python_mirror(eng):
    xs, rng = points(21), random.Random(9)
    ot = M.SubProductTree.new_from_points(xs)
    with kzg_amd.PointTree.new_from_points(eng, xs) as tree:
        assert tree.shape() == (21, 32, PT.plan_bytes(21), True) and len(tree) == 21
        assert (tree.product.coeffs, tree.product.degree) == (ot.product.coeffs[:22], 21)
        p = [rng.randrange(R) for _ in range(50)]
        want = [M.Polynomial(p).eval(x) for x in xs]
        assert tree.eval(Polynomial(p)) == want and tree.eval(p) == want
        assert tree.eval_batch(p + p[::-1], batch=2) == [want, [M.Polynomial(p[::-1]).eval(x) for x in xs]]
        buf, out = kzg_amd.DeviceBuffer(eng, 50).upload(pack_scalars(p)), kzg_amd.DeviceBuffer(eng, 21)
        try:
            assert tree.eval_batch(buf) == want
            assert tree.eval_batch(buf, out=out) is out and unpack_scalars(out.download()) == want
        finally:
            buf.free()
            out.free()
        cs, ys = [rng.randrange(R) for _ in xs], [rng.randrange(R) for _ in xs]
        assert tree.linear_mod_combination(cs).coeffs == (ot.linear_mod_combination(cs).coeffs + [0] * 21)[:21]
        want = (M.Polynomial.lagrange_interpolation(xs, ys).coeffs + [0] * 21)[:21]
        assert tree.interpolate(ys) == want and tree.interpolate([ys, ys[::-1]])[0] == want
        f = Polynomial.lagrange_interpolation_with_tree(eng, xs, ys, tree)
        assert f.coeffs == want and f == Polynomial.lagrange_interpolation(eng, xs, ys)
        with pytest.raises(ReferencePanic):
            tree.interpolate(ys[:-1])
    assert tree.handle is None
    one = eng.point_tree([7])
    try:
        assert one.interpolate([9]) == [9] and one.product.coeffs == [R - 7, 1]
        q = Polynomial.lagrange_interpolation_with_tree(eng, [7], [9], one)  # the reference's X + (y - x)
        assert (q.coeffs, q.degree) == ([2, 1], 1)
    finally:
        one.close()
    with pytest.raises(ReferencePanic):
        eng.point_tree([])
    with pytest.raises(ReferencePanic):
        eng.point_tree([R])


def test_cpp_wrapper(tmp_path):
    """PointTree and Polynomial::lagrange_interpolation_with_tree of include/kzg_mi355x.hpp: tests/cpp_point_tree_test.cpp against the
    shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_point_tree_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_point_tree_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
