"""kzg_mle_eq / kzg_mle_bind / kzg_mle_eval (kzg_amd/csrc/mle.hip) on bytes against the Python-integer model of tests/mle_model.py.  Every
output has 0xA5 sentinel bytes behind it, checked after every call.  Like the FK20 files this one sorts after the tests that release
the session's contexts, so it uses the module-scoped Engine of tests/fk20_common.py."""
import random

import pytest

from kzg_amd import _lib as L
from tests import mle_model as MM
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture
from tests.mle_gpu_common import A5, CAN, DD, DH, HD, HH, MONT, PAD, SH, Buf, Options, data, enc, ptrs

pytestmark = pytest.mark.gpu

R = MM.R


# ---- eq --------------------------------------------------------------------------------------------------------------------------------
def eq_gpu(eng, point, sfmt, dev):
    m = len(point)
    out = Buf(eng, 32 << m, dev)
    try:
        rc = eng.lib.kzg_mle_eq(eng.ctx, enc(point, sfmt) or None, m, sfmt, L.OUT_DEVICE if dev else 0, out.addr)
        assert rc == 0, eng.last_error()
        return out.body()
    finally:
        out.free()


def special_point(rng, m):
    """random coordinates with 0, 1 and r - 1 among them"""
    pt = [rng.randrange(R) for _ in range(m)]
    for j, v in zip(rng.sample(range(m), min(m, 3)), (0, 1, R - 1)):
        pt[j] = v
    return pt


# (m, mle_local_log, mle_block): both sides of the in-workgroup / global boundary at 10 levels (default) and, by option, at 1, 3 and 5
EQ_CASES = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 0, 0), (6, 0, 64), (7, 0, 128), (10, 0, 0), (11, 0, 0), (13, 0, 0),
            (1, 1, 0), (2, 1, 64), (3, 3, 0), (4, 3, 64), (5, 5, 128), (6, 5, 0), (7, 5, 64), (13, 3, 64), (12, 10, 256)]


@pytest.mark.parametrize("m,local,block", EQ_CASES)
def test_eq_table(eng, m, local, block):
    rng = random.Random(8100 + 16 * m + local)
    pt = special_point(rng, m)
    want = MM.eq(pt)
    with Options(eng, mle_local_log=local, mle_block=block):
        for sfmt, dev in ((CAN, False), (MONT, True), (CAN, True), (MONT, False))[:4 if m <= 7 else 2]:
            assert eq_gpu(eng, pt, sfmt, dev) == enc(want, sfmt), (sfmt, dev)


@pytest.mark.parametrize("m,local", [(1, 0), (6, 0), (6, 3), (12, 0)])
def test_eq_at_a_corner_is_an_indicator(eng, m, local):
    rng = random.Random(8200 + m)
    pt = [rng.randrange(2) for _ in range(m)]
    idx = sum(b << j for j, b in enumerate(pt))
    with Options(eng, mle_local_log=local):
        for sfmt in (CAN, MONT):
            assert eq_gpu(eng, pt, sfmt, True) == enc([int(i == idx) for i in range(1 << m)], sfmt)


def test_eq_refusals_write_nothing(eng):
    out = Buf(eng, 64, False)
    lib, ctx = eng.lib, eng.ctx
    assert lib.kzg_mle_eq(ctx, enc([R], CAN), 1, CAN, 0, out.addr) == SH                  # a coordinate not below r
    assert lib.kzg_mle_eq(ctx, enc([R], CAN), 1, MONT, 0, out.addr) == SH                 # (the limbs, whatever the format)
    assert lib.kzg_mle_eq(ctx, None, 1, CAN, 0, out.addr) == SH
    assert lib.kzg_mle_eq(ctx, enc([1], CAN), 1, CAN, 0, None) == SH
    assert lib.kzg_mle_eq(ctx, enc([1], CAN), 1, 2, 0, out.addr) == SH
    assert lib.kzg_mle_eq(ctx, enc([1] * 29, CAN), 29, CAN, 0, out.addr) == SH
    assert out.untouched()
    assert lib.kzg_mle_eq(ctx, None, 0, CAN, 0, out.addr) == 0 and out.raw()[:32] == enc([1], CAN) and out.raw()[32:] == A5 * (32 + PAD)


# ---- bind ------------------------------------------------------------------------------------------------------------------------------
def bind_case(eng, rng, n, n_cols, rho, sfmt, flags, in_place):
    in_dev, out_dev = bool(flags & L.IN_DEVICE), bool(flags & L.OUT_DEVICE)
    cols = [data(rng, n, sfmt) for _ in range(n_cols)]
    blobs = [enc(c, sfmt) for c in cols]
    cb = [Buf(eng, 32 * n, in_dev, b) for b in blobs]
    ob = cb if in_place else [Buf(eng, 16 * n, out_dev) for _ in range(n_cols)]
    try:
        rc = eng.lib.kzg_mle_bind(eng.ctx, ptrs(cb), n_cols, n, enc([rho], sfmt), sfmt, flags, ptrs(ob))
        assert rc == 0, eng.last_error()
        for c in range(n_cols):
            want = enc(MM.bind(cols[c], rho), sfmt)
            if in_place:
                assert cb[c].body() == want + blobs[c][16 * n:], "in place: the folded half, and the upper half byte for byte as it was"
            else:
                assert ob[c].body() == want and cb[c].untouched()
    finally:
        for b in cb + ([] if in_place else ob):
            b.free()


@pytest.mark.parametrize("n", [2, 4, 128, 1 << 11, 1 << 13])
def test_bind(eng, n):
    rng = random.Random(8300 + n)
    # (n_cols, rho, sfmt, flags, in place, mle_block)
    cases = [(1, rng.randrange(R), CAN, HH, False, 0), (3, rng.randrange(R), MONT, DD, True, 0), (17, rng.randrange(R), CAN, DD, False, 64),
             (3, 0, CAN, DD, True, 128), (3, 1, MONT, HH, True, 0), (1, 1, CAN, DH, False, 0), (3, 0, MONT, HD, False, 64),
             (17, R - 1, MONT, DD, True, 0), (1, rng.randrange(R), CAN, HH, True, 256)]
    for n_cols, rho, sfmt, flags, in_place, block in cases:
        with Options(eng, mle_block=block):
            bind_case(eng, rng, n, n_cols, rho, sfmt, flags, in_place)


@pytest.mark.parametrize("dev", [False, True])
def test_bind_rejects_every_overlap_and_writes_nothing(eng, dev):
    rng = random.Random(8400)
    n, flags = 8, (DD if dev else HH)
    cols = [Buf(eng, 32 * n, dev, enc(data(rng, n, CAN), CAN)) for _ in range(3)]
    outs = [Buf(eng, 16 * n + 64, dev) for _ in range(3)]
    rho = enc([5], CAN)
    lib, ctx = eng.lib, eng.ctx

    def refused(cp, op, n_cols=3, n_=n, rho_=rho, sfmt=CAN):
        assert lib.kzg_mle_bind(ctx, cp, n_cols, n_, rho_, sfmt, flags, op) == SH
        assert all(b.untouched() for b in cols + outs)

    good_c, good_o = ptrs(cols), ptrs(outs)
    refused(good_c, ptrs([outs[0], cols[2], outs[2]]))                             # an output is another column
    refused(good_c, ptrs([cols[0].addr + 16 * n, outs[1], outs[2]]))               # the upper half of its own column
    refused(good_c, ptrs([cols[0].addr + 32, outs[1], outs[2]]))                   # its own column, shifted by one element
    refused(good_c, ptrs([outs[0], outs[1], cols[0].addr + 32 * n - 32]))          # the last element of another column
    refused(good_c, ptrs([outs[0], outs[0], outs[2]]))                             # two outputs are one buffer
    refused(good_c, ptrs([outs[0], outs[0].addr + 16 * n - 32, outs[2]]))          # ... or share one element
    refused(ptrs([cols[0], cols[0], cols[2]]), ptrs([cols[0], cols[0], outs[2]]))  # one column twice, in place
    refused(ptrs([cols[0], cols[0].addr + 32, cols[2]]), ptrs([cols[0], outs[1], outs[2]]))   # in place under another column's feet
    refused(good_c, good_o, n_=6)
    refused(good_c, good_o, n_=1)
    refused(good_c, good_o, n_=0)
    refused(good_c, good_o, n_=1 << 29)
    refused(good_c, good_o, n_cols=0)
    refused(good_c, good_o, n_cols=4097)
    refused(good_c, good_o, rho_=enc([R], CAN))
    refused(good_c, good_o, rho_=None)
    refused(good_c, good_o, sfmt=7)
    refused(None, good_o)
    refused(good_c, None)
    refused(ptrs([cols[0], None, cols[2]]), good_o)
    refused(good_c, ptrs([outs[0], outs[1], None]))
    assert lib.kzg_mle_bind(ctx, good_c, 1, n, rho, CAN, flags, good_o) == 0, eng.last_error()
    for b in cols + outs:
        b.free()


def test_bind_outputs_back_to_back(eng):
    rng = random.Random(8450)
    n = 16
    vals = [data(rng, n, MONT) for _ in range(2)]
    cols = [Buf(eng, 32 * n, True, enc(v, MONT)) for v in vals]
    out = Buf(eng, 2 * 16 * n, True)
    rho = rng.randrange(R)
    assert eng.lib.kzg_mle_bind(eng.ctx, ptrs(cols), 2, n, enc([rho], MONT), MONT, DD, ptrs([out.addr, out.addr + 16 * n])) == 0, eng.last_error()
    assert out.body() == enc(MM.bind(vals[0], rho) + MM.bind(vals[1], rho), MONT)
    for b in cols + [out]:
        b.free()


# ---- eval ------------------------------------------------------------------------------------------------------------------------------
def eval_gpu(eng, tables, m, batch, point, sfmt, flags, with_q):
    """(ys, quotients or None) as bytes; the tables must be unchanged afterwards"""
    n = 1 << m
    tb = Buf(eng, 32 * n * batch, bool(flags & L.IN_DEVICE), enc(tables, sfmt))
    ys = Buf(eng, 32 * batch, False)
    qb = Buf(eng, max(32 * (n - 1) * batch, 32), bool(flags & L.OUT_DEVICE)) if with_q else None
    try:
        rc = eng.lib.kzg_mle_eval(eng.ctx, tb.addr, m, batch, enc(point, sfmt) or None, sfmt, flags, ys.addr, qb.addr if with_q else None)
        assert rc == 0, eng.last_error()
        assert tb.untouched(), "the inputs were written"
        return ys.body(), (qb.body()[:32 * (n - 1) * batch] if with_q else None)
    finally:
        for b in (tb, ys) + ((qb,) if with_q else ()):
            b.free()


# (m, batch, mle_local_log, mle_eval_chunk, mle_block)
EVAL_CASES = [(0, 1, 0, 0, 0), (0, 3, 0, 1, 0), (1, 1, 0, 0, 0), (1, 3, 0, 2, 64), (2, 1, 0, 0, 0), (2, 3, 2, 1, 0), (3, 1, 2, 0, 64), (3, 3, 3, 2, 0),
              (7, 1, 0, 0, 0), (7, 3, 5, 1, 128), (7, 3, 7, 2, 0), (7, 1, 6, 0, 64), (12, 1, 0, 0, 0), (12, 3, 0, 2, 0), (12, 3, 9, 1, 64), (11, 3, 10, 0, 0),
              (10, 3, 0, 0, 0)]


@pytest.mark.parametrize("m,batch,local,chunk,block", EVAL_CASES)
def test_eval_with_and_without_quotients(eng, m, batch, local, chunk, block):
    rng = random.Random(8500 + 32 * m + batch + local)
    n = 1 << m
    pt = special_point(rng, m) if m >= 3 else [rng.randrange(R) for _ in range(m)]
    eq = MM.eq(pt)
    for sfmt, flags in ((CAN, HH), (MONT, DD)) if m > 7 else ((CAN, HH), (MONT, DD), (CAN, DH), (MONT, HD)):
        tables = data(rng, n * batch, sfmt)
        model = [MM.evaluate(tables[b * n:(b + 1) * n], pt) for b in range(batch)]
        # the evaluation is the dot product with the eq table
        assert [y for y, _ in model] == [sum(e * f for e, f in zip(eq, tables[b * n:(b + 1) * n])) % R for b in range(batch)]
        with Options(eng, mle_local_log=local, mle_eval_chunk=chunk, mle_block=block):
            ys, q = eval_gpu(eng, tables, m, batch, pt, sfmt, flags, True)
            assert ys == enc([y for y, _ in model], sfmt), (sfmt, flags)
            assert q == enc([v for _, qs in model for v in qs], sfmt), (sfmt, flags)
            ys2, _ = eval_gpu(eng, tables, m, batch, pt, sfmt, flags, False)
            assert ys2 == ys


def test_eval_agrees_with_the_eq_table_of_the_device(eng):
    rng = random.Random(8600)
    m = 9
    pt = [rng.randrange(R) for _ in range(m)]
    f = [rng.randrange(R) for _ in range(1 << m)]
    e = eq_gpu(eng, pt, CAN, True)
    dot = sum(int.from_bytes(e[32 * i:32 * i + 32], "little") * f[i] for i in range(1 << m)) % R
    ys, _ = eval_gpu(eng, f, m, 1, pt, CAN, DH, False)
    assert ys == enc([dot], CAN)


def test_eval_refusals_write_nothing(eng):
    tb = Buf(eng, 32 * 4, False, enc([1, 2, 3, 4], CAN))
    ys, qb = Buf(eng, 32, False), Buf(eng, 96, False)
    lib, ctx = eng.lib, eng.ctx
    pt = enc([5, 6], CAN)
    for rc in (lib.kzg_mle_eval(ctx, None, 2, 1, pt, CAN, 0, ys.addr, qb.addr), lib.kzg_mle_eval(ctx, tb.addr, 2, 1, None, CAN, 0, ys.addr, qb.addr),
               lib.kzg_mle_eval(ctx, tb.addr, 2, 1, pt, CAN, 0, None, qb.addr), lib.kzg_mle_eval(ctx, tb.addr, 2, 1, enc([5, R], CAN), CAN, 0, ys.addr, qb.addr),
               lib.kzg_mle_eval(ctx, tb.addr, 2, 1, pt, 3, 0, ys.addr, qb.addr), lib.kzg_mle_eval(ctx, tb.addr, 29, 1, pt, CAN, 0, ys.addr, qb.addr),
               lib.kzg_mle_eval(ctx, tb.addr, 2, 1 << 60, pt, CAN, 0, ys.addr, qb.addr)):
        assert rc == SH
    assert lib.kzg_mle_eval(ctx, None, 2, 0, None, CAN, 0, None, None) == 0              # batch == 0: nothing to do, nothing touched
    assert ys.untouched() and qb.untouched() and tb.untouched()
    for b in (tb, ys, qb):
        b.free()


def test_python_mirrors(eng):
    rng = random.Random(8700)
    m = 5
    pt = [rng.randrange(R) for _ in range(m)]
    f = [rng.randrange(R) for _ in range(2 << m)]
    assert eng.mle_eq(pt) == MM.eq(pt)
    ys, qs = eng.mle_eval(f, pt, batch=2, quotients=True)
    model = [MM.evaluate(f[:1 << m], pt), MM.evaluate(f[1 << m:], pt)]
    assert ys == [model[0][0], model[1][0]] and qs == [model[0][1], model[1][1]] and eng.mle_eval(f, pt, batch=2) == ys
    assert eng.mle_bind([f[:1 << m], f[1 << m:]], pt[-1]) == [MM.bind(f[:1 << m], pt[-1]), MM.bind(f[1 << m:], pt[-1])]
    import kzg_amd
    buf = eng.alloc_scalars(1 << m, L.FR_MONT).upload(enc(f[:1 << m], MONT))
    out = eng.alloc_scalars(1 << m, L.FR_MONT)
    try:
        assert eng.mle_eq(pt, out=out) is out and out.download() == enc(MM.eq(pt), MONT)
        assert eng.mle_eval(buf, pt) == [model[0][0]]
        eng.mle_bind([buf], pt[-1])
        assert buf.download(1 << (m - 1)) == enc(MM.bind(f[:1 << m], pt[-1]), MONT)
        assert kzg_amd.sumcheck.prove is not None
    finally:
        buf.free()
        out.free()
