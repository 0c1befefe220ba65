"""kzg_recover_cosets (kzg_amd/csrc/recover.hip): a polynomial from any sufficient subset of its coset values, against the big-int
model (tests/recover_model.py) at small sizes and against the device-generated original at large ones.  Like the FK20 files this
one sorts after the tests that release the session's contexts, so it opens and closes its own module-scoped Engine."""
import ctypes
import itertools
import math
import random
import threading

import numpy as np
import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.api import pack_scalars, unpack_scalars
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import recover_model as RM
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
LEAF = RM.LEAF
A5 = b"\xa5"


def call(eng, log_n, log_l, n, ids, cells, batch=1, sfmt=CAN, flags=0, out_c=True, out_e=True, status=None):
    """(rc, coefficient bytes or None, evaluation bytes or None); out_c / out_e: True = a host buffer, None / False = NULL, else
    the pointer to pass"""
    N = 1 << log_n
    idv = (ctypes.c_size_t * max(len(ids), 1))(*ids)
    c = ctypes.create_string_buffer(32 * n * batch) if out_c is True else (out_c or None)
    e = ctypes.create_string_buffer(32 * N * batch) if out_e is True else (out_e or None)
    rc = eng.lib.kzg_recover_cosets(eng.ctx, log_n, log_l, n, idv, len(ids), cells, batch, sfmt, flags, c, e, status)
    return rc, (c.raw if out_c is True else None), (e.raw if out_e is True else None)


def evals_of(coeffs, N):
    return C.fft(list(coeffs) + [0] * (N - len(coeffs))) if N > 1 else list(coeffs)


def cells_blob(ev, N, l, ids):
    K = N // l
    return pack_scalars([ev[i + t * K] for i in ids for t in range(l)])


def check_exact(eng, log_n, log_l, n, ids, coeffs, ev=None, sfmt=CAN):
    N, l = 1 << log_n, 1 << log_l
    ev = ev if ev is not None else evals_of(coeffs, N)
    rc, c, e = call(eng, log_n, log_l, n, ids, cells_blob(ev, N, l, ids))
    assert rc == 0, (eng.last_error(), log_n, log_l, n, ids[:8])
    assert c == pack_scalars(coeffs) and e == pack_scalars(ev), (log_n, log_l, n, len(ids), ids[:8])


# ---- 1. every subset at N = 16 -----------------------------------------------------------------------------------------------
# (log_l, known, n, part of parts): the subsets of one size are dealt over `parts` cases where there are thousands of them (a call
# costs ~0.4 ms), so that every subset is covered and no case runs longer than a few seconds
SMALL = []
for _log_l in (0, 1, 2):
    for _known in range(1, (16 >> _log_l) + 1):
        for _n in sorted({1, 1 << _log_l, 8}):
            if _known << _log_l >= _n:
                _parts = 4 if math.comb(16 >> _log_l, _known) > 3000 else 1
                SMALL += [(_log_l, _known, _n, _p, _parts) for _p in range(_parts)]


@pytest.mark.parametrize("log_l,known,n,part,parts", SMALL)
def test_every_subset_of_sixteen_points(eng, log_l, known, n, part, parts):
    rng = random.Random(16 * log_l + known)
    N, l = 16, 1 << log_l
    K = N // l
    coeffs = [rng.randrange(R) for _ in range(n)]
    ev = evals_of(coeffs, N)
    per_coset = [pack_scalars([ev[i + t * K] for t in range(l)]) for i in range(K)]
    want_c, want_e = pack_scalars(coeffs), pack_scalars(ev)
    first = True
    for k, sub in enumerate(itertools.combinations(range(K), known)):
        if k % parts != part:
            continue
        ids = list(sub)
        if (k // parts) % 2:
            rng.shuffle(ids)
        if first:  # the model's own output for this shape: the bytes every subset must give
            mc, me, ok = RM.recover(N, l, n, ids, [[ev[i + t * K] for t in range(l)] for i in ids])
            assert ok and pack_scalars(mc) == want_c and pack_scalars(me) == want_e
            first = False
        rc, c, e = call(eng, 4, log_l, n, ids, b"".join(per_coset[i] for i in ids))
        assert rc == 0 and c == want_c and e == want_e, (l, n, ids)


# ---- 2. degenerate shapes ----------------------------------------------------------------------------------------------------
def test_degenerate_shapes(eng):
    rng = random.Random(2)
    check_exact(eng, 0, 0, 1, [0], [rng.randrange(R)])                                  # N = 1
    check_exact(eng, 0, 0, 1, [0], [0])
    for log_n in (1, 5, 13):                                                              # l = N: the one coset
        N = 1 << log_n
        for n in (1, N - 1, N):
            check_exact(eng, log_n, log_n, n, [0], [rng.randrange(R) for _ in range(n)])
    for log_n, log_l in ((6, 0), (6, 2), (13, 4)):                                        # m = 0: interpolation, check active
        N, K = 1 << log_n, 1 << (log_n - log_l)
        ids = rng.sample(range(K), K)
        n = N - 3
        coeffs = [rng.randrange(R) for _ in range(n)]
        check_exact(eng, log_n, log_l, n, ids, coeffs)
        ev = evals_of(coeffs, N)
        ev[5] = (ev[5] + 1) % R
        rc, _, _ = call(eng, log_n, log_l, n, ids, cells_blob(ev, N, 1 << log_l, ids))
        assert rc == L.KZG_ERR_POINT_NOT_ON_POLY
    for log_n, log_l in ((6, 2), (10, 3), (13, 1)):                                       # m = K - 1 with n <= l
        l, K = 1 << log_l, 1 << (log_n - log_l)
        for n in sorted({1, l - 1, l}):
            check_exact(eng, log_n, log_l, n, [rng.randrange(K)], [rng.randrange(R) for _ in range(n)])
    for log_n, log_l in ((3, 0), (8, 8), (9, 3)):                                         # n = 1
        K = 1 << (log_n - log_l)
        check_exact(eng, log_n, log_l, 1, rng.sample(range(K), max(1, K // 3)), [rng.randrange(R)])


# ---- 3. the edges of the product tree ----------------------------------------------------------------------------------------
TREE = [(LEAF - 1, 1), (LEAF, 1), (LEAF + 1, 1), (2 * LEAF + 1, 1), (1 << 11, 1), ((1 << 11) + 1, 1), (1 << 11, 1 << 11)]


@pytest.mark.parametrize("m,n", TREE)
def test_tree_boundaries(eng, m, n):
    # N = 2^12, l = 1: the smallest shapes that cross the leaf / level and the padding edges (n = 1 is the only n that allows
    # m > N / 2).  Compared with the model run through its own padded tree, and with the original polynomial
    rng = random.Random(3000 + m + n)
    N = 1 << 12
    assert RM.padded_roots(m) == {LEAF - 1: LEAF, LEAF: LEAF, LEAF + 1: 2 * LEAF, 2 * LEAF + 1: 4 * LEAF, 1 << 11: 1 << 11,
                                  (1 << 11) + 1: 1 << 12}[m]
    ids = rng.sample(range(N), N - m)
    coeffs = [rng.randrange(R) for _ in range(n)]
    ev = evals_of(coeffs, N)
    mc, me, ok = RM.recover_with_tree(N, 1, n, ids, [[ev[i]] for i in ids])
    rc, c, e = call(eng, 12, 0, n, ids, cells_blob(ev, N, 1, ids))
    assert rc == 0 and ok, eng.last_error()
    assert c == pack_scalars(mc) and e == pack_scalars(me), (m, n)
    assert mc == coeffs and me == ev
    if N - m > n:  # one wrong value is detected
        ev[ids[7]] = (ev[ids[7]] + 1) % R
        assert call(eng, 12, 0, n, ids, cells_blob(ev, N, 1, ids))[0] == L.KZG_ERR_POINT_NOT_ON_POLY


# ---- 4. formats and residency ------------------------------------------------------------------------------------------------
def test_formats_and_residency(eng):
    rng = random.Random(4)
    log_n, log_l, B = 10, 4, 2
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    known = 40
    n = known * l - 7
    ids = rng.sample(range(K), known)
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(B)]
    evs = [evals_of(p, N) for p in polys]
    slack = 96
    for sfmt, conv in ((CAN, lambda v: v), (MONT, lambda v: v * MONT_R % R)):
        blob = b"".join(pack_scalars([conv(ev[i + t * K]) for i in ids for t in range(l)]) for ev in evs)
        want_c = b"".join(pack_scalars([conv(c) for c in p]) for p in polys)
        want_e = b"".join(pack_scalars([conv(v) for v in ev]) for ev in evs)
        din = eng.alloc_scalars(B * known * l, sfmt).upload(blob)
        try:
            for flags in (0, L.IN_DEVICE, L.OUT_DEVICE, L.IN_DEVICE | L.OUT_DEVICE):
                src = din.ptr if flags & L.IN_DEVICE else blob
                for with_c, with_e in ((True, False), (False, True), (True, True)):
                    if not flags & L.OUT_DEVICE:
                        rc, c, e = call(eng, log_n, log_l, n, ids, src, B, sfmt, flags, with_c or None, with_e or None)
                        assert rc == 0 and (c is None or c == want_c) and (e is None or e == want_e), (sfmt, flags, with_c, with_e)
                        continue
                    dc, de = dev_buffer(eng, B * n * 32 + slack), dev_buffer(eng, B * N * 32 + slack)
                    try:
                        rc, _, _ = call(eng, log_n, log_l, n, ids, src, B, sfmt, flags, dc if with_c else None, de if with_e else None)
                        assert rc == 0, eng.last_error()
                        got_c, got_e = dev_download(eng, dc, B * n * 32 + slack), dev_download(eng, de, B * N * 32 + slack)
                        assert got_c == (want_c if with_c else A5 * (B * n * 32)) + A5 * slack, (sfmt, flags, with_c, with_e)
                        assert got_e == (want_e if with_e else A5 * (B * N * 32)) + A5 * slack, (sfmt, flags, with_c, with_e)
                    finally:
                        eng.lib.kzg_dev_free(eng.ctx, dc)
                        eng.lib.kzg_dev_free(eng.ctx, de)
        finally:
            din.free()


def test_python_surface(eng):
    rng = random.Random(5)
    N, l, n = 64, 4, 21
    K = N // l
    ids = rng.sample(range(K), 7)
    coeffs = [rng.randrange(R) for _ in range(n)]
    ev = evals_of(coeffs, N)
    cells = [[ev[i + t * K] for t in range(l)] for i in ids]
    p = eng.recover_cosets(6, 2, n, ids, cells)
    assert isinstance(p, kzg_amd.Polynomial) and p.slice_coeffs() == coeffs
    p, got_ev = eng.recover_cosets(6, 2, n, ids, cells, want_evals=True)
    assert p.slice_coeffs() == coeffs and got_ev == ev
    buf = eng.alloc_scalars(len(ids) * l, MONT).upload(pack_scalars([v * MONT_R % R for c in cells for v in c]))
    try:
        assert eng.recover_cosets(6, 2, n, ids, buf).slice_coeffs() == coeffs
    finally:
        buf.free()
    other = [rng.randrange(R) for _ in range(n)]
    ev2 = evals_of(other, N)
    polys, both = eng.recover_cosets_batch(6, 2, n, ids, [cells, [[ev2[i + t * K] for t in range(l)] for i in ids]], want_evals=True)
    assert [q.slice_coeffs() for q in polys] == [coeffs, other] and both == [ev, ev2]
    cells[3][1] = (cells[3][1] + 1) % R
    with pytest.raises(kzg_amd.PointNotOnPolynomial):
        eng.recover_cosets(6, 2, n, ids, cells)
    with pytest.raises(kzg_amd.ReferencePanic):
        eng.recover_cosets(6, 2, n, ids[:5], cells[:5])  # 5 * 4 < 21
    flat = pack_scalars([v for c in cells for v in c])
    short = eng.alloc_scalars(len(ids) * l - 1)
    try:
        for bad in (flat[:-32], short):  # fewer scalars than batch * known * l: refused before the call could read past them
            with pytest.raises(kzg_amd.ReferencePanic):
                eng.recover_cosets(6, 2, n, ids, bad)
        with pytest.raises(kzg_amd.ReferencePanic):
            eng.recover_cosets_batch(6, 2, n, ids, flat, batch=2)
        with pytest.raises(kzg_amd.ReferencePanic):
            eng.recover_cosets_batch(6, 2, -1, ids, flat, batch=1)
    finally:
        short.free()


# ---- device-generated polynomials --------------------------------------------------------------------------------------------
def device_polys(eng, log_n, n, batch, seed, sfmt):
    """(coefficient bytes batch x n, evaluations as a uint8 array batch x N x 32): kzg_fill_random_fr, zero-padded, kzg_ntt_fr"""
    N = 1 << log_n
    rnd = eng.alloc_scalars(batch * n, sfmt).fill_random(seed)
    coeff = rnd.download()
    rnd.free()
    padded = np.zeros((batch, N, 32), dtype=np.uint8)
    padded[:, :n, :] = np.frombuffer(coeff, dtype=np.uint8).reshape(batch, n, 32)
    buf = eng.alloc_scalars(batch * N, sfmt).upload(padded.tobytes())
    try:
        for b in range(batch):
            rc = eng.lib.kzg_ntt_fr(eng.ctx, ctypes.c_void_p(buf.ptr.value + b * N * 32), log_n, 0, L.IN_DEVICE)
            assert rc == 0, eng.last_error()
        ev = np.frombuffer(buf.download(), dtype=np.uint8).reshape(batch, N, 32)
    finally:
        buf.free()
    return coeff, ev


def gather(ev, log_n, log_l, ids):
    """coset-major cells of every polynomial: batch x known x l x 32 (point m = id + t K)"""
    l, K = 1 << log_l, 1 << (log_n - log_l)
    return np.ascontiguousarray(ev.reshape(ev.shape[0], l, K, 32)[:, :, ids, :].transpose(0, 2, 1, 3))


# ---- 5. a batch of several chunks --------------------------------------------------------------------------------------------
@pytest.mark.limit(300)
def test_batch_across_chunks(eng):
    # 2^14 / 64: chunks of 64, 130 = 64 + 64 + 2; n < known l < N, so the cell (b0 known l), coefficient (b0 n) and evaluation (b0 N)
    # offsets all differ
    rng = random.Random(6)
    log_n, log_l, B = 14, 6, 130
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    assert (RM.chunk_size(N), B % RM.chunk_size(N)) == (64, 2)
    known = 150
    n = known * l - 3
    ids = rng.sample(range(K), known)
    coeff, ev = device_polys(eng, log_n, n, B, 0xC0FFEE, CAN)
    cells = gather(ev, log_n, log_l, ids)
    rc, c, e = call(eng, log_n, log_l, n, ids, cells.tobytes(), B)
    assert rc == 0, eng.last_error()
    assert c == coeff and e == ev.tobytes()
    for b in range(B):
        rc, c1, e1 = call(eng, log_n, log_l, n, ids, cells[b].tobytes())
        assert rc == 0 and c1 == coeff[b * n * 32:(b + 1) * n * 32] and e1 == ev[b].tobytes(), b
    bad = (0, 127, 128)  # polynomial 0, the last of chunk 1, the first of chunk 2
    broken = cells.copy()
    for b in bad:
        broken[b, rng.randrange(known), rng.randrange(l), 0] ^= 1
    status = (ctypes.c_int * B)(*([7] * B))
    rc, c, e = call(eng, log_n, log_l, n, ids, broken.tobytes(), B, status=status)
    assert rc == 0 and [b for b in range(B) if status[b]] == list(bad) and set(status) == {0, 1}
    for b in range(B):
        if b not in bad:
            assert c[b * n * 32:(b + 1) * n * 32] == coeff[b * n * 32:(b + 1) * n * 32] and e[b * N * 32:(b + 1) * N * 32] == ev[b].tobytes(), b
    assert call(eng, log_n, log_l, n, ids, broken.tobytes(), B)[0] == L.KZG_ERR_POINT_NOT_ON_POLY


# ---- 6. recovered polynomials open like the original -------------------------------------------------------------------------
@pytest.mark.limit(300)
def test_round_trip_through_the_prover(eng):
    rng = random.Random(7)
    log_n, log_l = 12, 4
    N, l = 1 << log_n, 1 << log_l
    K = N // l
    n = N // 2 - 1
    gs = kzg_amd.setup(eng, 0x5EED_C05E7, N, g2_len=0).gs
    plan = kzg_amd.FK20CosetPlan(eng, gs, log_n, log_l)
    dc = de = None
    try:
        coeffs = [rng.randrange(R) for _ in range(n)]
        blob = pack_scalars(coeffs)
        w0, r0 = ctypes.create_string_buffer(96 * K), ctypes.create_string_buffer(32 * N)
        assert eng.lib.kzg_witness_cosets_coeff(eng.ctx, plan.handle, blob, n, 1, CAN, 0, w0, L.G1_AFFINE_MONT, r0) == 0
        ev = evals_of(coeffs, N)
        ids = rng.sample(range(K), K // 2)
        cells = cells_blob(ev, N, l, ids)
        dc, de = dev_buffer(eng, n * 32), dev_buffer(eng, N * 32)
        rc, _, _ = call(eng, log_n, log_l, n, ids, cells, 1, CAN, L.OUT_DEVICE, dc, de)
        assert rc == 0, eng.last_error()
        w1, r1 = ctypes.create_string_buffer(96 * K), ctypes.create_string_buffer(32 * N)
        assert eng.lib.kzg_witness_cosets_coeff(eng.ctx, plan.handle, dc, n, 1, CAN, L.IN_DEVICE, w1, L.G1_AFFINE_MONT, r1) == 0
        assert w1.raw == w0.raw and r1.raw == r0.raw
        got = unpack_scalars(dev_download(eng, de, N * 32))
        assert cells_blob(got, N, l, ids) == cells
        w2, r2 = ctypes.create_string_buffer(96 * K), ctypes.create_string_buffer(32 * N)
        assert eng.lib.kzg_witness_cosets_eval(eng.ctx, plan.handle, de, N, 1, CAN, L.IN_DEVICE, w2, L.G1_AFFINE_MONT, r2) == 0
        assert w2.raw == w0.raw and r2.raw == r0.raw
    finally:
        for p in (dc, de):
            if p is not None:
                eng.lib.kzg_dev_free(eng.ctx, p)
        plan.free()
        gs.free()


# ---- 7. large sizes against the device-generated original --------------------------------------------------------------------
@pytest.mark.limit(300)
@pytest.mark.parametrize("log_n,log_l,missing,sfmt", [(20, 6, 8192, CAN), (20, 0, 1 << 19, MONT), (22, 1, (1 << 20) + 5, CAN)])
def test_large_sizes(eng, log_n, log_l, missing, sfmt):
    # (20, 0): the full depth of the tree (2^19 roots); (22, 1): the limit.  n leaves the consistency check a few coefficients
    rng = random.Random(log_n + log_l)
    N, l, K = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
    known = K - missing
    n = known * l - 5
    ids = np.array(sorted(rng.sample(range(K), known)))
    coeff, ev = device_polys(eng, log_n, n, 1, 0xABCD + log_l, sfmt)
    cells = gather(ev, log_n, log_l, ids)
    rc, c, e = call(eng, log_n, log_l, n, ids.tolist(), cells.tobytes(), 1, sfmt)
    assert rc == 0, eng.last_error()
    assert c == coeff
    assert e == ev.tobytes()
    cells[0, known // 2, l - 1, 3] ^= 0x10
    assert call(eng, log_n, log_l, n, ids.tolist(), cells.tobytes(), 1, sfmt, out_e=None)[0] == L.KZG_ERR_POINT_NOT_ON_POLY


# ---- 8. every shape error, with the outputs untouched ------------------------------------------------------------------------
def test_validation(eng):
    log_n, log_l = 4, 1
    N, l, K = 16, 2, 8
    ids = [3, 0, 6, 7]
    n = 8
    cells = pack_scalars(list(range(1, 2 * len(ids) * l + 1)))
    c, e = ctypes.create_string_buffer(A5 * (32 * N * 2), 32 * N * 2), ctypes.create_string_buffer(A5 * (32 * N * 2), 32 * N * 2)
    status = (ctypes.c_int * 2)(9, 9)

    def go(log_n=log_n, log_l=log_l, n=n, ids=ids, known=None, cells=cells, batch=1, sfmt=CAN, out_c=c, out_e=e, ctx=eng.ctx,
           null_ids=False):
        idv = None if null_ids else (ctypes.c_size_t * max(len(ids), 1))(*ids)
        return eng.lib.kzg_recover_cosets(ctx, log_n, log_l, n, idv, len(ids) if known is None else known, cells, batch, sfmt, 0,
                                          out_c, out_e, status)

    S = L.KZG_ERR_SHAPE
    assert go(log_l=5) == S and go(log_n=3, log_l=4) == S                       # log_l > log_n
    assert go(log_n=23, log_l=1) == S and go(log_n=40, log_l=1) == S            # log_n > 22
    assert go(n=0) == S and go(n=N + 1) == S
    assert go(known=0) == S and go(ids=list(range(K)) + [0], n=1) == S          # known == 0, known > K
    assert go(n=len(ids) * l + 1) == S                                          # known l == n - 1
    assert go(ids=[3, 0, 6, K]) == S and go(ids=[3, 0, 6, 1 << 40]) == S        # an id equal to K
    assert go(ids=[3, 0, 6, 3]) == S and go(ids=[3, 3, 6, 7]) == S              # a duplicate id, at the last position too
    assert go(null_ids=True) == S and go(cells=None) == S
    assert go(out_c=None, out_e=None) == S
    assert go(sfmt=7) == S
    assert go(ctx=None) == S
    assert c.raw == A5 * (32 * N * 2) and e.raw == A5 * (32 * N * 2) and list(status) == [9, 9]
    assert go(batch=0) == 0
    assert c.raw == A5 * (32 * N * 2) and e.raw == A5 * (32 * N * 2) and list(status) == [9, 9]
    # the boundary cases that are accepted: known l == n (every input is consistent), one output only
    assert go(n=len(ids) * l) == 0 and list(status) == [0, 9]
    assert go(out_e=None) in (0, L.KZG_ERR_POINT_NOT_ON_POLY) and go(out_c=None) in (0, L.KZG_ERR_POINT_NOT_ON_POLY)
    with pytest.raises(kzg_amd.ReferencePanic):
        eng.recover_cosets(4, 1, 8, [3, 0, 6, 3], cells)


# ---- 9. two threads, one context ---------------------------------------------------------------------------------------------
def test_two_threads_on_one_context(eng):
    rng = random.Random(9)
    log_n, log_l = 13, 3
    N, l, K = 1 << log_n, 8, 1 << 10
    jobs = []
    for known in (600, 777):
        n = known * l - 11
        ids = rng.sample(range(K), known)
        coeffs = [rng.randrange(R) for _ in range(n)]
        ev = evals_of(coeffs, N)
        jobs.append((n, ids, cells_blob(ev, N, l, ids), pack_scalars(coeffs), pack_scalars(ev)))
    results, errors = [[], []], []

    def work(k):
        try:
            n, ids, cells, _, _ = jobs[k]
            for _ in range(4):
                results[k].append(call(eng, log_n, log_l, n, ids, cells))
        except Exception as ex:  # noqa: BLE001 -- reported below
            errors.append(ex)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert len(results[k]) == 4
        for rc, c, e in results[k]:
            assert rc == 0 and c == jobs[k][3] and e == jobs[k][4], k
