"""kzg_lookup_setup / kzg_lookup_count / kzg_logup_terms (kzg_amd/csrc/lookup.hip) on bytes against the Python-integer model of
tests/lookup_model.py.  Every output buffer, host or device, carries 0xA5 sentinel bytes behind its last element, and they are checked
after every call.  Like the FK20 files this one sorts after the tests that release the session's contexts, so it uses the
module-scoped Engine of tests/fk20_common.py."""
import ctypes
import os
import random
import struct
import subprocess
import threading

import pytest

from kzg_amd import _lib as L
from oracle import kzg_model as M
from tests import fr_scan_model as FM
from tests import lookup_model as LM
from tests.fk20_common import MONT_R, SIZE_MAX, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
TOP = 1 << 256
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
DEV = L.IN_DEVICE | L.OUT_DEVICE
SH = L.KZG_ERR_SHAPE
PAD = 64
A5 = b"\xa5"
GUARD = int.from_bytes(A5 * ctypes.sizeof(ctypes.c_size_t), "little")
U32P = ctypes.POINTER(ctypes.c_uint32)
NONE = LM.NONE


def enc(vals, sfmt):
    if sfmt == MONT:
        return b"".join((v * MONT_R % R).to_bytes(32, "little") for v in vals)
    return b"".join((v % R).to_bytes(32, "little") for v in vals)


def words(vals):
    """256-bit words as they are (canonical format, residues not reduced)"""
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def sentinel_buf(nbytes):
    return ctypes.create_string_buffer(A5 * (nbytes + PAD), nbytes + PAD)


def body(buf, nbytes):
    """the first nbytes of a sentinel buffer, after checking that the bytes behind them are untouched"""
    assert buf.raw[nbytes:] == A5 * PAD, "bytes behind the output were written"
    return buf.raw[:nbytes]


def upload(eng, blob):
    p = ctypes.c_void_p()
    assert eng.lib.kzg_dev_alloc(eng.ctx, len(blob) + PAD, ctypes.byref(p)) == 0
    assert eng.lib.kzg_dev_upload(eng.ctx, p, blob + A5 * PAD, len(blob) + PAD) == 0
    return p


def dev_body(eng, p, nbytes):
    raw = dev_download(eng, p, nbytes + PAD)
    assert raw[nbytes:] == A5 * PAD, "bytes behind the device output were written"
    return raw[:nbytes]


def free(eng, *ptrs):
    for p in ptrs:
        assert eng.lib.kzg_dev_free(eng.ctx, p) == 0


def option(eng, key, value):
    assert eng.lib.kzg_ctx_set_option(eng.ctx, key, value) == 0, eng.last_error()


class options:
    """options set for a block and put back to their defaults behind it"""

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, kv

    def __enter__(self):
        for k, v in self.kv.items():
            option(self.eng, k.encode(), v)

    def __exit__(self, *exc):
        for k in self.kv:
            option(self.eng, k.encode(), 0)


def make_plan(eng, blob, n_t, sfmt, dev=False):
    h = ctypes.c_void_p()
    src = upload(eng, blob) if dev else blob
    rc = eng.lib.kzg_lookup_setup(eng.ctx, src, n_t, sfmt, L.IN_DEVICE if dev else 0, ctypes.byref(h))
    assert rc == 0, eng.last_error()
    if dev:
        assert dev_body(eng, src, len(blob)) == blob      # the table stays
        free(eng, src)
    return h


def plan_shape(eng, h):
    n_t, distinct, nbytes = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert eng.lib.kzg_lookup_shape(h, ctypes.byref(n_t), ctypes.byref(distinct), ctypes.byref(nbytes)) == 0
    return n_t.value, distinct.value, nbytes.value


def count_raw(eng, plan, blob, n, batch, n_t, sfmt, dev=False, outs="MIRF"):
    """One kzg_lookup_count with the outputs named in `outs` (Multiplicities, Indices, missing Reports, First missing).  Returns
    (status, (mult bytes, index bytes, missing, first_missing)) with None for an output that was not asked for; such an output's
    buffer is checked to be untouched."""
    nb_m, nb_i = 32 * batch * n_t, 4 * batch * n
    arr = ctypes.c_size_t * (batch + 1)
    miss, first = arr(*[GUARD] * (batch + 1)), arr(*[GUARD] * (batch + 1))
    if dev:
        vals, m, i, flags = upload(eng, blob), dev_buffer(eng, nb_m + PAD), dev_buffer(eng, nb_i + PAD), DEV
    else:
        vals, m, i, flags = blob, sentinel_buf(nb_m), sentinel_buf(nb_i), 0
    rc = eng.lib.kzg_lookup_count(eng.ctx, plan, vals, n, batch, sfmt, flags, m if "M" in outs else None, ctypes.cast(i, U32P) if "I" in outs else None,
                                  miss if "R" in outs else None, first if "F" in outs else None)
    mb, ib = (dev_body(eng, m, nb_m), dev_body(eng, i, nb_i)) if dev else (body(m, nb_m), body(i, nb_i))
    assert miss[batch] == GUARD and first[batch] == GUARD
    if "M" not in outs:
        assert mb == A5 * nb_m
    if "I" not in outs:
        assert ib == A5 * nb_i
    if "R" not in outs:
        assert list(miss) == [GUARD] * (batch + 1)
    if "F" not in outs:
        assert list(first) == [GUARD] * (batch + 1)
    if dev:
        assert dev_body(eng, vals, len(blob)) == blob     # the values stay
        free(eng, vals, m, i)
    return rc, (mb if "M" in outs else None, ib if "I" in outs else None, list(miss[:batch]) if "R" in outs else None,
                list(first[:batch]) if "F" in outs else None)


def count_want(table, vecs, sfmt, outs="MIRF"):
    mults, idxs, miss, first = [], [], [], []
    for v in vecs:
        m, i, c, f = LM.multiplicities(table, v)
        mults += m
        idxs += i
        miss.append(c)
        first.append(SIZE_MAX if f is None else f)
    return (enc(mults, sfmt) if "M" in outs else None, struct.pack("<%dI" % len(idxs), *idxs) if "I" in outs else None,
            miss if "R" in outs else None, first if "F" in outs else None)


def draw(rng, table, n, missing=0.1):
    """n values: rows of the table, and with probability `missing` a fresh residue (not in the table, up to chance 2^-200)"""
    return [rng.randrange(R) if rng.random() < missing else table[rng.randrange(len(table))] for _ in range(n)]


def flat(vecs):
    return [x for v in vecs for x in v]


def check_count(eng, plan, table, vecs, sfmt, dev=False, outs="MIRF"):
    n = len(vecs[0])
    rc, got = count_raw(eng, plan, enc(flat(vecs), sfmt), n, len(vecs), len(table), sfmt, dev, outs)
    assert rc == 0, eng.last_error()
    assert got == count_want(table, vecs, sfmt, outs), (len(table), n, len(vecs), sfmt, dev, outs)
    return got


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", [1, 2, 3, 63, 64, 65, 257, 1000, 4096])
def test_count_shapes(eng, n_t):
    """every n against this table size, batch 1 and 3; the formats of table and values and the residence of the buffers rotate
    through all eight combinations (a plan set up in one format queried in the other among them)"""
    rng = random.Random(9100 + n_t)
    table = [rng.randrange(R) for _ in range(n_t)]
    plans = {(f, d): make_plan(eng, enc(table, f), n_t, f, d) for f in (CAN, MONT) for d in (False, True)}
    assert all(plan_shape(eng, h)[:2] == (n_t, n_t) for h in plans.values())
    k = n_t
    for n in (1, 63, 64, 65, 1000, 5000):
        for batch in (1, 3):
            tf, td, vf, vd = (CAN, MONT)[k & 1], bool(k & 2), (CAN, MONT)[(k >> 2) & 1], bool(k & 8)
            k += 1
            vecs = [draw(rng, table, n) for _ in range(batch)]
            check_count(eng, plans[(tf, td)], table, vecs, vf, vd)
    for h in plans.values():
        eng.lib.kzg_lookup_free(eng.ctx, h)


def test_count_every_combination_once(eng):
    rng = random.Random(9150)
    n_t, n = 257, 1000
    table = [rng.randrange(R) for _ in range(n_t)]
    vecs = [draw(rng, table, n) for _ in range(3)]
    for tf in (CAN, MONT):
        for td in (False, True):
            h = make_plan(eng, enc(table, tf), n_t, tf, td)
            for vf in (CAN, MONT):
                for vd in (False, True):
                    check_count(eng, h, table, vecs, vf, vd)
            eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 2. probe chains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", [5, 64, 300])
def test_one_wrapping_probe_chain(eng, n_t):
    """lookup_hash_bits = 1: every key starts at slot 0, every compare is a full-key compare; values outside the table walk the whole
    chain to its empty end"""
    rng = random.Random(9200 + n_t)
    table = [rng.randrange(R) for _ in range(n_t)]
    with options(eng, lookup_hash_bits=1):
        h = make_plan(eng, enc(table, CAN), n_t, CAN)
    assert plan_shape(eng, h)[:2] == (n_t, n_t)
    for n, batch in ((1, 1), (65, 3), (1000, 2)):
        check_count(eng, h, table, [draw(rng, table, n, 0.3) for _ in range(batch)], MONT if n & 1 else CAN, dev=n == 65)
    eng.lib.kzg_lookup_free(eng.ctx, h)


@pytest.mark.parametrize("hash_bits", [0, 1, 4])
def test_every_slot_full(eng, hash_bits):
    """lookup_spare_log = 1 with 64 distinct keys: 64 slots, all taken; a value outside the table visits each once and comes back
    missing -- the probe loop is bounded by the slot count"""
    rng = random.Random(9300 + hash_bits)
    n_t = 64
    table = [rng.randrange(R) for _ in range(n_t)]
    with options(eng, lookup_spare_log=1, lookup_hash_bits=hash_bits):
        h = make_plan(eng, enc(table, MONT), n_t, MONT)
    assert plan_shape(eng, h) == (n_t, n_t, n_t * 32 + 64 * 8)
    vecs = [draw(rng, table, 1000, 0.5), [rng.randrange(R) for _ in range(1000)], draw(rng, table, 1000, 0.0)]
    got = check_count(eng, h, table, vecs, CAN)
    assert got[2] == [sum(1 for x in v if x not in table) for v in vecs] and got[2][1] == 1000 and got[2][2] == 0
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 3. duplicates -----------------------------------------------------------------------------------------------------------------
def duplicate_tables(rng):
    one = [rng.randrange(R)] * 100
    head = [rng.randrange(R) for _ in range(200)]
    padded = head + [head[-1]] * 56
    half = [rng.randrange(R) for _ in range(500)]
    return {"one value": one, "padded": padded, "pairs far apart": half + half}


@pytest.mark.parametrize("case", ["one value", "padded", "pairs far apart"])
def test_duplicates_in_the_table(eng, case):
    rng = random.Random(9400)
    table = duplicate_tables(rng)[case]
    n_t = len(table)
    own = LM.owners(table)
    vecs = [draw(rng, table, 1000), [table[-1]] * 1000]       # the second: a repeated row only -- its first occurrence owns all of them
    seen = []
    for hash_bits in (0, 0, 1, 1):
        with options(eng, lookup_hash_bits=hash_bits):
            h = make_plan(eng, enc(table, CAN), n_t, CAN)
        assert plan_shape(eng, h)[:2] == (n_t, len(own))
        got = check_count(eng, h, table, vecs, CAN, dev=hash_bits == 1 and len(seen) == 3)
        seen.append(got)
        eng.lib.kzg_lookup_free(eng.ctx, h)
    assert all(g == seen[0] for g in seen)
    mult = [int.from_bytes(seen[0][0][32 * i:32 * i + 32], "little") for i in range(2 * n_t)]
    idx = struct.unpack("<2000I", seen[0][1])
    owners_only = set(own.values())
    assert all(mult[b * n_t + i] == 0 for b in range(2) for i in range(n_t) if i not in owners_only)
    assert all(i == NONE or i in owners_only for i in idx)
    assert idx[1000:] == (table.index(table[-1]),) * 1000 and mult[n_t + table.index(table[-1])] == 1000


# ---- 4. skew -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["all equal", "a row per lane", "two rows", "runs of 64 and 65"])
def test_skewed_values(eng, case):
    rng = random.Random(9500)
    n_t, n = 256, 5000
    table = [rng.randrange(R) for _ in range(n_t)]
    if case == "all equal":
        rows = [77] * n
    elif case == "a row per lane":
        rows = [j % 256 for j in range(n)]
    elif case == "two rows":
        rows = [(3, 200)[j & 1] for j in range(n)]
    else:
        rows, r = [], 0
        while len(rows) < n:          # wave boundaries fall inside the runs
            rows += [r % n_t] * (64 + (r & 1))
            r += 1
        rows = rows[:n]
    h = make_plan(eng, enc(table, CAN), n_t, CAN)
    vec = [table[r] for r in rows]
    hole = list(vec)
    hole[100] = hole[4999] = rng.randrange(R)        # the same with two lanes that count nothing
    check_count(eng, h, table, [vec, hole, vec[::-1]], MONT)
    check_count(eng, h, table, [vec], CAN, dev=True)
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 5. missing values -------------------------------------------------------------------------------------------------------------
def test_missing_values(eng):
    rng = random.Random(9600)
    n_t, n = 300, 1000
    table = [rng.randrange(R) for _ in range(n_t)]
    h = make_plan(eng, enc(table, CAN), n_t, CAN)
    full = [draw(rng, table, n, 0.0) for _ in range(3)]
    for at in ((0,), (n - 1,), (n // 2,), (0, n - 1), (n // 2, n // 2 + 64, n - 1)):
        vecs = [list(v) for v in full]
        for j in at:
            vecs[1][j] = rng.randrange(R)          # vector 1 of 3 only
        vecs[2][at[-1]] = rng.randrange(R)         # and the last of them in vector 2
        for sfmt, dev in ((CAN, False), (MONT, True)):
            m, i, miss, first = check_count(eng, h, table, vecs, sfmt, dev)
            assert miss == [0, len(at), 1] and first == [SIZE_MAX, at[0], at[-1]]
            idx = struct.unpack("<%dI" % (3 * n), i)
            assert all(idx[n + j] == NONE for j in at) and idx[2 * n + at[-1]] == NONE and sum(1 for x in idx if x == NONE) == len(at) + 1
            # the multiplicities count the found values
            mult = [int.from_bytes(m[32 * k:32 * k + 32], "little") for k in range(3 * n_t)]
            if sfmt == CAN:
                assert [sum(mult[b * n_t:(b + 1) * n_t]) for b in range(3)] == [n, n - len(at), n - 1]
            # one reporting pointer is enough for KZG_OK
            for outs in ("MIR", "MIF"):
                rc, got = count_raw(eng, h, enc(flat(vecs), sfmt), n, 3, n_t, sfmt, dev, outs)
                assert rc == 0 and got == count_want(table, vecs, sfmt, outs)
            # none: KZG_ERR_SHAPE, and the other outputs are still written in full
            rc, got = count_raw(eng, h, enc(flat(vecs), sfmt), n, 3, n_t, sfmt, dev, "MI")
            assert rc == SH and got == count_want(table, vecs, sfmt, "MI")
    rc, got = count_raw(eng, h, enc(flat(full), CAN), n, 3, n_t, CAN, False, "MI")      # nothing missing, nothing to report
    assert rc == 0 and got == count_want(table, full, CAN, "MI")
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 6. residues -------------------------------------------------------------------------------------------------------------------
def test_canonical_words_count_as_their_residue(eng):
    """t + r and, where it fits in 256 bits, t + 2r match t, in the table and in the values; the zero residue is given as 0 and as r"""
    rng = random.Random(9700)
    small = [rng.randrange(1, TOP - 2 * R) for _ in range(20)]        # t + 2r fits
    large = [rng.randrange(TOP - 2 * R, R) for _ in range(20)]
    res = [0] + small + large
    lifts = lambda t: [t, t + R] + ([t + 2 * R] if t + 2 * R < TOP else [])          # noqa: E731
    for zero_word in (0, R, 2 * R):
        table_words = [zero_word] + [lifts(t)[k % len(lifts(t))] for k, t in enumerate(res[1:])]
        assert [w % R for w in table_words] == res
        h = make_plan(eng, words(table_words), len(res), CAN)
        assert plan_shape(eng, h)[:2] == (len(res), len(res))
        value_words = [w for t in res for w in lifts(t)] + [R - 1, TOP - 1]            # the last two are in no table
        want = count_want(res, [value_words], CAN)
        assert want[2] == [2] and want[3] == [len(value_words) - 2]
        rc, got = count_raw(eng, h, words(value_words), len(value_words), 1, len(res), CAN)
        assert rc == 0 and got == want
        # the same residues in Montgomery form
        check_count(eng, h, res, [[w % R for w in value_words]], MONT)
        eng.lib.kzg_lookup_free(eng.ctx, h)
    # a table that holds one residue under three words has one distinct key
    h = make_plan(eng, words([5, 5 + R, 5 + 2 * R, 0, R]), 5, CAN)
    assert plan_shape(eng, h)[:2] == (5, 2)
    rc, got = count_raw(eng, h, words([5 + 2 * R, 2 * R, 5, 6]), 4, 1, 5, CAN)
    assert rc == 0 and got == (enc([2, 0, 0, 1, 0], CAN), struct.pack("<4I", 0, 3, 0, NONE), [1], [3])
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 7. optional outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outs", ["M", "I", "R", "F"])
def test_each_output_alone(eng, outs):
    rng = random.Random(9800)
    n_t, n = 65, 1000
    table = [rng.randrange(R) for _ in range(n_t)]
    h = make_plan(eng, enc(table, CAN), n_t, CAN)
    clean, holes = [draw(rng, table, n, 0.0) for _ in range(2)], [draw(rng, table, n, 0.2) for _ in range(2)]
    for dev in (False, True):
        check_count(eng, h, table, clean, CAN, dev, outs)
        rc, got = count_raw(eng, h, enc(flat(holes), MONT), n, 2, n_t, MONT, dev, outs)
        assert rc == (0 if outs in "RF" else SH) and got == count_want(table, holes, MONT, outs)
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 8. staging and chunks ---------------------------------------------------------------------------------------------------------
def test_staged_pieces_and_vector_chunks(eng):
    """three scalars per staged piece, one vector per chunk: the same bytes as the defaults"""
    rng = random.Random(9900)
    n_t, n, batch = 50, 100, 3
    table = [rng.randrange(R) for _ in range(n_t // 2)] * 2
    vecs = [draw(rng, table, n) for _ in range(batch)]
    h0 = make_plan(eng, enc(table, CAN), n_t, CAN)
    default = check_count(eng, h0, table, vecs, CAN)
    with options(eng, lookup_stage=96, lookup_chunk=1):
        h1 = make_plan(eng, enc(table, MONT), n_t, MONT)
        assert plan_shape(eng, h1) == plan_shape(eng, h0)
        for h in (h0, h1):
            assert check_count(eng, h, table, vecs, CAN) == default
            assert check_count(eng, h, table, vecs, CAN, dev=True) == default
            for outs in ("M", "I"):
                check_count(eng, h, table, [draw(rng, table, n, 0.0) for _ in range(batch)], MONT, False, outs)
    with options(eng, lookup_chunk=2):
        assert check_count(eng, h1, table, vecs, CAN, dev=True) == default
    for h in (h0, h1):
        eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 9. a whole grid ---------------------------------------------------------------------------------------------------------------
def test_large_table_and_values_on_the_device(eng):
    rng = random.Random(10000)
    n_t, n = 1 << 16, 1 << 18
    table = [rng.randrange(R) for _ in range(3 * n_t // 4)]
    table += [table[rng.randrange(len(table))] for _ in range(n_t // 4)]      # a quarter of the rows are duplicates
    rng.shuffle(table)
    hot = [table[rng.randrange(n_t)] for _ in range(16)]
    vec = [table[rng.randrange(n_t)] for _ in range(n // 2)] + [hot[rng.randrange(16)] for _ in range(n // 2)]
    rng.shuffle(vec)
    h = make_plan(eng, enc(table, CAN), n_t, CAN, dev=True)
    assert plan_shape(eng, h)[:2] == (n_t, len(set(table)))
    m, i, miss, first = check_count(eng, h, table, [vec], CAN, dev=True)
    assert miss == [0] and first == [SIZE_MAX]
    eng.lib.kzg_lookup_free(eng.ctx, h)


# ---- 10. statuses ------------------------------------------------------------------------------------------------------------------
def test_shape_errors_touch_nothing(eng):
    lib, ctx = eng.lib, eng.ctx
    rng = random.Random(10100)
    n_t, n = 9, 20
    table = [rng.randrange(R) for _ in range(n_t)]
    blob_t, blob_v = enc(table, CAN), enc(draw(rng, table, 2 * n), CAN)
    plan = make_plan(eng, blob_t, n_t, CAN)
    m, i = sentinel_buf(32 * 2 * n_t), sentinel_buf(4 * 2 * n)
    ip = ctypes.cast(i, U32P)
    miss, first = (ctypes.c_size_t * 2)(GUARD, GUARD), (ctypes.c_size_t * 2)(GUARD, GUARD)
    out, zd = sentinel_buf(32 * 2 * n), (ctypes.c_int * 2)(-7, -7)
    h = ctypes.c_void_p(0x1234)
    hp = ctypes.byref(h)
    beta = enc([5], CAN)
    big, huge = (1 << 28) + 1, SIZE_MAX >> 8
    calls = [
        lambda: lib.kzg_lookup_setup(ctx, blob_t, n_t, 2, 0, hp),                                   # unknown format
        lambda: lib.kzg_lookup_setup(ctx, blob_t, 0, CAN, 0, hp),                                   # n_t == 0
        lambda: lib.kzg_lookup_setup(ctx, blob_t, (1 << 26) + 1, CAN, 0, hp),                       # n_t > 2^26
        lambda: lib.kzg_lookup_setup(ctx, None, n_t, CAN, 0, hp),
        lambda: lib.kzg_lookup_setup(ctx, blob_t, n_t, CAN, 0, None),
        lambda: lib.kzg_lookup_setup(None, blob_t, n_t, CAN, 0, hp),
        lambda: lib.kzg_lookup_count(None, plan, blob_v, n, 2, CAN, 0, m, ip, miss, first),
        lambda: lib.kzg_lookup_count(ctx, None, blob_v, n, 2, CAN, 0, m, ip, miss, first),          # NULL plan
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, n, 2, 2, 0, m, ip, miss, first),            # unknown format
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, 0, 2, CAN, 0, m, ip, miss, first),          # n == 0 with batch > 0
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, big, 1, CAN, 0, m, ip, miss, first),        # n > 2^28
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, 1 << 28, huge, CAN, 0, m, ip, miss, first),  # batch x n x 32 beyond size_t
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, 1, SIZE_MAX >> 7, CAN, 0, m, ip, miss, first),  # batch x n_t x 32 beyond size_t
        lambda: lib.kzg_lookup_count(ctx, plan, None, n, 2, CAN, 0, m, ip, miss, first),            # NULL values
        lambda: lib.kzg_lookup_count(ctx, plan, blob_v, n, 2, CAN, 0, None, None, None, None),      # every output NULL
        lambda: lib.kzg_logup_terms(None, blob_v, blob_v, blob_v, beta, n, 1, 2, CAN, 0, out, zd),
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, n, 1, 2, 2, 0, out, zd),     # unknown format
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, 0, 1, 2, CAN, 0, out, zd),   # n == 0
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, big, 1, 1, CAN, 0, out, zd),
        lambda: lib.kzg_logup_terms(ctx, blob_v, None, None, beta, n, 0, 2, CAN, 0, out, zd),       # no columns and no table
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, None, beta, n, 1, 2, CAN, 0, out, zd),     # a table without multiplicities
        lambda: lib.kzg_logup_terms(ctx, blob_v, None, blob_v, beta, n, 1, 2, CAN, 0, out, zd),
        lambda: lib.kzg_logup_terms(ctx, None, blob_v, blob_v, beta, n, 1, 2, CAN, 0, out, zd),     # NULL with work to do
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, None, n, 1, 2, CAN, 0, out, zd),
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, n, 1, 2, CAN, 0, None, zd),
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, words([R]), n, 1, 2, CAN, 0, out, zd),   # beta not below r
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, 1 << 28, huge, 1, CAN, 0, out, zd),
        lambda: lib.kzg_logup_terms(ctx, blob_v, blob_v, blob_v, beta, 1 << 28, 3, huge, CAN, 0, out, zd),
    ]
    for k, call in enumerate(calls):
        assert call() == SH, k
        assert m.raw == A5 * len(m.raw) and i.raw == A5 * len(i.raw) and out.raw == A5 * len(out.raw), k
        assert list(miss) + list(first) == [GUARD] * 4 and list(zd) == [-7, -7] and h.value == 0x1234, k
    # batch == 0: nothing to do, nothing touched (n == 0 goes with it)
    assert lib.kzg_lookup_count(ctx, plan, None, n, 0, CAN, 0, None, None, None, None) == 0
    assert lib.kzg_lookup_count(ctx, plan, None, 0, 0, CAN, 0, m, ip, miss, first) == 0
    assert lib.kzg_logup_terms(ctx, None, None, None, None, n, 1, 0, CAN, 0, None, None) == 0
    assert m.raw == A5 * len(m.raw) and list(miss) + list(first) == [GUARD] * 4
    for key, bad in ((b"lookup_spare_log", 5), (b"lookup_spare_log", -1), (b"lookup_hash_bits", 33), (b"lookup_hash_bits", -1), (b"lookup_stage", 16),
                     (b"lookup_stage", 100), (b"lookup_stage", (64 << 20) + 32), (b"lookup_chunk", -1), (b"lookup_chunk", 65536)):
        assert lib.kzg_ctx_set_option(ctx, key, bad) == SH
    # the context and the plan still compute
    check_count(eng, plan, table, [draw(rng, table, n)], CAN)
    lib.kzg_lookup_free(ctx, plan)
    lib.kzg_lookup_free(ctx, None)


# ---- 11. concurrency ---------------------------------------------------------------------------------------------------------------
def test_four_threads_query_one_plan(eng):
    rng = random.Random(10200)
    n_t = 257
    table = [rng.randrange(R) for _ in range(200)] + [0] * 57
    plan = make_plan(eng, enc(table, CAN), n_t, CAN)
    jobs = []
    for k, n in enumerate((65, 1000, 1000, 5000)):
        vecs = [draw(rng, table, n) for _ in range(1 + k % 2)]
        sfmt = (CAN, MONT)[k & 1]
        jobs.append((enc(flat(vecs), sfmt), n, len(vecs), sfmt, k >= 2, count_want(table, vecs, sfmt)))
    bad = []

    def work(k):
        blob, n, batch, sfmt, dev, want = jobs[k]
        try:
            for _ in range(20):
                if count_raw(eng, plan, blob, n, batch, n_t, sfmt, dev) != (0, want):
                    bad.append(k)
        except BaseException as e:  # noqa: BLE001 -- reported below
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad
    eng.lib.kzg_lookup_free(eng.ctx, plan)


# ---- 12. the terms -----------------------------------------------------------------------------------------------------------------
def terms_raw(eng, cols, table, mult, beta, n, t, batch, sfmt, dev=False, flags_out=True):
    """cols: batch x t x n values or None; table: n or None; mult: batch x n or None.  (status, out bytes, zero_den)"""
    blobs = [enc(x, sfmt) if x is not None else None for x in (cols, table, mult)]
    out = dev_buffer(eng, 32 * n * batch + PAD) if dev else sentinel_buf(32 * n * batch)
    args = [upload(eng, b) if (dev and b is not None) else b for b in blobs]
    zd = (ctypes.c_int * (batch + 1))(*([-7] * (batch + 1)))
    rc = eng.lib.kzg_logup_terms(eng.ctx, args[0], args[1], args[2], enc([beta], sfmt), n, t, batch, sfmt, DEV if dev else 0, out,
                                 zd if flags_out else None)
    assert zd[batch] == -7 and (flags_out or list(zd[:batch]) == [-7] * batch)
    got = dev_body(eng, out, 32 * n * batch) if dev else body(out, 32 * n * batch)
    if dev:
        for a, b in zip(args, blobs):
            if b is not None:
                assert dev_body(eng, a, len(b)) == b        # the inputs stay
                free(eng, a)
        free(eng, out)
    return rc, got, list(zd[:batch])


def terms_want(cols, table, mult, beta, n, t, batch, sfmt):
    outs, flags = [], []
    for b in range(batch):
        o, z = LM.logup_terms([cols[(b * t + j) * n:(b * t + j + 1) * n] for j in range(t)], table, mult[b * n:(b + 1) * n] if mult is not None else None, beta)
        outs += o
        flags.append(z)
    return enc(outs, sfmt), flags


@pytest.mark.parametrize("n", [1, 7, 300, 2049])
def test_logup_terms(eng, n):
    rng = random.Random(10300 + n)
    beta = rng.randrange(R)
    table = [rng.randrange(R) for _ in range(n)]
    k = 0
    for t in (0, 1, 3):
        for batch in (1, 2):
            cols = [rng.randrange(R) for _ in range(batch * t * n)]
            mult = [rng.randrange(1 << 28) if rng.random() < 0.7 else rng.randrange(R) for _ in range(batch * n)]
            sides = [(table, mult)] + ([(None, None)] if t else [])
            for tb, mu in sides:
                ints = terms_want(cols, tb, mu, beta, n, t, batch, CAN)          # the model once per shape
                for sfmt in (CAN, MONT):
                    want = (0, enc([int.from_bytes(ints[0][32 * i:32 * i + 32], "little") for i in range(batch * n)], sfmt), ints[1])
                    dev = bool(k & 1)
                    k += 1
                    assert terms_raw(eng, cols if t else None, tb, mu, beta, n, t, batch, sfmt, dev) == want, (n, t, batch, sfmt, dev, tb is None)
                    if n == 300:         # the other residence too
                        assert terms_raw(eng, cols if t else None, tb, mu, beta, n, t, batch, sfmt, not dev) == want


def test_logup_terms_zero_denominators(eng):
    rng = random.Random(10400)
    n, t, batch = 300, 3, 2
    beta = rng.randrange(1, R)
    table = [rng.randrange(R) for _ in range(n)]
    mult = [rng.randrange(100) for _ in range(batch * n)]
    for where in ("column", "table"):
        cols = [rng.randrange(R) for _ in range(batch * t * n)]
        tab = list(table)
        if where == "column":
            cols[(1 * t + 2) * n + 77] = R - beta           # vector 1 of 2, column 2
            flags = [0, 1]
        else:
            tab[n - 1] = R - beta                           # the table is shared: both vectors
            flags = [1, 1]
        for sfmt, dev in ((CAN, False), (MONT, True)):
            want = terms_want(cols, tab, mult, beta, n, t, batch, sfmt)
            assert want[1] == flags
            rc, out, zd = terms_raw(eng, cols, tab, mult, beta, n, t, batch, sfmt, dev)
            assert (rc, out, zd) == (0, want[0], flags)
            assert out[32 * n:] == bytes(32 * n) and (flags[0] or out[:32 * n] != bytes(32 * n))
            rc, out, _ = terms_raw(eng, cols, tab, mult, beta, n, t, batch, sfmt, dev, flags_out=False)
            assert rc == SH and out == want[0]
    # canonical words of the residue -beta are zero denominators too
    if R - beta + R < TOP:
        blob = words([R - beta + R] + [1] * (n - 1))
        out, zd = sentinel_buf(32 * n), (ctypes.c_int * 1)(-7)
        assert eng.lib.kzg_logup_terms(eng.ctx, blob, None, None, enc([beta], CAN), n, 1, 1, CAN, 0, out, zd) == 0
        assert body(out, 32 * n) == bytes(32 * n) and zd[0] == 1


def test_logup_terms_in_pieces(eng):
    """three denominators per chunk (t + 1 = 4 of them per element: one element at a time) and 33 (eight elements, the last run
    shorter); one vector per chunk of whole vectors: the same bytes as the defaults"""
    rng = random.Random(10500)
    n, t, batch = 37, 3, 3
    beta = rng.randrange(R)
    cols, table, mult = [rng.randrange(R) for _ in range(batch * t * n)], [rng.randrange(R) for _ in range(n)], [rng.randrange(50) for _ in range(batch * n)]
    cols[(2 * t + 1) * n + 36] = R - beta                    # the last element of the last vector
    want = terms_want(cols, table, mult, beta, n, t, batch, CAN)
    assert want[1] == [0, 0, 1]
    for opts in ({"lookup_stage": 96}, {"lookup_stage": 33 * 32}, {"lookup_chunk": 1}, {"lookup_chunk": 2}):
        with options(eng, **opts):
            for dev in (False, True):
                assert terms_raw(eng, cols, table, mult, beta, n, t, batch, CAN, dev) == (0, want[0], want[1]), (opts, dev)
            assert terms_raw(eng, cols, None, None, beta, n, t, batch, CAN)[0] == 0


# ---- 13. end to end ----------------------------------------------------------------------------------------------------------------
def test_logup_argument_end_to_end(eng):
    rng = random.Random(10600)
    n, t = 1024, 3
    rows = [rng.randrange(R) for _ in range(256)]
    table = rows + [rows[-1]] * (n - 256)                    # padded to its domain by repeating the last row
    columns = [[rows[rng.randrange(256)] for _ in range(n)] for _ in range(t)]
    beta = rng.randrange(R)
    m_want = LM.multiplicities(table, flat(columns))[0]
    terms, zd = LM.logup_terms(columns, table, m_want, beta)
    acc_want, total_want = FM.scan(terms, "sum", True)
    assert zd == 0 and total_want == 0 and sum(m_want) == t * n and m_want[256:] == [0] * (n - 256)
    for sfmt in (CAN, MONT):
        plan = make_plan(eng, enc(table, sfmt), n, sfmt)
        assert plan_shape(eng, plan)[:2] == (n, 256)
        d_cols, d_tab = upload(eng, enc(flat(columns), sfmt)), upload(eng, enc(table, sfmt))
        d_m, d_out = dev_buffer(eng, 32 * n + PAD), dev_buffer(eng, 32 * n + PAD)
        # all t columns are one vector of t n values for the count
        assert eng.lib.kzg_lookup_count(eng.ctx, plan, d_cols, t * n, 1, sfmt, DEV, d_m, None, None, None) == 0, eng.last_error()
        assert dev_body(eng, d_m, 32 * n) == enc(m_want, sfmt)
        tot = sentinel_buf(32)
        for bump in (0, 1):
            if bump:                                          # one multiplicity raised by one: the argument no longer balances
                wrong = list(m_want)
                wrong[17] += 1
                free(eng, d_m)
                d_m = upload(eng, enc(wrong, sfmt))
            assert eng.lib.kzg_logup_terms(eng.ctx, d_cols, d_tab, d_m, enc([beta], sfmt), n, t, 1, sfmt, DEV, d_out, None) == 0, eng.last_error()
            assert eng.lib.kzg_fr_scan(eng.ctx, d_out, n, 1, L.SCAN_SUM, 1, sfmt, DEV, d_out, tot) == 0, eng.last_error()
            if bump:
                assert body(tot, 32) != bytes(32)
            else:
                assert body(tot, 32) == bytes(32) and dev_body(eng, d_out, 32 * n) == enc(acc_want, sfmt)
        free(eng, d_cols, d_tab, d_m, d_out)
        eng.lib.kzg_lookup_free(eng.ctx, plan)


def test_python_mirrors(eng):
    import kzg_amd
    rng = random.Random(10700)
    n, t = 1024, 3
    rows = [rng.randrange(R) for _ in range(256)]
    table = rows + [rows[-1]] * (n - 256)
    columns = [[rows[rng.randrange(256)] for _ in range(n)] for _ in range(t)]
    beta = rng.randrange(R)
    m_want = LM.multiplicities(table, flat(columns))[0]
    acc_want, total_want = FM.scan(LM.logup_terms(columns, table, m_want, beta)[0], "sum", True)
    with eng.lookup_table(table) as plan:
        assert isinstance(plan, kzg_amd.LookupTable) and plan.shape()[:2] == (n, 256) and len(plan) == n
        assert eng.logup_accumulator(plan, table, columns, beta) == (m_want, acc_want, 0)
        vals = columns[0][:50] + [rows[0] + 1, rows[1] + 1]
        want = LM.multiplicities(table, vals)
        assert plan.count(vals) == (want[0], [None if i == NONE else i for i in want[1]], [2], [50])
        assert plan.count(vals[:50], n=25)[2:] == ([0, 0], [None, None])
        with pytest.raises(kzg_amd.ReferencePanic):
            plan.count(vals, strict=True)
        buf = kzg_amd.DeviceBuffer(eng, 50, MONT).upload(enc(vals[:50], MONT))
        out = kzg_amd.DeviceBuffer(eng, n, MONT)
        got = plan.count(buf, out=out)
        assert got[0] is out and got[1] is None and out.download() == enc(LM.multiplicities(table, vals[:50])[0], MONT)
        buf.free()
        out.free()
    small_t, small_m = table[:8], [3, 0, 1, 2, 0, 0, 7, 1]
    cols = [c[:8] for c in columns]
    assert eng.logup_terms(flat(cols), 8, t, beta, table=small_t, mult=small_m) == (LM.logup_terms(cols, small_t, small_m, beta)[0], [0])
    assert eng.logup_terms(flat(cols), 8, t, beta) == (LM.logup_terms(cols, None, None, beta)[0], [0])
    assert eng.logup_terms(None, 8, 0, beta, table=small_t, mult=small_m) == (LM.logup_terms([], small_t, small_m, beta)[0], [0])
    cols[1][3] = R - beta
    with pytest.raises(kzg_amd.ReferencePanic):
        eng.logup_terms(flat(cols), 8, t, beta)
    assert eng.logup_terms(flat(cols), 8, t, beta, strict=False) == ([0] * 8, [1])


# ---- 14. the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_wrapper(tmp_path):
    """LookupTable, lookup_count and logup_terms of include/kzg_mi355x.hpp: tests/cpp_lookup_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_lookup_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_lookup_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
