"""kzg_fr_scan / kzg_fr_grand_product / kzg_fr_batch_inverse (kzg_amd/csrc/fr_scan.hip, the batch inversion of poly.hip) on bytes against
the Python-integer model of tests/fr_scan_model.py.  Every output buffer carries 0xA5 sentinel bytes behind its last element, and they
are checked after every call.  Like the FK20 files this one sorts after the tests that release the session's contexts, so it uses the
module-scoped Engine of tests/fk20_common.py."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

from kzg_amd import _lib as L
from oracle import kzg_model as M
from tests import fr_scan_model as FM
from tests import residue_lift as RL
from tests.fk20_common import MONT_R, SIZE_MAX, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
PROD, SUM = L.SCAN_PRODUCT, L.SCAN_SUM
OPS = {PROD: "product", SUM: "sum"}
DEV = L.IN_DEVICE | L.OUT_DEVICE
SH = L.KZG_ERR_SHAPE
PAD = 64
A5 = b"\xa5"
MONT_R_INV = pow(MONT_R, -1, R)


def enc(vals, sfmt):
    if sfmt == MONT:
        return b"".join((v * MONT_R % R).to_bytes(32, "little") for v in vals)
    return b"".join((v % R).to_bytes(32, "little") for v in vals)


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


def scan_raw(eng, blob, n, batch, op, excl, sfmt, totals=True):
    """host to host; (out bytes, totals bytes or None)"""
    out, tot = sentinel_buf(32 * n * batch), sentinel_buf(32 * batch)
    rc = eng.lib.kzg_fr_scan(eng.ctx, blob, n, batch, op, excl, sfmt, 0, out, tot if totals else None)
    assert rc == 0, eng.last_error()
    if not totals:
        assert tot.raw == A5 * (32 * batch + PAD)
    return body(out, 32 * n * batch), (body(tot, 32 * batch) if totals else None)


def scan_want(vecs, op, excl, sfmt):
    outs, tots = [], []
    for v in vecs:
        o, t = FM.scan(v, OPS[op], bool(excl))
        outs += o
        tots.append(t)
    return enc(outs, sfmt), enc(tots, sfmt)


def rand_vecs(rng, n, batch):
    return [[rng.randrange(1, R) for _ in range(n)] for _ in range(batch)]


def check_scan(eng, vecs, op, excl, sfmt):
    n = len(vecs[0])
    got = scan_raw(eng, enc([x for v in vecs for x in v], sfmt), n, len(vecs), op, excl, sfmt)
    assert got == scan_want(vecs, op, excl, sfmt), (n, len(vecs), op, excl, sfmt)


# ---- 1. the scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 2047, 2048, 2049, 4097])
def test_scan_default_tile(eng, n):
    rng = random.Random(4100 + n)
    for batch in (1, 3):
        vecs = rand_vecs(rng, n, batch)
        for op in (PROD, SUM):
            for excl in (0, 1):
                for sfmt in (CAN, MONT):
                    check_scan(eng, vecs, op, excl, sfmt)


def test_scan_device_buffers(eng):
    """in == out on the device; host in, device out; device in, host out"""
    rng = random.Random(4200)
    n, batch = 2049, 3
    vecs = rand_vecs(rng, n, batch)
    nb = 32 * n * batch
    for op, excl, sfmt in ((PROD, 0, CAN), (SUM, 1, MONT), (PROD, 1, MONT)):
        blob = enc([x for v in vecs for x in v], sfmt)
        want, want_tot = scan_want(vecs, op, excl, sfmt)
        d = upload(eng, blob)
        tot = sentinel_buf(32 * batch)
        assert eng.lib.kzg_fr_scan(eng.ctx, d, n, batch, op, excl, sfmt, DEV, d, tot) == 0, eng.last_error()
        assert dev_body(eng, d, nb) == want and body(tot, 32 * batch) == want_tot
        o = dev_buffer(eng, nb + PAD)
        assert eng.lib.kzg_fr_scan(eng.ctx, blob, n, batch, op, excl, sfmt, L.OUT_DEVICE, o, None) == 0, eng.last_error()
        assert dev_body(eng, o, nb) == want
        i, h = upload(eng, blob), sentinel_buf(nb)
        assert eng.lib.kzg_fr_scan(eng.ctx, i, n, batch, op, excl, sfmt, L.IN_DEVICE, h, tot) == 0, eng.last_error()
        assert body(h, nb) == want and body(tot, 32 * batch) == want_tot
        assert dev_body(eng, i, nb) == blob          # the input stays
        free(eng, d, o, i)


@pytest.mark.parametrize("tile", [8, 64])
def test_scan_small_tiles_reach_the_carry_boundaries(eng, tile):
    """512 tiles fill the carry workgroup; 512 tile + 1 and 1024 tile + 3 give it two and three partials per thread"""
    rng = random.Random(4300 + tile)
    option(eng, b"fr_scan_tile", tile)
    try:
        for n in (tile - 1, tile, tile + 1, 3 * tile + 5, 512 * tile, 512 * tile + 1, 1024 * tile + 3):
            vecs = rand_vecs(rng, n, 2)
            for op, excl, sfmt in ((PROD, 0, CAN), (PROD, 1, MONT), (SUM, 0, MONT), (SUM, 1, CAN)):
                check_scan(eng, vecs, op, excl, sfmt)
    finally:
        option(eng, b"fr_scan_tile", 0)


def test_scan_large_default_tile(eng):
    """513 tiles of 2048: two partials per carry thread with the real tile"""
    rng = random.Random(4400)
    n = (1 << 20) + 2049
    vec = [rng.randrange(1, R) for _ in range(n)]
    check_scan(eng, [vec], PROD, 0, CAN)


def test_scan_special_values(eng):
    n = 4097
    rng = random.Random(4500)
    for fill in (1, R - 1, 0):
        for op in (PROD, SUM):
            for excl in (0, 1):
                check_scan(eng, [[fill] * n], op, excl, CAN)
                check_scan(eng, [[fill] * n], op, excl, MONT)
    for at in ((0,), (n - 1,), (2047,), (2048,), (0, n - 1)):
        vec = [rng.randrange(1, R) for _ in range(n)]
        for i in at:
            vec[i] = 0
        for excl in (0, 1):
            for sfmt in (CAN, MONT):
                check_scan(eng, [vec, vec[::-1]], PROD, excl, sfmt)
            got, _ = scan_raw(eng, enc(vec, CAN), n, 1, PROD, excl, CAN)
            first = at[0] + excl                      # zero from the first zero on, one element later when exclusive
            assert got[32 * first:] == bytes(32 * (n - first)) and (first == 0 or got[32 * (first - 1):32 * first] != bytes(32))
        check_scan(eng, [vec], SUM, 0, CAN)


@pytest.mark.parametrize("mode", RL.MODES)
def test_scan_canonical_words_count_as_their_residue(eng, mode):
    rng = random.Random(4600)
    n = 2049
    vecs = [RL.base(rng, n), [rng.randrange(1, R) for _ in range(n)]]
    blob = RL.pack([x for v in vecs for x in RL.lift(v, mode)])
    for op in (PROD, SUM):
        for excl in (0, 1):
            assert scan_raw(eng, blob, n, 2, op, excl, CAN) == scan_want(vecs, op, excl, CAN), (mode, op, excl)


def test_scan_totals(eng):
    """the total is the last inclusive element, exclusive or not, with the output on the host or the device, and may be left out"""
    rng = random.Random(4700)
    n, batch = 2049, 3
    vecs = rand_vecs(rng, n, batch)
    blob = enc([x for v in vecs for x in v], CAN)
    for op in (PROD, SUM):
        incl, tot = scan_raw(eng, blob, n, batch, op, 0, CAN)
        assert tot == b"".join(incl[32 * (b * n + n - 1):32 * (b * n + n)] for b in range(batch))
        assert scan_raw(eng, blob, n, batch, op, 1, CAN)[1] == tot
        assert scan_raw(eng, blob, n, batch, op, 0, CAN, totals=False)[0] == incl
        o, t = dev_buffer(eng, 32 * n * batch + PAD), sentinel_buf(32 * batch)
        assert eng.lib.kzg_fr_scan(eng.ctx, blob, n, batch, op, 1, CAN, L.OUT_DEVICE, o, t) == 0
        assert body(t, 32 * batch) == tot
        free(eng, o)


# ---- 2. batch inversion ------------------------------------------------------------------------------------------------------------
def inverse_raw(eng, blob, sfmt):
    n = len(blob) // 32
    out, z = sentinel_buf(32 * n), ctypes.c_size_t(12345)
    assert eng.lib.kzg_fr_batch_inverse(eng.ctx, blob, n, sfmt, 0, out, ctypes.byref(z)) == 0, eng.last_error()
    return body(out, 32 * n), z.value


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097, 70000])
def test_batch_inverse(eng, n):
    rng = random.Random(5100 + n)
    vals = [rng.randrange(1, R) for _ in range(n)]
    inverses = FM.batch_inverse(vals)[0]          # the model once: a zero changes its own inverse only
    for zeros_at in ((), (0,), (n - 1,), (n // 2,), (0, n // 2, n - 1)):
        v, want = list(vals), list(inverses)
        for i in zeros_at:
            v[i] = want[i] = 0
        zeros = len(set(zeros_at))
        for sfmt in (CAN, MONT):
            assert inverse_raw(eng, enc(v, sfmt), sfmt) == (enc(want, sfmt), zeros), (n, zeros_at, sfmt)
    for sfmt in (CAN, MONT):
        assert inverse_raw(eng, bytes(32 * n), sfmt) == (bytes(32 * n), n)
    # the zero count is optional
    out = sentinel_buf(32 * n)
    assert eng.lib.kzg_fr_batch_inverse(eng.ctx, enc(vals, CAN), n, CAN, 0, out, None) == 0
    assert body(out, 32 * n) == enc(inverses, CAN)


@pytest.mark.parametrize("mode", RL.MODES)
def test_batch_inverse_canonical_words_count_as_their_residue(eng, mode):
    """the words r and 2r ("edges") are zeros"""
    rng = random.Random(5200)
    v = RL.base(rng, 4097)
    want, zeros = FM.batch_inverse(v)
    assert zeros == 2
    assert inverse_raw(eng, RL.pack(RL.lift(v, mode)), CAN) == (enc(want, CAN), zeros)


def test_batch_inverse_in_place_on_the_device_and_against_vec_mul(eng):
    rng = random.Random(5300)
    n = 70000
    vals = [rng.randrange(1, R) for _ in range(n)]
    vals[77] = 0
    for sfmt in (CAN, MONT):
        blob = enc(vals, sfmt)
        d, z = upload(eng, blob), ctypes.c_size_t(0)
        assert eng.lib.kzg_fr_batch_inverse(eng.ctx, d, n, sfmt, DEV, d, ctypes.byref(z)) == 0, eng.last_error()
        inv = dev_body(eng, d, 32 * n)
        assert z.value == 1 and inv == inverse_raw(eng, blob, sfmt)[0]
        # host in, device out and the reverse
        o = dev_buffer(eng, 32 * n + PAD)
        assert eng.lib.kzg_fr_batch_inverse(eng.ctx, blob, n, sfmt, L.OUT_DEVICE, o, None) == 0
        assert dev_body(eng, o, 32 * n) == inv
        i, h = upload(eng, blob), sentinel_buf(32 * n)
        assert eng.lib.kzg_fr_batch_inverse(eng.ctx, i, n, sfmt, L.IN_DEVICE, h, None) == 0
        assert body(h, 32 * n) == inv
        free(eng, d, o, i)
        # model-free: in * out == 1 except at the zero
        prod = ctypes.create_string_buffer(blob, len(blob))
        assert eng.lib.kzg_fr_vec_mul(eng.ctx, prod, inv, n, sfmt, 0) == 0
        one = enc([1], sfmt)
        assert prod.raw == one * 77 + bytes(32) + one * (n - 78)


# ---- 3. the grand product ----------------------------------------------------------------------------------------------------------
def grand_raw(eng, num, den, n, t, batch, sfmt, flags_out=True):
    z, tot = sentinel_buf(32 * n * batch), sentinel_buf(32 * batch)
    zd = (ctypes.c_int * (batch + 1))(*([-7] * (batch + 1)))
    rc = eng.lib.kzg_fr_grand_product(eng.ctx, num, den, n, t, batch, sfmt, 0, z, tot, zd if flags_out else None)
    assert zd[batch] == -7
    return rc, body(z, 32 * n * batch), body(tot, 32 * batch), list(zd[:batch])


def grand_want(nums, dens, n, t, sfmt):
    zs, tots, flags = [], [], []
    for a, b in zip(nums, dens):
        z, total, zd = FM.grand_product(a, b, n, t)
        zs += z
        tots.append(total)
        flags.append(zd)
    return enc(zs, sfmt), enc(tots, sfmt), flags


def check_grand(eng, nums, dens, n, t, sfmt):
    blob_n, blob_d = enc([x for v in nums for x in v], sfmt), enc([x for v in dens for x in v], sfmt)
    rc, z, tot, zd = grand_raw(eng, blob_n, blob_d, n, t, len(nums), sfmt)
    assert rc == 0, eng.last_error()
    assert (z, tot, zd) == grand_want(nums, dens, n, t, sfmt), (n, t, len(nums), sfmt)


def rand_cols(rng, n, t, batch):
    return [[rng.randrange(1, R) for _ in range(t * n)] for _ in range(batch)]


@pytest.mark.parametrize("n", [1, 2, 9, 2049])
def test_grand_product_default_tile(eng, n):
    rng = random.Random(6100 + n)
    for t in (1, 2, 3, 4):
        for batch in (1, 3):
            nums, dens = rand_cols(rng, n, t, batch), rand_cols(rng, n, t, batch)
            for sfmt in (CAN, MONT):
                check_grand(eng, nums, dens, n, t, sfmt)


def test_grand_product_small_tile_reaches_the_carry_boundaries(eng):
    rng = random.Random(6200)
    tile = 8
    option(eng, b"fr_scan_tile", tile)
    try:
        for k, n in enumerate((tile - 1, tile, tile + 1, 3 * tile + 5, 512 * tile, 512 * tile + 1, 1024 * tile + 3)):
            t = 1 + k % 4
            nums, dens = rand_cols(rng, n, t, 2), rand_cols(rng, n, t, 2)
            check_grand(eng, nums, dens, n, t, CAN if k % 2 else MONT)
    finally:
        option(eng, b"fr_scan_tile", 0)


def test_grand_product_of_a_permutation_is_one(eng):
    rng = random.Random(6300)
    n, t = 2049, 3
    num = [rng.randrange(1, R) for _ in range(t * n)]
    den = list(num)
    rng.shuffle(den)                       # a permutation across (j, i)
    for sfmt in (CAN, MONT):
        rc, z, tot, zd = grand_raw(eng, enc(num, sfmt), enc(den, sfmt), n, t, 1, sfmt)
        assert rc == 0 and tot == enc([1], sfmt) and zd == [0] and z[:32] == enc([1], sfmt)
        assert (z, tot, zd) == grand_want([num], [den], n, t, sfmt)


def test_grand_product_zeros(eng):
    rng = random.Random(6400)
    n, t = 4097, 2
    for at in (0, n - 1, 2047, 2048):
        nums, dens = rand_cols(rng, n, t, 3), rand_cols(rng, n, t, 3)
        nums[0][n + at] = 0                                    # a zero numerator is legal: z is zero from there on
        check_grand(eng, nums, dens, n, t, CAN)
        check_grand(eng, nums, dens, n, t, MONT)
        z = grand_raw(eng, enc(nums[0], CAN), enc(dens[0], CAN), n, t, 1, CAN)[1]
        assert z[32 * (at + 1):] == bytes(32 * (n - at - 1)) and z[32 * at:32 * at + 32] != bytes(32)
        dens[1][at] = 0                                        # a zero denominator in vector 1 of 3
        for sfmt in (CAN, MONT):
            blob_n, blob_d = enc([x for v in nums for x in v], sfmt), enc([x for v in dens for x in v], sfmt)
            rc, z, tot, zd = grand_raw(eng, blob_n, blob_d, n, t, 3, sfmt)
            assert rc == 0 and zd == [0, 1, 0]
            assert z[32 * n:64 * n] == bytes(32 * n) and tot[32:64] == bytes(32)
            assert (z, tot, zd) == grand_want(nums, dens, n, t, sfmt)
            assert grand_raw(eng, blob_n, blob_d, n, t, 3, sfmt, flags_out=False)[0] == SH
    # the words r and 2r are zero denominators too
    nums, dens = rand_cols(rng, 9, 1, 2), rand_cols(rng, 9, 1, 2)
    words = [list(dens[0]), list(dens[1])]
    words[0][3], words[1][8] = R, 2 * R
    rc, z, tot, zd = grand_raw(eng, enc(nums[0] + nums[1], CAN), RL.pack(words[0] + words[1]), 9, 1, 2, CAN)
    assert rc == 0 and zd == [1, 1] and z == bytes(32 * 18) and tot == bytes(64)


@pytest.mark.parametrize("mode", RL.MODES)
def test_grand_product_canonical_words_count_as_their_residue(eng, mode):
    rng = random.Random(6500)
    n, t = 2049, 2
    num, den = RL.base(rng, t * n), [rng.randrange(1, R) for _ in range(t * n)]
    rc, z, tot, zd = grand_raw(eng, RL.pack(RL.lift(num, mode)), RL.pack(RL.lift(den, mode)), n, t, 1, CAN)
    assert rc == 0 and (z, tot, zd) == grand_want([num], [den], n, t, CAN)


def test_grand_product_equals_its_composition(eng):
    """batch inverse of den, vec_mul, exclusive scan: a consistency check (the model is the judge)"""
    rng = random.Random(6600)
    n = 4097
    num, den = [rng.randrange(1, R) for _ in range(n)], [rng.randrange(1, R) for _ in range(n)]
    for sfmt in (CAN, MONT):
        rc, z, tot, _ = grand_raw(eng, enc(num, sfmt), enc(den, sfmt), n, 1, 1, sfmt)
        assert rc == 0
        f = ctypes.create_string_buffer(enc(num, sfmt), 32 * n)
        assert eng.lib.kzg_fr_vec_mul(eng.ctx, f, inverse_raw(eng, enc(den, sfmt), sfmt)[0], n, sfmt, 0) == 0
        assert scan_raw(eng, f.raw, n, 1, PROD, 1, sfmt) == (z, tot)


def test_grand_product_device_buffers(eng):
    rng = random.Random(6700)
    n, t, batch = 2049, 3, 2
    nums, dens = rand_cols(rng, n, t, batch), rand_cols(rng, n, t, batch)
    blob_n, blob_d = enc([x for v in nums for x in v], CAN), enc([x for v in dens for x in v], CAN)
    want = grand_want(nums, dens, n, t, CAN)
    dn, dd, dz = upload(eng, blob_n), upload(eng, blob_d), dev_buffer(eng, 32 * n * batch + PAD)
    tot, zd = sentinel_buf(32 * batch), (ctypes.c_int * batch)()
    assert eng.lib.kzg_fr_grand_product(eng.ctx, dn, dd, n, t, batch, CAN, DEV, dz, tot, zd) == 0, eng.last_error()
    assert (dev_body(eng, dz, 32 * n * batch), body(tot, 32 * batch), list(zd)) == want
    h = sentinel_buf(32 * n * batch)
    assert eng.lib.kzg_fr_grand_product(eng.ctx, dn, dd, n, t, batch, CAN, L.IN_DEVICE, h, None, None) == 0
    assert body(h, 32 * n * batch) == want[0]
    assert dev_body(eng, dn, len(blob_n)) == blob_n and dev_body(eng, dd, len(blob_d)) == blob_d
    free(eng, dn, dd, dz)


# ---- 4. staging, chunking, launches --------------------------------------------------------------------------------------------------
def launches(eng, name):
    c, ms = ctypes.c_uint64(0), ctypes.c_double(0)
    if eng.lib.kzg_prof_get(eng.ctx, name, ctypes.byref(c), ctypes.byref(ms)) != 0:
        return 0
    return c.value


class profiled:
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        assert self.eng.lib.kzg_prof_enable(self.eng.ctx, 1) == 0 and self.eng.lib.kzg_prof_reset(self.eng.ctx) == 0

    def __exit__(self, *exc):
        assert self.eng.lib.kzg_prof_enable(self.eng.ctx, 0) == 0


SCAN_KERNELS = (b"k_frscan_partials", b"k_frscan_carry", b"k_frscan_apply")
GRAND_KERNELS = (b"k_grand_partials", b"k_grand_carry", b"k_grand_apply")


def test_one_launch_of_each_kernel_per_chunk(eng):
    rng = random.Random(7100)
    n = 4097
    vecs = rand_vecs(rng, n, 8)
    with profiled(eng):
        check_scan(eng, vecs, PROD, 0, CAN)
        assert [launches(eng, k) for k in SCAN_KERNELS] == [1, 1, 1]
    nums, dens = rand_cols(rng, 2049, 3, 2), rand_cols(rng, 2049, 3, 2)
    with profiled(eng):
        check_grand(eng, nums, dens, 2049, 3, CAN)
        assert [launches(eng, k) for k in GRAND_KERNELS] == [1, 1, 1]
        assert [launches(eng, k) for k in SCAN_KERNELS] == [0, 0, 0]


def test_staged_pieces_and_vector_chunks(eng):
    """a 4 KiB staging piece holds one vector of these shapes (three pieces for three vectors) and 128 scalars of an inversion; two
    vectors per chunk of launches work five device vectors off in three"""
    rng = random.Random(7200)
    vecs = rand_vecs(rng, 100, 3)
    nums, dens = rand_cols(rng, 40, 2, 3), rand_cols(rng, 40, 2, 3)
    vals = [rng.randrange(R) for _ in range(300)]
    option(eng, b"fr_scan_stage", 4096)
    try:
        with profiled(eng):
            check_scan(eng, vecs, PROD, 1, CAN)
            check_grand(eng, nums, dens, 40, 2, MONT)
            assert [launches(eng, k) for k in SCAN_KERNELS + GRAND_KERNELS] == [3] * 6
            assert inverse_raw(eng, enc(vals, CAN), CAN) == (enc(FM.batch_inverse(vals)[0], CAN), FM.batch_inverse(vals)[1])
            assert launches(eng, b"k_batch_inverse") == 3
        # a vector larger than the piece is staged whole
        check_scan(eng, rand_vecs(rng, 300, 2), SUM, 0, MONT)
    finally:
        option(eng, b"fr_scan_stage", 0)
    vecs = rand_vecs(rng, 100, 5)
    blob = enc([x for v in vecs for x in v], CAN)
    option(eng, b"fr_scan_chunk", 2)
    try:
        with profiled(eng):
            d, tot = upload(eng, blob), sentinel_buf(32 * 5)
            assert eng.lib.kzg_fr_scan(eng.ctx, d, 100, 5, PROD, 0, CAN, DEV, d, tot) == 0
            assert (dev_body(eng, d, len(blob)), body(tot, 32 * 5)) == scan_want(vecs, PROD, 0, CAN)
            free(eng, d)
            assert [launches(eng, k) for k in SCAN_KERNELS] == [3, 3, 3]
            nums, dens = rand_cols(rng, 40, 2, 5), rand_cols(rng, 40, 2, 5)
            check_grand(eng, nums, dens, 40, 2, CAN)
            assert [launches(eng, k) for k in GRAND_KERNELS] == [3, 3, 3]
    finally:
        option(eng, b"fr_scan_chunk", 0)


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------------
def test_shape_errors_touch_nothing(eng):
    lib, ctx = eng.lib, eng.ctx
    rng = random.Random(7300)
    n = 9
    vals = [rng.randrange(1, R) for _ in range(2 * n)]
    blob = enc(vals, CAN)
    out, tot = sentinel_buf(32 * 2 * n), sentinel_buf(64)
    zc, zd = ctypes.c_size_t(4242), (ctypes.c_int * 2)(-7, -7)
    big = (1 << 28) + 1
    huge = SIZE_MAX >> 8
    calls = [
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, PROD, 0, 2, 0, out, tot),                       # unknown format
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, 2, 0, CAN, 0, out, tot),                        # unknown op
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, -1, 0, CAN, 0, out, tot),
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, PROD, 2, CAN, 0, out, tot),                     # exclusive not 0 or 1
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, PROD, -1, CAN, 0, out, tot),
        lambda: lib.kzg_fr_scan(ctx, blob, 0, 2, PROD, 0, CAN, 0, out, tot),                     # n == 0
        lambda: lib.kzg_fr_scan(ctx, None, n, 2, PROD, 0, CAN, 0, out, tot),                     # NULL with work to do
        lambda: lib.kzg_fr_scan(ctx, blob, n, 2, PROD, 0, CAN, 0, None, tot),
        lambda: lib.kzg_fr_scan(ctx, blob, big, 1, PROD, 0, CAN, 0, out, tot),                   # n > 2^28
        lambda: lib.kzg_fr_scan(ctx, blob, 1 << 28, huge, PROD, 0, CAN, 0, out, tot),            # batch x n x 32 beyond size_t
        lambda: lib.kzg_fr_scan(None, blob, n, 2, PROD, 0, CAN, 0, out, tot),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, n, 1, 2, 2, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, 0, 1, 2, CAN, 0, out, tot, zd),        # n == 0
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, n, 0, 2, CAN, 0, out, tot, zd),        # t == 0
        lambda: lib.kzg_fr_grand_product(ctx, None, blob, n, 1, 2, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, None, n, 1, 2, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, n, 1, 2, CAN, 0, None, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, big, 1, 1, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, 1 << 28, huge, 1, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(ctx, blob, blob, 1 << 28, 3, huge, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_grand_product(None, blob, blob, n, 1, 2, CAN, 0, out, tot, zd),
        lambda: lib.kzg_fr_batch_inverse(ctx, blob, 2 * n, 2, 0, out, ctypes.byref(zc)),
        lambda: lib.kzg_fr_batch_inverse(ctx, blob, 0, CAN, 0, out, ctypes.byref(zc)),           # n == 0
        lambda: lib.kzg_fr_batch_inverse(ctx, None, 2 * n, CAN, 0, out, ctypes.byref(zc)),
        lambda: lib.kzg_fr_batch_inverse(ctx, blob, 2 * n, CAN, 0, None, ctypes.byref(zc)),
        lambda: lib.kzg_fr_batch_inverse(ctx, blob, big, CAN, 0, out, ctypes.byref(zc)),
        lambda: lib.kzg_fr_batch_inverse(None, blob, 2 * n, CAN, 0, out, ctypes.byref(zc)),
    ]
    for k, call in enumerate(calls):
        assert call() == SH, k
        assert out.raw == A5 * len(out.raw) and tot.raw == A5 * len(tot.raw) and zc.value == 4242 and list(zd) == [-7, -7], k
    # batch == 0: nothing to do, nothing touched
    assert lib.kzg_fr_scan(ctx, None, n, 0, PROD, 0, CAN, 0, None, None) == 0
    assert lib.kzg_fr_grand_product(ctx, None, None, n, 1, 0, CAN, 0, None, None, None) == 0
    for bad in (3, 4, 4096, -1):
        assert lib.kzg_ctx_set_option(ctx, b"fr_scan_tile", bad) == SH
    for key, bad in ((b"fr_scan_stage", 16), (b"fr_scan_stage", 100), (b"fr_scan_stage", (64 << 20) + 32), (b"fr_scan_chunk", -1), (b"fr_scan_chunk", 65536)):
        assert lib.kzg_ctx_set_option(ctx, key, bad) == SH
    # the context still computes
    check_scan(eng, [vals[:n], vals[n:]], PROD, 0, CAN)
    check_grand(eng, [vals[:n]], [vals[n:]], n, 1, CAN)


# ---- 6. concurrency ----------------------------------------------------------------------------------------------------------------
def test_eight_threads_on_one_context(eng):
    rng = random.Random(7400)
    jobs = []
    for k, n in enumerate((7, 2047, 2049, 4097)):
        vecs = rand_vecs(rng, n, 1 + k % 3)
        blob = enc([x for v in vecs for x in v], CAN)
        jobs.append(lambda blob=blob, n=n, b=len(vecs), k=k: scan_raw(eng, blob, n, b, k % 2, k // 2 % 2, CAN))
    for n, t in ((9, 4), (2049, 3)):
        bn, bd = enc(rand_cols(rng, n, t, 2)[0] * 2, MONT), enc([x for v in rand_cols(rng, n, t, 2) for x in v], MONT)
        jobs.append(lambda bn=bn, bd=bd, n=n, t=t: grand_raw(eng, bn, bd, n, t, 2, MONT))
    for n in (17, 4097):
        blob = enc([rng.randrange(R) for _ in range(n)], CAN)
        jobs.append(lambda blob=blob: inverse_raw(eng, blob, CAN))
    assert len(jobs) == 8
    alone = [job() for job in jobs]
    bad = []

    def work(k):
        try:
            for _ in range(20):
                if jobs[k]() != alone[k]:
                    bad.append(k)
        except BaseException as e:  # noqa: BLE001 -- reported below
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad


# ---- 7. the mirrors ----------------------------------------------------------------------------------------------------------------
def test_python_mirrors(eng):
    import kzg_amd
    rng = random.Random(7500)
    n, t = 33, 2
    vecs = rand_vecs(rng, n, 2)
    flat = [x for v in vecs for x in v]
    for op in ("product", "sum"):
        for excl in (False, True):
            want = [FM.scan(v, op, excl) for v in vecs]
            assert eng.fr_scan(flat, n, op, excl) == ([x for o, _ in want for x in o], [tt for _, tt in want])
    assert eng.prefix_product(flat, n) == eng.fr_scan(flat, n, "product") and eng.prefix_sum(flat, n, True) == eng.fr_scan(flat, n, "sum", True)
    vals = flat[:40] + [0]
    assert eng.batch_inverse(vals) == FM.batch_inverse(vals)
    nums, dens = rand_cols(rng, n, t, 2), rand_cols(rng, n, t, 2)
    want = [FM.grand_product(a, b, n, t) for a, b in zip(nums, dens)]
    got = eng.grand_product(nums[0] + nums[1], dens[0] + dens[1], n, t)
    assert got == ([x for z, _, _ in want for x in z], [tt for _, tt, _ in want], [0, 0])
    dens[1][5] = 0
    with pytest.raises(kzg_amd.ReferencePanic):
        eng.grand_product(nums[0] + nums[1], dens[0] + dens[1], n, t)
    z, tot, zd = eng.grand_product(nums[0] + nums[1], dens[0] + dens[1], n, t, strict=False)
    assert zd == [0, 1] and tot[1] == 0 and z[n:] == [0] * n and z[:n] == want[0][0]
    # DeviceBuffers, Montgomery form, in place where the call allows it
    buf = kzg_amd.DeviceBuffer(eng, 2 * n, MONT).upload(enc(flat, MONT))
    out, tot = eng.fr_scan(buf, n, "product", out=buf)
    assert out is buf and buf.download() == enc([x for v in vecs for x in FM.scan(v)[0]], MONT) and tot == [FM.scan(v)[1] for v in vecs]
    inv, zeros = eng.batch_inverse(buf, out=buf)
    assert zeros == 0 and buf.download() == enc([pow(x, -1, R) for v in vecs for x in FM.scan(v)[0]], MONT)
    dn = kzg_amd.DeviceBuffer(eng, t * n, MONT).upload(enc(nums[0], MONT))
    dd = kzg_amd.DeviceBuffer(eng, t * n, MONT).upload(enc(dens[0], MONT))
    dz = kzg_amd.DeviceBuffer(eng, n, MONT)
    z, tot, zd = eng.grand_product(dn, dd, n, t, out=dz)
    assert z is dz and dz.download() == enc(want[0][0], MONT) and tot == [want[0][1]] and zd == [0]
    for b in (buf, dn, dd, dz):
        b.free()


def test_cpp_wrapper(tmp_path):
    """batch_inverse, fr_scan and grand_product of include/kzg_mi355x.hpp: tests/cpp_fr_scan_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_fr_scan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_fr_scan_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
