"""kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch on the GPU, through the C ABI via kzg_amd.  Expected bytes come from
oracle.c_oracle.fft_bytes per vector, on the residues of the inputs, and for the coset calls from coset_fft / icoset_fft of
oracle.kzg_model; at the two sizes around the crossover to the per-vector loop they come from kzg_ntt_fr, which the existing tests pin
to the oracle there.  Every comparison is equality of bytes.  Buffers carry one sentinel vector before the first and one after the
last vector, and a pattern in the words between strided vectors: all of it must come back byte for byte."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests.fk20_common import dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = M.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
LAST_BATCHED, FIRST_LOOPED = 19, 20  # the default crossover (include/kzg_mi355x.h, kzg_ntt_fr_batch)
PLANTED = [0, R - 1, R, R + 1, (1 << 256) - 1]


def le(v):
    return int(v).to_bytes(32, "little")


def vectors(seed, log_n, batch):
    """`batch` vectors of random full-width words with 0, r - 1, r, r + 1 and 2^256 - 1 planted in each, as far as it is long"""
    rng = random.Random(seed * 1000 + log_n * 31 + batch)
    n = 1 << log_n
    out = []
    for _ in range(batch):
        v = [rng.getrandbits(256) for _ in range(n)]
        for p, w in zip(rng.sample(range(n), min(n, len(PLANTED))), PLANTED):
            v[p] = w
        out.append(v)
    return out


def expected_fft(v, log_n, inverse):
    return C.fft_bytes(b"".join(le(x % R) for x in v), log_n, inverse)


def layout(vecs, log_n, stride):
    """(buffer bytes, offset of vector 0 in bytes): sentinel vector, the vectors `stride` elements apart with a pattern between, sentinel"""
    n = 1 << log_n
    stride = stride or n
    gap = bytes((i * 7 + 3) & 0xFF for i in range((stride - n) * 32))
    body = b"".join(b"".join(le(x) for x in v) + (gap if b + 1 < len(vecs) else b"") for b, v in enumerate(vecs))
    sent = b"\xa5" * (32 * n)
    return sent + body + sent, len(sent)


def run(eng, vecs, log_n, stride=0, inverse=False, device=True, coset=None, batch=None):
    """the call on the laid-out buffer; returns (result bytes per vector, whole buffer before, whole buffer after)"""
    n = 1 << log_n
    batch = len(vecs) if batch is None else batch
    before, off = layout(vecs, log_n, stride)
    if device:
        p = dev_buffer(eng, len(before))
        try:
            assert eng.lib.kzg_dev_upload(eng.ctx, p, before, len(before)) == 0
            data = ctypes.c_void_p(p.value + off)
            if coset is None:
                rc = eng.lib.kzg_ntt_fr_batch(eng.ctx, data, log_n, batch, stride, int(inverse), L.IN_DEVICE)
            else:
                rc = eng.lib.kzg_coset_ntt_fr_batch(eng.ctx, data, log_n, batch, stride, int(inverse), coset, L.IN_DEVICE)
            assert rc == 0, eng.last_error()
            after = dev_download(eng, p, len(before))
        finally:
            eng.lib.kzg_dev_free(eng.ctx, p)
    else:
        buf = ctypes.create_string_buffer(before, len(before))
        data = ctypes.c_void_p(ctypes.addressof(buf) + off)
        if coset is None:
            rc = eng.lib.kzg_ntt_fr_batch(eng.ctx, data, log_n, batch, stride, int(inverse), 0)
        else:
            rc = eng.lib.kzg_coset_ntt_fr_batch(eng.ctx, data, log_n, batch, stride, int(inverse), coset, 0)
        assert rc == 0, eng.last_error()
        after = buf.raw
    st = (stride or n) * 32
    return [after[off + b * st: off + b * st + 32 * n] for b in range(len(vecs))], before, after


def check(eng, vecs, log_n, want, **kw):
    """results equal `want` per vector; everything else in the buffer (sentinels, gaps, vectors beyond `batch`) is unchanged"""
    n = 1 << log_n
    got, before, after = run(eng, vecs, log_n, **kw)
    batch = kw.get("batch")
    batch = len(vecs) if batch is None else batch
    st = (kw.get("stride") or n) * 32
    expect = bytearray(before)
    for b in range(batch):
        expect[32 * n + b * st: 32 * n + b * st + 32 * n] = want[b]
    bad = [b for b in range(batch) if got[b] != want[b]]
    assert not bad, "vectors %s differ from the expectation" % bad
    assert after == bytes(expect), "bytes outside the %d transformed vectors changed" % batch


class options:
    """context options for the block, back to their defaults afterwards"""

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.eng.lib.kzg_ctx_set_option(self.eng.ctx, k.encode(), v) == 0, self.eng.last_error()

    def __exit__(self, *exc):
        for k in self.kv:
            assert self.eng.lib.kzg_ctx_set_option(self.eng.ctx, k.encode(), 0) == 0


@pytest.mark.parametrize("log_n", range(13))
def test_every_small_size(eng, log_n):
    for inverse in (False, True):
        for batch in (1, 2, 3, 5):
            vecs = vectors(1, log_n, batch)
            check(eng, vecs, log_n, [expected_fft(v, log_n, inverse) for v in vecs], inverse=inverse)


@pytest.mark.parametrize("log_n", [2, 5, 8, 10])
def test_tile_boundaries(eng, log_n):
    """R = 1, 2, 4 rows per tile forced; batches around one and two tiles; the vector behind the batch is a transform input that the
    call must leave alone, beside the sentinels"""
    for v in (0, 1, 2):
        rows = 1 << v
        with options(eng, ntt_batch_rows_log=1 + v):
            for batch in sorted({rows - 1, rows, rows + 1, 2 * rows + 1} - {0}):
                vecs = vectors(2 + v, log_n, batch + 1)
                want = [expected_fft(x, log_n, False) for x in vecs[:batch]]
                check(eng, vecs, log_n, want, batch=batch)


@pytest.mark.parametrize("log_n", [3, 12, 13])
@pytest.mark.parametrize("device", [True, False])
def test_stride(eng, log_n, device):
    n = 1 << log_n
    vecs = vectors(5, log_n, 3)
    want = [expected_fft(v, log_n, False) for v in vecs]
    for stride in (n + 1, 2 * n):
        check(eng, vecs, log_n, want, stride=stride, device=device)


@pytest.mark.parametrize("log_n", [4, 12, 13, 14])
def test_chunks(eng, log_n):
    vecs = vectors(6, log_n, 5)
    default = run(eng, vecs, log_n)[0]
    assert default == [expected_fft(v, log_n, False) for v in vecs]
    for chunk in (1, 2, 3):
        with options(eng, ntt_batch_chunk=chunk):
            check(eng, vecs, log_n, default)


@pytest.mark.parametrize("log_n,batches", [(13, (3, 5)), (14, (3, 5)), (15, (3, 5)), (16, (2,))])
def test_two_pass_regime(eng, log_n, batches):
    for batch in batches:
        vecs = vectors(7, log_n, batch)
        for inverse in (False, True):
            check(eng, vecs, log_n, [expected_fft(v, log_n, inverse) for v in vecs], inverse=inverse)


@pytest.mark.parametrize("log_n", [LAST_BATCHED, FIRST_LOOPED])
def test_crossover(eng, log_n):
    """the last size on the batched two-pass kernels and the first on the per-vector loop, against kzg_ntt_fr vector by vector"""
    n = 1 << log_n
    buf = kzg_amd.DeviceBuffer(eng, 2 * n).fill_random(40 + log_n)
    one = kzg_amd.DeviceBuffer(eng, n)
    try:
        want = []
        for b in range(2):
            one.upload(buf.download(n, b * n))
            eng.ntt(one, log_n)
            want.append(one.download())
        eng.ntt_batch(buf, log_n, 2)
        assert [buf.download(n, 0), buf.download(n, n)] == want
    finally:
        buf.free()
        one.free()


_COSET = {}


def expected_coset(v, log_n, inverse):
    key = (tuple(v), inverse)
    if key not in _COSET:
        d = M.EvaluationDomain.from_coeffs([x % R for x in v])
        d.icoset_fft() if inverse else d.coset_fft()
        _COSET[key] = list(d.coeffs)
    return _COSET[key]


@pytest.mark.parametrize("log_n", [0, 1, 6, 12, 13])
def test_coset(eng, log_n):
    n = 1 << log_n
    vecs = vectors(8, log_n, 3)
    for inverse in (False, True):
        want = [expected_coset(v, log_n, inverse) for v in vecs]
        check(eng, vecs, log_n, [b"".join(le(x) for x in w) for w in want], inverse=inverse, coset=CAN)
        # Montgomery words: the residue x stands for x / 2^256, and the map is linear
        check(eng, vecs, log_n, [b"".join(le(x) for x in w) for w in want], inverse=inverse, coset=MONT)
    want = [b"".join(le(x) for x in expected_coset(v, log_n, False)) for v in vecs]
    check(eng, vecs, log_n, want, stride=n + 1, coset=CAN)
    check(eng, vecs, log_n, want, stride=n + 1, coset=CAN, device=False)


@pytest.mark.parametrize("log_n,batch", [(12, 7), (14, 3)])
def test_round_trip(eng, log_n, batch):
    n = 1 << log_n
    vecs = vectors(9, log_n, batch)
    buf = kzg_amd.DeviceBuffer(eng, batch * n).upload(b"".join(le(x) for v in vecs for x in v))
    try:
        eng.ntt_batch(buf, log_n, batch)
        eng.ntt_batch(buf, log_n, batch, inverse=True)
        assert buf.download() == b"".join(le(x % R) for v in vecs for x in v)
    finally:
        buf.free()


def launches(eng, call):
    eng.prof_reset()
    call()
    return {k: c for k, (c, _ms) in eng.prof_all().items() if c}


def test_batching_happens(eng):
    """one call's kernel launches do not depend on the batch (default options: one chunk)"""
    eng.prof_enable(True)
    try:
        for log_n, batch, coset in ((10, 64, False), (14, 8, False), (10, 64, True)):
            n = 1 << log_n
            buf = kzg_amd.DeviceBuffer(eng, batch * n).fill_random(3)
            try:
                fn = eng.coset_ntt_batch if coset else eng.ntt_batch
                fn(buf, log_n, 1)  # tables and plans exist from here on
                one = launches(eng, lambda: fn(buf, log_n, 1))
                many = launches(eng, lambda: fn(buf, log_n, batch))
                assert sum(one.values()) >= 1 and sum(many.values()) == sum(one.values()), (log_n, batch, coset, one, many)
            finally:
                buf.free()
    finally:
        eng.prof_enable(False)
        eng.prof_reset()


def test_kzg_ntt_fr_launches_what_it_launched(eng):
    eng.prof_enable(True)
    try:
        for log_n, want in ((10, {"k_ntt_single": 1}), (14, {"k_ntt_pass1": 1, "k_ntt_pass2": 1})):
            buf = kzg_amd.DeviceBuffer(eng, 1 << log_n).fill_random(4)
            try:
                eng.ntt(buf, log_n)
                assert launches(eng, lambda: eng.ntt(buf, log_n)) == want
            finally:
                buf.free()
    finally:
        eng.prof_enable(False)
        eng.prof_reset()


def test_statuses(eng):
    lib, ctx = eng.lib, eng.ctx
    p = dev_buffer(eng, 32 << 12)
    try:
        before = dev_download(eng, p, 32 << 12)
        assert lib.kzg_ntt_fr_batch(ctx, p, 12, 0, 0, 0, L.IN_DEVICE) == 0
        assert lib.kzg_coset_ntt_fr_batch(ctx, p, 12, 0, 0, 0, CAN, L.IN_DEVICE) == 0
        assert dev_download(eng, p, 32 << 12) == before
        for args, status in (((12, 1, (1 << 12) - 1), L.KZG_ERR_SHAPE), ((32, 1, 0), L.KZG_ERR_DEGREE_TOO_LARGE), ((29, 1, 0), L.KZG_ERR_SHAPE),
                             ((12, 1 << 62, 1 << 12), L.KZG_ERR_SHAPE)):
            log_n, batch, stride = args
            eng.prof_reset()
            assert lib.kzg_ntt_fr_batch(ctx, p, log_n, batch, stride, 0, L.IN_DEVICE) == status
            assert eng.last_error()
            assert lib.kzg_coset_ntt_fr_batch(ctx, p, log_n, batch, stride, 0, CAN, L.IN_DEVICE) == status
            assert eng.last_error()
        assert dev_download(eng, p, 32 << 12) == before
        eng.prof_enable(True)
        try:
            assert launches(eng, lambda: lib.kzg_ntt_fr_batch(ctx, p, 12, 1 << 62, 1 << 12, 0, L.IN_DEVICE)) == {}
        finally:
            eng.prof_enable(False)
            eng.prof_reset()
        assert lib.kzg_ntt_fr_batch(None, p, 12, 1, 0, 0, L.IN_DEVICE) == L.KZG_ERR_SHAPE
        assert lib.kzg_ntt_fr_batch(ctx, None, 12, 1, 0, 0, L.IN_DEVICE) == L.KZG_ERR_SHAPE
        for key in (b"ntt_batch_chunk", b"ntt_batch_rows_log"):
            assert lib.kzg_ctx_set_option(ctx, key, 1) == 0
            assert lib.kzg_ctx_set_option(ctx, key, 0) == 0
            assert lib.kzg_ctx_set_option(ctx, key, -1) == L.KZG_ERR_SHAPE and eng.last_error()
    finally:
        lib.kzg_dev_free(ctx, p)


def test_concurrent_callers(eng):
    """four threads on one context, 20 calls each at a size of their own"""
    sizes = [6, 10, 12, 13]
    cases = {t: vectors(20 + t, t, 3) for t in sizes}
    want = {t: [expected_fft(v, t, False) for v in cases[t]] for t in sizes}
    errors = []

    def worker(t):
        try:
            for _ in range(20):
                got = run(eng, cases[t], t, device=False)[0]
                if got != want[t]:
                    errors.append("2^%d: wrong bytes" % t)
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append("2^%d: %r" % (t, e))
    threads = [threading.Thread(target=worker, args=(t,)) for t in sizes]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_python_mirror(eng):
    rng = random.Random(11)
    vecs = [[rng.randrange(R) for _ in range(64)] for _ in range(3)]
    assert eng.ntt_batch(vecs, 6) == [C.fft(v) for v in vecs]
    domains = [kzg_amd.EvaluationDomain.from_coeffs(v) for v in vecs]
    kzg_amd.EvaluationDomain.fft_many(eng, domains)
    assert [d.coeffs for d in domains] == [C.fft(v) for v in vecs]
    kzg_amd.EvaluationDomain.ifft_many(eng, domains)
    assert [d.coeffs for d in domains] == vecs
    kzg_amd.EvaluationDomain.coset_fft_many(eng, domains)
    assert [d.coeffs for d in domains] == [expected_coset(v, 6, False) for v in vecs]
    kzg_amd.EvaluationDomain.icoset_fft_many(eng, domains)
    assert [d.coeffs for d in domains] == vecs


def test_cpp_wrapper(tmp_path):
    """ntt_batch and EvaluationDomain::fft_many / ifft_many of include/kzg_mi355x.hpp: tests/cpp_ntt_batch_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_ntt_batch_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_ntt_batch_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
