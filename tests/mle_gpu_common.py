"""What tests/test_gpu_mle.py and tests/test_gpu_sumcheck.py share: byte encodings, options, and buffers with 0xA5 sentinels behind them."""
import ctypes

from kzg_amd import _lib as L
from tests import mle_model as MM
from tests.fk20_common import MONT_R, dev_buffer, dev_download

R = MM.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
SH = L.KZG_ERR_SHAPE
PAD = 64
A5 = b"\xa5"
HH, DD, HD, DH = 0, L.IN_DEVICE | L.OUT_DEVICE, L.OUT_DEVICE, L.IN_DEVICE


def enc(vals, sfmt):
    """canonical: the words as they are (a word at or above r stays one); Montgomery: the residue's Montgomery form"""
    if sfmt == MONT:
        return b"".join((v % R * MONT_R % R).to_bytes(32, "little") for v in vals)
    return b"".join(v.to_bytes(32, "little") for v in vals)


def data(rng, n, sfmt):
    """n data words: in canonical form any 256-bit word (about three in four lie at or above r, and r and 2^256 - 1 are among them)"""
    if sfmt == MONT:
        return [rng.randrange(R) for _ in range(n)]
    vals = [rng.randrange(1 << 256) for _ in range(n)]
    vals[0] = R
    vals[-1] = (1 << 256) - 1
    return vals


def option(eng, key, value):
    assert eng.lib.kzg_ctx_set_option(eng.ctx, key.encode(), value) == 0, eng.last_error()


class Options:
    """with Options(eng, mle_block=64, ...): the options set, and back at 0 afterwards"""

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, kv

    def __enter__(self):
        for k, v in self.kv.items():
            option(self.eng, k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            option(self.eng, k, 0)
        return False


class Buf:
    """`nbytes` of payload with PAD sentinel bytes behind them, host or device; filled with `blob` or with 0xA5"""

    def __init__(self, eng, nbytes, dev, blob=None):
        self.eng, self.nbytes, self.dev = eng, nbytes, dev
        init = (blob if blob is not None else A5 * nbytes) + A5 * PAD
        assert len(init) == nbytes + PAD
        self.init = init
        if dev:
            self.p = dev_buffer(eng, nbytes + PAD)
            assert eng.lib.kzg_dev_upload(eng.ctx, self.p, init, len(init)) == 0
            self.addr = self.p.value
        else:
            self.h = ctypes.create_string_buffer(init, len(init))
            self.addr = ctypes.addressof(self.h)

    def raw(self):
        return dev_download(self.eng, self.p, self.nbytes + PAD) if self.dev else self.h.raw

    def body(self):
        r = self.raw()
        assert r[self.nbytes:] == A5 * PAD, "bytes behind a buffer were written"
        return r[:self.nbytes]

    def untouched(self):
        return self.raw() == self.init

    def free(self):
        if self.dev:
            assert self.eng.lib.kzg_dev_free(self.eng.ctx, self.p) == 0


def ptrs(bufs):
    return (ctypes.c_void_p * max(len(bufs), 1))(*[b.addr if isinstance(b, Buf) else b for b in bufs])
