"""What tests/test_gpu_fk20.py and tests/test_gpu_fk20_cosets.py share: helpers and the bodies of their module-scoped fixtures.
Both files sort after the tests that release the session's contexts (tests/conftest.py ORDER), so each opens and closes an Engine
and a HooksEngine of its own: they import the fixture functions below by name, which makes them fixtures of the importing module.
What differs between the two files is read from the importing module: TAU, SRS_LEN, G2_LEN and PLAN (the plan class)."""
import ctypes

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests.gpu_common import HooksEngine

VP, SZ, I32, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
FORMATS = [L.G1_AFFINE_MONT, L.G1_JACOBIAN_MONT, L.G1_ZCASH_UNCOMPRESSED, L.G1_ZCASH_COMPRESSED]
MONT_R = pow(2, 256, M.R)
SIZE_MAX = ctypes.c_size_t(-1).value


@pytest.fixture(scope="module")
def eng():
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hooks():
    h = HooksEngine(0)
    h.lib.kzg_test_g1_mul_glv.argtypes = [VP, VP, VP, SZ, VP]
    h.lib.kzg_test_g1_mul_glv.restype = I32
    h.lib.kzg_test_g1_ntt.argtypes = [VP, VP, U32, I32, VP]
    h.lib.kzg_test_g1_ntt.restype = I32
    h.lib.kzg_test_fk20_cosets_combine.argtypes = [VP, VP, VP, SZ, SZ, I32, SZ, VP]
    h.lib.kzg_test_fk20_cosets_combine.restype = I32
    yield h
    h.close()


@pytest.fixture(scope="module")
def params(request, eng):
    m = request.module
    p = kzg_amd.setup(eng, m.TAU, m.SRS_LEN, g2_len=m.G2_LEN)
    yield p
    p.gs.free()
    if p.hs is not None:
        p.hs.free()


@pytest.fixture(scope="module")
def plans(request, eng, params):
    """plans(log_n) / plans(log_n, log_l): the importing module's PLAN for that shape over `params`, built once"""
    cache = {}

    def get(*shape):
        if shape not in cache:
            cache[shape] = request.module.PLAN(eng, params.gs, *shape)
        return cache[shape]
    yield get
    for p in cache.values():
        p.free()


def G():
    return C.g1_generator()


def same_point(a, b, fmt):
    """byte equality; the Jacobian form is not canonical, so there the projective coordinates are compared"""
    if fmt != L.G1_JACOBIAN_MONT:
        return a == b
    q = M.Q
    X1, Y1, Z1 = (int.from_bytes(a[i:i + 48], "little") for i in (0, 48, 96))
    X2, Y2, Z2 = (int.from_bytes(b[i:i + 48], "little") for i in (0, 48, 96))
    if Z1 % q == 0 or Z2 % q == 0:
        return Z1 % q == 0 and Z2 % q == 0
    return (X1 * Z2 * Z2 - X2 * Z1 * Z1) % q == 0 and (Y1 * Z2 ** 3 - Y2 * Z1 ** 3) % q == 0


def split(raw, psz, count):
    return [raw[i * psz:(i + 1) * psz] for i in range(count)]


def dev_buffer(eng, nbytes):
    """a device allocation filled with 0xA5, so that a region no call writes cannot pass for a result"""
    p = ctypes.c_void_p()
    assert eng.lib.kzg_dev_alloc(eng.ctx, nbytes, ctypes.byref(p)) == 0
    assert eng.lib.kzg_dev_upload(eng.ctx, p, b"\xa5" * nbytes, nbytes) == 0
    return p


def dev_download(eng, p, nbytes):
    back = ctypes.create_string_buffer(nbytes)
    assert eng.lib.kzg_dev_download(eng.ctx, back, p, nbytes) == 0
    return back.raw
