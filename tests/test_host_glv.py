"""CPU checks of kzg_amd/csrc/glv.h (the GLV scalar multiplication of the FK20 kernels), compiled with g++ from the same source
hipcc builds for gfx950 (tests/host_glv.cpp), against the oracle."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import fk20_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("glv") / "host_glv.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "host_glv.cpp")])
    return ctypes.CDLL(so)


EDGE = [0, 1, 2, F.GLV_LAMBDA - 1, F.GLV_LAMBDA, F.GLV_LAMBDA + 1, M.R - 2, M.R - 1]


def test_split_and_recode(lib):
    rng = random.Random(3)
    for k in EDGE + [rng.randrange(M.R) for _ in range(100)]:
        k1, k2, rec = ctypes.create_string_buffer(16), ctypes.create_string_buffer(16), ctypes.create_string_buffer(48)
        lib.hg_glv_split(M.fr_to_le(k), k1, k2, rec)
        a, b = int.from_bytes(k1.raw, "little"), int.from_bytes(k2.raw, "little")
        assert (a, b) == F.glv_split(k)
        top = int.from_bytes(rec.raw[32:36], "little")
        mask, eights = (1 << 128) - 1, int("8" * 32, 16)
        assert int.from_bytes(rec.raw[:16], "little") == (a + eights) & mask and (top & 1) == (a + eights) >> 128
        assert int.from_bytes(rec.raw[16:32], "little") == (b + eights) & mask and (top >> 1) == (b + eights) >> 128


def test_mul_matches_oracle(lib):
    rng = random.Random(4)
    G = C.g1_generator()
    for P in (bytes(96), G, C.g1_mul(G, rng.randrange(1, M.R))):
        for k in EDGE + [rng.randrange(M.R) for _ in range(12)]:
            for glv in (1, 0):
                out = ctypes.create_string_buffer(96)
                lib.hg_g1_mul(P, M.fr_to_le(k), glv, out)
                assert out.raw == C.g1_mul(P, k), (glv, k)
