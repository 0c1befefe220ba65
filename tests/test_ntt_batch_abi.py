"""kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch: the declarations of the header and their mirrors (ctypes table, C++ header, Rust binding,
Python classes).  No GPU: nothing here creates a context."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "kzg_ntt_fr_batch": "int kzg_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int flags);",
    "kzg_coset_ntt_fr_batch": "int kzg_coset_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int sfmt, int flags);",
}
CTYPES = {"kzg_ctx *": ctypes.c_void_p, "void *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "int": ctypes.c_int}


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_call(name):
    assert SIGNATURES[name] in squeeze(text("include", "kzg_mi355x.h"))


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_ctypes_binding_matches_the_header(name):
    import kzg_amd
    lib = kzg_amd.load()
    params = SIGNATURES[name][SIGNATURES[name].index("(") + 1:SIGNATURES[name].index(")")].split(", ")
    want = [CTYPES[re.sub(r"\w+$", "", p).strip()] for p in params]
    restype, argtypes = lib._kzg_signatures[name]
    assert restype is ctypes.c_int and list(argtypes) == want
    assert list(getattr(lib, name).argtypes) == want


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_cpp_and_rust_name_the_call(name):
    assert re.search(r"\b%s\(" % name, text("include", "kzg_mi355x.hpp"))
    assert re.search(r"pub fn %s\(" % name, text("integration", "mi355x_sys.rs"))


def test_cpp_header_has_the_mirrors():
    hpp = text("include", "kzg_mi355x.hpp")
    for fn in ("ntt_batch", "coset_ntt_batch", "fft_many", "ifft_many", "coset_fft_many", "icoset_fft_many"):
        assert re.search(r"\bvoid %s\(const Engine &e" % fn, hpp), fn


def test_python_mirrors_exist():
    import kzg_amd
    for fn in ("ntt_batch", "coset_ntt_batch"):
        assert callable(getattr(kzg_amd.Engine, fn))
    for fn in ("fft_many", "ifft_many", "coset_fft_many", "icoset_fft_many"):
        assert callable(getattr(kzg_amd.EvaluationDomain, fn))


class NoEngine:
    """any use of the engine fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched (%s)" % name)


@pytest.mark.parametrize("fn", ["fft_many", "ifft_many", "coset_fft_many", "icoset_fft_many"])
def test_many_rejects_mixed_sizes_before_any_call(fn):
    import kzg_amd
    a = kzg_amd.EvaluationDomain.from_coeffs([1, 2, 3, 4])
    b = kzg_amd.EvaluationDomain.from_coeffs([1, 2, 3, 4, 5, 6, 7, 8])
    with pytest.raises(ValueError):
        getattr(kzg_amd.EvaluationDomain, fn)(NoEngine(), [a, b])
    assert a.coeffs == [1, 2, 3, 4] and b.coeffs == [1, 2, 3, 4, 5, 6, 7, 8]
