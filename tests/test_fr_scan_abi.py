"""kzg_fr_scan / kzg_fr_grand_product / kzg_fr_batch_inverse: the declarations of the header and their mirrors (ctypes table, C++ header,
Rust binding, Python methods).  No GPU: nothing here creates a context."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "kzg_fr_batch_inverse": "int kzg_fr_batch_inverse(kzg_ctx *ctx, const void *in, size_t n, int sfmt, int flags, void *out, size_t *zeros);",
    "kzg_fr_scan": "int kzg_fr_scan(kzg_ctx *ctx, const void *in, size_t n, size_t batch, int op, int exclusive, int sfmt, int flags, void *out, void *totals);",
    "kzg_fr_grand_product": "int kzg_fr_grand_product(kzg_ctx *ctx, const void *num, const void *den, size_t n, size_t t, size_t batch, int sfmt, int flags, void *z_out, void *totals, int *zero_den);",
}
CTYPES = {"kzg_ctx *": ctypes.c_void_p, "const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
          "size_t *": ctypes.POINTER(ctypes.c_size_t), "int *": ctypes.POINTER(ctypes.c_int)}


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_call(name):
    assert SIGNATURES[name] in squeeze(text("include", "kzg_mi355x.h"))


def test_header_declares_the_enum_and_documents_the_options():
    hdr = squeeze(text("include", "kzg_mi355x.h"))
    assert "enum { KZG_SCAN_PRODUCT = 0, KZG_SCAN_SUM = 1 };" in hdr
    for key in ('"fr_scan_tile"', '"fr_scan_stage"', '"fr_scan_chunk"'):
        assert key in hdr, key
    # the three calls lease a lane: they are in the list of calls that run concurrently on one context (it ends at the reference's types)
    concurrent = hdr[hdr.index("The reference's blocking calls"):hdr.index("run CONCURRENTLY")]
    for name in SIGNATURES:
        assert name in concurrent, name


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_ctypes_binding_matches_the_header(name):
    import kzg_amd
    lib = kzg_amd.load()
    params = SIGNATURES[name][SIGNATURES[name].index("(") + 1:SIGNATURES[name].index(")")].split(", ")
    want = [CTYPES[re.sub(r"\w+$", "", p).strip()] for p in params]
    restype, argtypes = lib._kzg_signatures[name]
    assert restype is ctypes.c_int and list(argtypes) == want
    assert list(getattr(lib, name).argtypes) == want


def test_enum_constants_match_the_header():
    from kzg_amd import _lib as L
    hdr = text("include", "kzg_mi355x.h")
    for c_name, value in (("KZG_SCAN_PRODUCT", L.SCAN_PRODUCT), ("KZG_SCAN_SUM", L.SCAN_SUM)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % c_name, hdr).group(1)) == value
        assert re.search(r"pub const %s: c_int = %d;" % (c_name, value), text("integration", "mi355x_sys.rs"))


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_cpp_and_rust_name_the_call(name):
    assert re.search(r"\b%s\(" % name, text("include", "kzg_mi355x.hpp"))
    assert re.search(r"pub fn %s\(" % name, text("integration", "mi355x_sys.rs"))


def test_cpp_header_has_the_mirrors():
    hpp = text("include", "kzg_mi355x.hpp")
    for fn in ("batch_inverse", "fr_scan", "grand_product"):
        assert re.search(r"\b%s\(const Engine &e" % fn, hpp), fn


def test_python_mirrors_exist():
    import kzg_amd
    for fn in ("batch_inverse", "fr_scan", "prefix_product", "prefix_sum", "grand_product"):
        assert callable(getattr(kzg_amd.Engine, fn))


def test_null_context_is_a_shape_error():
    import kzg_amd
    from kzg_amd import _lib as L
    lib = kzg_amd.load()
    word = ctypes.create_string_buffer(32)
    assert lib.kzg_fr_batch_inverse(None, word, 1, L.FR_CANONICAL, 0, word, None) == L.KZG_ERR_SHAPE
    assert lib.kzg_fr_scan(None, word, 1, 1, L.SCAN_PRODUCT, 0, L.FR_CANONICAL, 0, word, None) == L.KZG_ERR_SHAPE
    assert lib.kzg_fr_grand_product(None, word, word, 1, 1, 1, L.FR_CANONICAL, 0, word, None, None) == L.KZG_ERR_SHAPE
    assert word.raw == bytes(32)
