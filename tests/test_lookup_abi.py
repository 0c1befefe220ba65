"""kzg_lookup_setup / _free / _shape / _count and kzg_logup_terms: the declarations of the header and their mirrors (ctypes table, C++
header, Rust binding, Python classes).  No GPU: nothing here creates a context."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "kzg_lookup_setup": "int kzg_lookup_setup(kzg_ctx *ctx, const void *table, size_t n_t, int sfmt, int flags, kzg_lookup **out);",
    "kzg_lookup_free": "void kzg_lookup_free(kzg_ctx *ctx, kzg_lookup *plan);",
    "kzg_lookup_shape": "int kzg_lookup_shape(const kzg_lookup *plan, size_t *n_t, size_t *distinct, size_t *bytes);",
    "kzg_lookup_count": "int kzg_lookup_count(kzg_ctx *ctx, const kzg_lookup *plan, const void *values, size_t n, size_t batch, int sfmt, int flags, "
                        "void *mult_out, uint32_t *index_out, size_t *missing, size_t *first_missing);",
    "kzg_logup_terms": "int kzg_logup_terms(kzg_ctx *ctx, const void *values, const void *table, const void *mult, const void *beta, size_t n, size_t t, "
                       "size_t batch, int sfmt, int flags, void *out, int *zero_den);",
}
CTYPES = {"kzg_ctx *": ctypes.c_void_p, "const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
          "size_t *": ctypes.POINTER(ctypes.c_size_t), "int *": ctypes.POINTER(ctypes.c_int), "uint32_t *": ctypes.POINTER(ctypes.c_uint32),
          "kzg_lookup *": ctypes.c_void_p, "const kzg_lookup *": ctypes.c_void_p, "kzg_lookup **": ctypes.POINTER(ctypes.c_void_p)}
OPTIONS = ('"lookup_spare_log"', '"lookup_hash_bits"', '"lookup_stage"', '"lookup_chunk"')
LEASE_CALLS = ("kzg_lookup_setup", "kzg_lookup_count", "kzg_logup_terms")


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_call(name):
    assert SIGNATURES[name] in squeeze(text("include", "kzg_mi355x.h"))


def test_header_declares_the_type_and_documents_options_and_limits():
    hdr = squeeze(text("include", "kzg_mi355x.h"))
    assert "typedef struct kzg_lookup kzg_lookup;" in hdr
    # the options, in the comment of kzg_ctx_set_option (it ends at the prototype)
    options = hdr[hdr.index('"window_bits"'):hdr.index("int kzg_ctx_set_option(")]
    for key in OPTIONS:
        assert key in options, key
    # the Limits block ends where the SRS footprint begins
    limits = hdr[hdr.index("/* Limits"):hdr.index("SRS footprint in HBM")]
    for name in LEASE_CALLS:
        assert name in limits, name
    assert "32 B per key plus the slot array" in limits and "one uint32_t counter per table row and vector" in limits
    # the calls that lease a lane are in the list of calls that run concurrently on one context (it ends at the reference's types)
    concurrent = hdr[hdr.index("The reference's blocking calls"):hdr.index("run CONCURRENTLY")]
    for name in LEASE_CALLS:
        assert name in concurrent, name
    assert "kzg_fr_lincomb first" in hdr          # tables of several columns are the caller's business


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_ctypes_binding_matches_the_header(name):
    import kzg_amd
    lib = kzg_amd.load()
    sig = SIGNATURES[name]
    params = sig[sig.index("(") + 1:sig.index(")")].split(", ")
    want = [CTYPES[re.sub(r"\w+$", "", p).strip()] for p in params]
    restype, argtypes = lib._kzg_signatures[name]
    assert restype is (None if sig.startswith("void") else ctypes.c_int) and list(argtypes) == want
    assert list(getattr(lib, name).argtypes) == want


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_cpp_and_rust_name_the_call(name):
    assert re.search(r"\b%s\(" % name, text("include", "kzg_mi355x.hpp"))
    assert re.search(r"pub fn %s\(" % name, text("integration", "mi355x_sys.rs"))


def test_rust_binding_has_the_opaque_type():
    assert "pub struct kzg_lookup { _p: [u8; 0] }" in text("integration", "mi355x_sys.rs")
    assert "out: *mut *mut kzg_lookup" in text("integration", "mi355x_sys.rs")


def test_cpp_header_has_the_mirrors():
    hpp = text("include", "kzg_mi355x.hpp")
    assert re.search(r"\bclass LookupTable \{", hpp)
    assert "LookupTable(const LookupTable &) = delete;" in hpp and "kzg_lookup_free(" in hpp      # RAII, like PointTree
    assert re.search(r"\blookup_count\(const LookupTable &plan", hpp) and re.search(r"\blogup_terms\(const Engine &e", hpp)


def test_python_mirrors_exist():
    import kzg_amd
    assert kzg_amd.LookupTable is kzg_amd.api.LookupTable
    for fn in ("count", "free", "shape"):
        assert callable(getattr(kzg_amd.LookupTable, fn))
    for fn in ("lookup_table", "logup_terms", "logup_accumulator"):
        assert callable(getattr(kzg_amd.Engine, fn))


def test_the_model_follows_the_owner_rule():
    from tests import lookup_model as LM
    R = LM.R
    mult, idx, missing, first = LM.multiplicities([5, 7, 5, 9 + R], [5, 9, 8, 5 + R, 7, 11])
    assert (mult, idx, missing, first) == ([2, 1, 0, 1], [0, 3, LM.NONE, 0, 1, LM.NONE], 2, 2)
    out, zd = LM.logup_terms([[5, 7]], [5, 7], [1, 1], 3)
    assert (out, zd) == ([0, 0], 0)
    assert LM.logup_terms([[5, R - 3]], None, None, 3) == ([0, 0], 1)


def test_null_context_is_a_shape_error():
    import kzg_amd
    from kzg_amd import _lib as L
    lib = kzg_amd.load()
    word = ctypes.create_string_buffer(32)
    h = ctypes.c_void_p(0x1234)
    idx, miss = (ctypes.c_uint32 * 1)(77), (ctypes.c_size_t * 2)(88, 99)
    zd = (ctypes.c_int * 1)(-7)
    assert lib.kzg_lookup_setup(None, word, 1, L.FR_CANONICAL, 0, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert h.value == 0x1234
    assert lib.kzg_lookup_count(None, None, word, 1, 1, L.FR_CANONICAL, 0, word, idx, miss, ctypes.cast(ctypes.byref(miss, ctypes.sizeof(ctypes.c_size_t)), ctypes.POINTER(ctypes.c_size_t))) == L.KZG_ERR_SHAPE
    assert lib.kzg_logup_terms(None, word, word, word, word, 1, 1, 1, L.FR_CANONICAL, 0, word, zd) == L.KZG_ERR_SHAPE
    assert lib.kzg_lookup_shape(None, miss, None, None) == L.KZG_ERR_SHAPE
    lib.kzg_lookup_free(None, None)               # a NULL plan is nothing to free
    assert word.raw == bytes(32) and idx[0] == 77 and list(miss) == [88, 99] and zd[0] == -7
