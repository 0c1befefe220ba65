"""CPU-side checks of kzg_poly_divide: the header declares it with its option and its limit and names it among the concurrent calls, the
library exports it, the Python signature table, the C++ mirror and the Rust declarations hold it, the api has its methods,
Polynomial.long_division returns the reference's shapes where no division is needed, and without a GPU the call fails loudly on a
NULL context."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "kzg_poly_divide", 11


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls():
    src = re.sub(r"/\*.*?\*/", "", read("include", "kzg_mi355x.h"), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_call_its_option_and_its_limit():
    decls = header_decls()
    assert NAME in decls, f"{NAME} is not declared in include/kzg_mi355x.h"
    assert len(decls[NAME].split(",")) == NARGS, decls[NAME]
    hdr = read("include", "kzg_mi355x.h")
    assert '"poly_divide_base"' in hdr
    limits = hdr[hdr.index("/* Limits"):hdr.index("typedef struct kzg_ctx")]
    assert re.search(r"kzg_poly_divide\s+na <= 2\^27", limits)
    opening = hdr[:hdr.index("#ifndef KZG_MI355X_H")]  # the calls that run concurrently on one context
    assert NAME in opening


def test_library_exports_it_and_the_table_holds_it():
    import kzg_amd
    lib = kzg_amd.load()
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    res, args = lib._kzg_signatures[NAME]
    assert len(args) == NARGS


def test_source_is_built_with_the_library():
    from kzg_amd import build
    assert "poly_divide.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "kzg_amd", "csrc", "poly_divide.hip"))


def test_hpp_mirror_and_rust_declaration_hold_it():
    hpp, rs = read("include", "kzg_mi355x.hpp"), read("integration", "mi355x_sys.rs")
    assert re.search(r"\b%s\s*\(" % NAME, hpp), f"{NAME} has no wrapper in include/kzg_mi355x.hpp"
    assert re.search(r"pub fn %s\s*\(" % NAME, rs), f"{NAME} is missing from integration/mi355x_sys.rs"
    for wrapper in ("poly_divide", "long_division"):
        assert re.search(r"\b%s\s*\(" % wrapper, hpp), wrapper


def test_python_api_has_the_methods():
    from kzg_amd import api
    assert hasattr(api.Engine, "poly_divide") and hasattr(api.Polynomial, "long_division")


def test_long_division_returns_the_reference_shapes_without_an_engine():
    from kzg_amd import api
    zero, p, d = api.Polynomial([0, 0, 0]), api.Polynomial([1, 2, 3]), api.Polynomial([4, 5, 6, 7])
    q, r = zero.long_division(None, d)           # a zero dividend: (new_zero, None)
    assert (q.coeffs, q.degree, r) == ([0], 0, None)
    with pytest.raises(api.ReferencePanic):      # "divisor must not be zero!"
        p.long_division(None, zero)
    q, r = zero.long_division(None, zero)        # the zero dividend is looked at first (src/polynomial.rs:194-199)
    assert (q.coeffs, q.degree, r) == ([0], 0, None)
    q, r = p.long_division(None, d)              # a lower degree: (new_zero, Some(self))
    assert (q.coeffs, q.degree) == ([0], 0)
    assert r is not p and (r.coeffs, r.degree) == ([1, 2, 3], 2)
    q, r = api.Polynomial([1, 2, 0, 0]).long_division(None, d)  # the degree counts, not the length
    assert (q.coeffs, q.degree) == ([0], 0) and (r.coeffs, r.degree) == ([1, 2, 0, 0], 1)


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    assert lib.kzg_poly_divide(None, None, 1, 1, None, 1, 0, 0, None, None, None) == 3
