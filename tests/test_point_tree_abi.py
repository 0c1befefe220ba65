"""CPU-side checks of kzg_point_tree_*: the header declares the calls with their option and their limit and names the blocking ones
among the concurrent calls, the library exports them, the Python signature table, the C++ mirror and the Rust declarations hold them,
the api has its classes and methods, the one-point quirk needs no engine, and without a GPU every call fails loudly on a NULL
context."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"kzg_point_tree_setup": 5, "kzg_point_tree_shape": 5, "kzg_point_tree_product": 5, "kzg_point_tree_eval": 8,
         "kzg_point_tree_combine": 7, "kzg_point_tree_interpolate": 7}
BLOCKING = ["kzg_point_tree_product", "kzg_point_tree_eval", "kzg_point_tree_combine", "kzg_point_tree_interpolate"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls():
    src = re.sub(r"/\*.*?\*/", "", read("include", "kzg_mi355x.h"), flags=re.S)
    return {m.group(2): m.group(3) for m in re.finditer(r"\b(int|void)\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_calls_the_option_and_the_limit():
    decls = header_decls()
    for name, nargs in list(CALLS.items()) + [("kzg_point_tree_free", 2)]:
        assert name in decls, f"{name} is not declared in include/kzg_mi355x.h"
        assert len(decls[name].split(",")) == nargs, decls[name]
    hdr = read("include", "kzg_mi355x.h")
    assert "typedef struct kzg_point_tree kzg_point_tree;" in hdr
    assert hdr.index("int kzg_interpolate(") < hdr.index("int kzg_point_tree_setup(") < hdr.index("int kzg_quotient_linear(")  # next to kzg_interpolate
    assert '"point_tree_leaf"' in hdr
    limits = hdr[hdr.index("/* Limits"):hdr.index("typedef struct kzg_ctx")]
    assert re.search(r"kzg_point_tree_setup\s+1 <= k <= 2\^22", limits)
    opening = hdr[:hdr.index("#ifndef KZG_MI355X_H")]  # the calls that run concurrently on one context
    for name in BLOCKING:
        assert name in opening, name
    doc = hdr[hdr.index("SubProductTree (src/polynomial.rs:303-365)"):hdr.index("typedef struct kzg_point_tree")]
    assert "xs.len() > degree" in doc and "zero remainder" in doc  # what the call does where the reference asserts / panics


def test_library_exports_them_and_the_table_holds_them():
    import kzg_amd
    lib = kzg_amd.load()
    for name, nargs in list(CALLS.items()) + [("kzg_point_tree_free", 2)]:
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = lib._kzg_signatures[name]
        assert len(args) == nargs, name


def test_source_is_built_with_the_library_and_declares_its_internals():
    from kzg_amd import build
    assert "point_tree.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "kzg_amd", "csrc", "point_tree.hip"))
    common = read("kzg_amd", "csrc", "common.h")
    assert "series_inverse_run(" in common and "pt_ntt_run(" in common and "opt_point_tree_leaf" in common
    assert "series_inverse_run(" in read("kzg_amd", "csrc", "poly_divide.hip") and "series_inverse_run(" in read("kzg_amd", "csrc", "point_tree.hip")


def test_hpp_mirror_and_rust_declarations_hold_them():
    hpp, rs = read("include", "kzg_mi355x.hpp"), read("integration", "mi355x_sys.rs")
    for name in list(CALLS) + ["kzg_point_tree_free"]:
        assert re.search(r"\b%s\s*\(" % name, hpp), f"{name} is not used in include/kzg_mi355x.hpp"
        assert re.search(r"pub fn %s\s*\(" % name, rs), f"{name} is missing from integration/mi355x_sys.rs"
    assert "kzg_point_tree" in re.sub(r"pub fn .*", "", rs)  # the opaque type
    assert re.search(r"\bclass PointTree\b", hpp)
    for method in ("new_from_points", "product", "eval", "eval_batch", "linear_mod_combination", "interpolate", "lagrange_interpolation_with_tree"):
        assert re.search(r"\b%s\s*\(" % method, hpp), method


def test_python_api_has_the_classes_and_methods():
    import kzg_amd
    from kzg_amd import api
    assert kzg_amd.PointTree is api.PointTree
    for method in ("new_from_points", "product", "eval", "eval_batch", "linear_mod_combination", "interpolate", "close", "__enter__", "__exit__"):
        assert hasattr(api.PointTree, method), method
    assert hasattr(api.Engine, "point_tree") and hasattr(api.Polynomial, "lagrange_interpolation_with_tree")


def test_one_point_interpolation_is_the_reference_quirk_without_an_engine():
    from kzg_amd import api
    p = api.Polynomial.lagrange_interpolation_with_tree(None, [7], [9], None)  # src/polynomial.rs:244-247: X + (y - x)
    assert (p.coeffs, p.degree) == ([2, 1], 1)
    p = api.Polynomial.lagrange_interpolation_with_tree(None, [9], [7], None)
    assert (p.coeffs, p.degree) == ([api.R_MODULUS - 2, 1], 1)
    with pytest.raises(api.ReferencePanic):
        api.Polynomial.lagrange_interpolation_with_tree(None, [1, 2], [3], None)


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    assert lib.kzg_point_tree_setup(None, None, 1, 1, None) == 3
    assert lib.kzg_point_tree_shape(None, None, None, None, None) == 3
    assert lib.kzg_point_tree_product(None, None, 1, 0, None) == 3
    assert lib.kzg_point_tree_eval(None, None, None, 1, 1, 1, 0, None) == 3
    assert lib.kzg_point_tree_combine(None, None, None, 1, 1, 0, None) == 3
    assert lib.kzg_point_tree_interpolate(None, None, None, 1, 1, 0, None) == 3
    lib.kzg_point_tree_free(None, None)
