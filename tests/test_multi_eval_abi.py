"""CPU-side checks of kzg_poly_multi_eval and kzg_interpolate: the header declares them, the library exports them, the Python signature
table and the C++ mirror hold them, the Rust declarations carry them, the api has its methods, and without a GPU the calls fail
loudly on a NULL context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    # name: number of arguments
    "kzg_poly_multi_eval": 9,
    "kzg_interpolate": 8,
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls():
    src = re.sub(r"/\*.*?\*/", "", read("include", "kzg_mi355x.h"), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_both_calls_their_options_and_their_limits():
    decls = header_decls()
    for name, nargs in CALLS.items():
        assert name in decls, f"{name} is not declared in include/kzg_mi355x.h"
        assert len(decls[name].split(",")) == nargs, f"{name}: {decls[name]}"
    hdr = read("include", "kzg_mi355x.h")
    assert '"multi_eval_segment"' in hdr and '"multi_eval_points_chunk"' in hdr
    limits = hdr[hdr.index("/* Limits"):hdr.index("typedef struct kzg_ctx")]
    assert re.search(r"kzg_poly_multi_eval\s+n <= 2\^28", limits) and re.search(r"kzg_interpolate\s+k <= 16384", limits)
    opening = hdr[:hdr.index("#ifndef KZG_MI355X_H")]  # the calls that run concurrently on one context
    assert "kzg_poly_multi_eval" in opening and "kzg_interpolate" in opening


def test_library_exports_them_and_the_table_holds_them():
    import kzg_amd
    lib = kzg_amd.load()
    for name, nargs in CALLS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = lib._kzg_signatures[name]
        assert len(args) == nargs, f"{name}: the signature table has {len(args)} arguments, the header {nargs}"


def test_hpp_mirror_and_rust_declarations_hold_them():
    hpp, rs = read("include", "kzg_mi355x.hpp"), read("integration", "mi355x_sys.rs")
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hpp), f"{name} has no wrapper in include/kzg_mi355x.hpp"
        assert re.search(r"pub fn %s\s*\(" % name, rs), f"{name} is missing from integration/mi355x_sys.rs"
    for wrapper in ("poly_multi_eval", "interpolate", "multi_eval", "lagrange_interpolation"):
        assert re.search(r"\b%s\s*\(" % wrapper, hpp), wrapper


def test_python_api_has_the_methods():
    from kzg_amd import api
    assert hasattr(api.Engine, "poly_multi_eval") and hasattr(api.Engine, "interpolate")
    assert hasattr(api.Polynomial, "multi_eval") and hasattr(api.Polynomial, "lagrange_interpolation")
    assert hasattr(api.KZGProver, "open_at_points")


def test_the_mirror_panics_where_the_reference_does_before_any_call():
    import pytest
    from kzg_amd import api
    p = api.Polynomial([1, 2, 3])
    with pytest.raises(api.ReferencePanic):  # assert!(xs.len() > self.degree())
        p.multi_eval(None, [5, 6])
    with pytest.raises(api.ReferencePanic):  # assert_eq!(xs.len(), ys.len())
        api.Polynomial.lagrange_interpolation(None, [1, 2], [3])
    one = api.Polynomial.lagrange_interpolation(None, [7], [3])  # X + (y - x), src/polynomial.rs:269-272
    assert one.coeffs == [api.R_MODULUS - 4, 1] and one.degree == 1


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    KZG_ERR_SHAPE = lib.kzg_poly_multi_eval(None, None, 1, 1, None, 1, 0, 0, None)
    assert KZG_ERR_SHAPE == 3
    assert lib.kzg_interpolate(None, None, None, 1, 1, 0, 0, None) == KZG_ERR_SHAPE
