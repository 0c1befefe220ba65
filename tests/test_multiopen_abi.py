"""CPU-side checks of the multiproof calls: the header declares them, the library exports them, the Python signature table and the C++
mirror hold them, the Rust declarations carry them, and without a GPU they fail loudly on a NULL context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    # name: number of arguments
    "kzg_fr_lincomb": 10,
    "kzg_multiopen_eval_commit": 15,
    "kzg_multiopen_eval_finish": 16,
    "kzg_multiopen_coeff_commit": 15,
    "kzg_multiopen_coeff_finish": 16,
    "kzg_verify_multiopen": 16,
}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls():
    src = re.sub(r"/\*.*?\*/", "", read("include", "kzg_mi355x.h"), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_six_calls_and_says_what_the_caller_owes():
    decls = header_decls()
    for name, nargs in CALLS.items():
        assert name in decls, f"{name} is not declared in include/kzg_mi355x.h"
        assert len(decls[name].split(",")) == nargs, f"{name}: {decls[name]}"
    hdr = read("include", "kzg_mi355x.h")
    assert "multiopen_points_chunk" in hdr
    assert re.search(r"t MUST BE DRAWN AFTER D", hdr) and "KZG_ERR_ALLOC" in hdr


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
    for wrapper in ("fr_lincomb", "multiopen_commit", "multiopen_finish", "verify_multiopen"):
        assert re.search(r"\b%s\s*\(" % wrapper, hpp), wrapper


def test_python_api_has_the_methods():
    from kzg_amd import api
    assert hasattr(api.Engine, "fr_lincomb")
    for cls in (api.KZGProverEvalForm, api.KZGProver):
        assert hasattr(cls, "multiopen_commit") and hasattr(cls, "multiopen_finish") and hasattr(cls, "multiopen"), cls
    for cls in (api.KZGVerifier, api.KZGVerifierEvalForm):
        assert hasattr(cls, "verify_multiopen"), cls


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    KZG_ERR_SHAPE = lib.kzg_fr_lincomb(None, None, 1, 1, None, None, 1, 0, 0, None)
    assert KZG_ERR_SHAPE != 0
    assert lib.kzg_multiopen_eval_commit(None, None, None, 1, 1, None, None, 1, None, 0, 0, None, None, None, 0) == KZG_ERR_SHAPE
    assert lib.kzg_multiopen_eval_finish(None, None, None, 1, 1, None, None, 1, None, None, None, 0, 0, None, None, 0) == KZG_ERR_SHAPE
    assert lib.kzg_multiopen_coeff_commit(None, None, None, 1, 1, None, None, 1, None, 0, 0, None, None, None, 0) == KZG_ERR_SHAPE
    assert lib.kzg_multiopen_coeff_finish(None, None, None, 1, 1, None, None, 1, None, None, None, 0, 0, None, None, 0) == KZG_ERR_SHAPE
    assert lib.kzg_verify_multiopen(None, None, None, None, None, 0, None, 0, None, 1, None, None, None, None, 0, None) == KZG_ERR_SHAPE
