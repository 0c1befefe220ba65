"""CPU-side checks of kzg_msm_g2_bucket, kzg_witness_coeff_tree and kzg_verify_eval_tree: the header declares them with their options and their limit, the
test header declares the g2_madd hook as an entry point of its own, the library exports them, the Python signature table, the C++
mirror and the Rust declarations hold them, the api has its methods, and without a GPU every call fails loudly on a NULL context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"kzg_msm_g2_bucket": 9, "kzg_verify_eval_tree": 11, "kzg_witness_coeff_tree": 13}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls(name="kzg_mi355x.h"):
    src = re.sub(r"/\*.*?\*/", "", read("include", name), flags=re.S)
    return {m.group(2): m.group(3) for m in re.finditer(r"\b(int|void)\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_calls_the_options_and_the_limit():
    decls = header_decls()
    for name, nargs in CALLS.items():
        assert name in decls, f"{name} is not declared in include/kzg_mi355x.h"
        assert len(decls[name].split(",")) == nargs, decls[name]
    hdr = read("include", "kzg_mi355x.h")
    assert hdr.index("int kzg_msm_g2(") < hdr.index("int kzg_msm_g2_bucket(") < hdr.index("int kzg_pairing_check(")  # next to kzg_msm_g2
    assert hdr.index("int kzg_verify_eval_batched(") < hdr.index("int kzg_verify_eval_tree(") < hdr.index("int kzg_verify_eval_all(")
    assert '"g2_msm_slice"' in hdr and '"g2_msm_slots"' in hdr
    limits = hdr[hdr.index("/* Limits"):hdr.index("typedef struct kzg_ctx")]
    assert re.search(r"kzg_msm_g2_bucket\s+any n the SRS holds", limits) and "18.9 MB" in limits
    assert hdr.index("int kzg_verify_eval_batched(") < hdr.index("int kzg_witness_coeff_tree(") < hdr.index("int kzg_verify_eval_tree(")
    assert re.search(r"kzg_witness_coeff_tree\s+the plan's 1 <= k <= 2\^22, n <= 2\^27", limits)
    assert hdr.count("typedef struct kzg_point_tree kzg_point_tree;") == 1


def test_the_hook_is_an_entry_point_of_its_own():
    decls = header_decls("kzg_mi355x_test.h")
    assert len(decls["kzg_test_g2_madd"].split(",")) == 5
    th = read("include", "kzg_mi355x_test.h")
    assert "KZG_TOWER_NUM_OPS = 22" in th and "KZG_ARITH_NUM_OPS = 25" in th  # the op tables keep their lengths


def test_library_exports_them_and_the_table_holds_them():
    import kzg_amd
    lib = kzg_amd.load()
    for name, nargs in CALLS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = lib._kzg_signatures[name]
        assert len(args) == nargs, name
    assert not hasattr(lib, "kzg_test_g2_madd")  # the product library holds no hooks


def test_sources_are_built_with_the_library():
    from kzg_amd import build
    for src in ("g2_msm.hip", "witness_tree.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(ROOT, "kzg_amd", "csrc", src))
    assert "g2_msm.hip" in build.HOOK_SOURCES
    assert "g2_madd(" in read("kzg_amd", "csrc", "tower.h")
    common = read("kzg_amd", "csrc", "common.h")
    assert "opt_g2_msm_slice" in common and "opt_g2_msm_slots" in common
    for fn in ("poly_divisor_run(", "poly_dividend_run(", "point_tree_interpolate_run("):  # the device-level entries the prover joins
        assert fn in common and fn in read("kzg_amd", "csrc", "witness_tree.hip"), fn
    assert "poly_dividend_run(" in read("kzg_amd", "csrc", "poly_divide.hip").split('extern "C" int kzg_poly_divide(')[1]  # one body, two callers


def test_hpp_mirror_and_rust_declarations_hold_them():
    hpp, rs = read("include", "kzg_mi355x.hpp"), read("integration", "mi355x_sys.rs")
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hpp), f"{name} is not used in include/kzg_mi355x.hpp"
        assert re.search(r"pub fn %s\s*\(" % name, rs), f"{name} is missing from integration/mi355x_sys.rs"
    assert re.search(r"\bmsm_g2_bucket\s*\(", hpp) and re.search(r"\bbool verify\s*\(", hpp) and re.search(r"\bKZGWitness create_witness\s*\(const KZGParams", hpp)
    assert "plan: *const kzg_point_tree" in rs


def test_python_api_has_the_methods():
    from kzg_amd import api
    assert hasattr(api.SrsG2, "msm_bucket")
    assert hasattr(api.PointTree, "create_witness") and hasattr(api.PointTree, "create_witness_batch")
    assert hasattr(api.KZGProver, "create_witness_batched_with_tree")
    assert hasattr(api.KZGVerifier, "verify_eval_batched_with_tree") and hasattr(api.KZGVerifier, "verify_eval_batched_with_tree_many")


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    assert lib.kzg_msm_g2_bucket(None, None, 0, None, 0, 1, 0, None, 0) == 3
    assert lib.kzg_verify_eval_tree(None, None, None, None, None, 1, None, None, 0, 0, None) == 3
    assert lib.kzg_witness_coeff_tree(None, None, None, None, 1, 1, None, 1, 0, None, 0, None, None) == 3
