"""CPU-side checks of kzg_ntt_g1 / kzg_ntt_g2: the header declares them with their limits and options, the library exports them, the
Python signature table, the C++ mirror and the Rust declarations hold them, the api has its methods, the hooks library's host-side
recoding agrees with the model, and without a GPU every call fails loudly on a NULL context."""
import ctypes
import os
import random
import re

from tests import group_ntt_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"kzg_ntt_g1": 9, "kzg_ntt_g2": 9}
OPTIONS = ["g2_ntt_mul", "group_ntt_chunk_points", "group_ntt_threads", "g2_lagrange_dft_from"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def header_decls(name="kzg_mi355x.h"):
    src = re.sub(r"/\*.*?\*/", "", read("include", name), flags=re.S)
    return {m.group(2): m.group(3) for m in re.finditer(r"\b(int|void)\s+(kzg_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_calls_the_options_and_the_limits():
    decls = header_decls()
    for name, nargs in CALLS.items():
        assert name in decls, f"{name} is not declared in include/kzg_mi355x.h"
        args = [a.strip() for a in decls[name].split(",")]
        assert len(args) == nargs, decls[name]
        assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "points", "log_n", "batch", "inverse", "pfmt", "flags", "out", "ofmt"]
    hdr = read("include", "kzg_mi355x.h")
    for opt in OPTIONS:
        assert '"%s"' % opt in hdr, opt
    limits = hdr[hdr.index("/* Limits"):hdr.index("typedef struct kzg_ctx")]
    assert re.search(r"kzg_ntt_g1 / kzg_ntt_g2\s+log_n <= 22 / log_n <= 20", limits)
    assert re.search(r"_g2: d <= 2\^20", limits) and "d <= 1024" not in hdr
    hooks = header_decls("kzg_mi355x_test.h")
    assert len(hooks["kzg_test_g2_mul_gls"].split(",")) == 6 and len(hooks["kzg_test_g2_gls_recode"].split(",")) == 3


def test_library_exports_them_and_the_table_holds_them():
    import kzg_amd
    lib = kzg_amd.load()
    for name, nargs in CALLS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = lib._kzg_signatures[name]
        assert len(args) == nargs, name
    assert not hasattr(lib, "kzg_test_g2_mul_gls")  # hooks stay out of the product library


def test_source_is_built_with_the_library():
    from kzg_amd import build
    assert "g2ntt.hip" in build.SOURCES and "g2ntt.hip" in build.HOOK_SOURCES
    src = read("kzg_amd", "csrc", "g2ntt.hip")
    for kernel in ("k_g2ntt_dif", "k_g2ntt_dit", "k_g2ntt_trivial", "k_g2ntt_load", "k_g2ntt_finish", "k_g2_twiddles"):
        assert kernel in src, kernel
    assert "g2_psi_limb" in read("kzg_amd", "csrc", "tower_consts.inc") and "g2_psi_limb" in read("tools", "gen_tower_consts.py")
    common = read("kzg_amd", "csrc", "common.h")
    for opt in OPTIONS:
        assert "opt_" + opt in common, opt


def test_hpp_mirror_and_rust_declarations_hold_them():
    hpp, rs = read("include", "kzg_mi355x.hpp"), read("integration", "mi355x_sys.rs")
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hpp), f"{name} is not used in include/kzg_mi355x.hpp"
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, rs)
        assert m, f"{name} is missing from integration/mi355x_sys.rs"
        assert len(m.group(1).split(",")) == CALLS[name]
    assert re.search(r"std::vector<G1Affine> ntt_g1\(", hpp) and re.search(r"std::vector<G2Affine> ntt_g2\(", hpp)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp_group_ntt_test.cpp"))


def test_python_api_has_the_methods():
    from kzg_amd import api
    assert hasattr(api.Engine, "ntt_g1") and hasattr(api.Engine, "ntt_g2")
    assert hasattr(api.Srs, "dft") and hasattr(api.SrsG2, "dft")
    assert "2^20" in api.compute_lagrange_basis_g2.__doc__ and "1024" not in api.compute_lagrange_basis_g2.__doc__


def test_host_recoding_of_the_hooks_library_is_the_models():
    import kzg_amd
    kzg_amd.load()
    lib = ctypes.CDLL(os.path.join(os.path.dirname(kzg_amd.__file__), "libkzg_mi355x_hooks.so"))
    fn = lib.kzg_test_g2_gls_recode
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int8)]
    fn.restype = ctypes.c_int
    rng = random.Random(77)
    for k in G.EDGE_SCALARS + [rng.randrange(G.R) for _ in range(50)]:
        words, digits = (ctypes.c_uint64 * 4)(), (ctypes.c_int8 * 68)()
        assert fn(k.to_bytes(32, "little"), words, digits) == 0
        ks = G.split_u(k)
        assert list(words) == ks, hex(k)
        assert list(digits) == [d for v in ks for d in G.recode64(v)], hex(k)
    assert fn(None, None, None) == 3


def test_null_context_is_a_shape_error_not_a_crash():
    import kzg_amd
    lib = kzg_amd.load()
    buf = ctypes.create_string_buffer(192)
    assert lib.kzg_ntt_g1(None, buf, 0, 1, 0, 0, 0, buf, 0) == 3
    assert lib.kzg_ntt_g2(None, buf, 0, 1, 0, 0, 0, buf, 0) == 3
