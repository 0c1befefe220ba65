"""kzg_mle_eq / kzg_mle_bind / kzg_mle_eval / kzg_fr_program_degree / kzg_sumcheck_round: the declarations of the header and their mirrors
(ctypes table, C++ header, Rust binding, Python classes), and the host-only code of mle.hip through tests/cpp_mle_test.cpp.  No GPU:
nothing here creates a context."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "kzg_mle_eq": "int kzg_mle_eq(kzg_ctx *ctx, const void *point, size_t m, int sfmt, int flags, void *out);",
    "kzg_mle_bind": "int kzg_mle_bind(kzg_ctx *ctx, const void *const *cols, size_t n_cols, size_t n, const void *rho, int sfmt, int flags, "
                    "void *const *outs);",
    "kzg_mle_eval": "int kzg_mle_eval(kzg_ctx *ctx, const void *tables, size_t m, size_t batch, const void *point, int sfmt, int flags, void *ys_out, "
                    "void *quotients_out);",
    "kzg_fr_program_degree": "int kzg_fr_program_degree(const kzg_fr_program *plan, size_t *degrees);",
    "kzg_sumcheck_round": "int kzg_sumcheck_round(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const void *consts, size_t n, "
                          "size_t n_eval, int sfmt, int flags, void *sums_out);",
}
OPTIONS = ("sumcheck_block", "sumcheck_grid", "mle_block", "mle_local_log", "mle_eval_chunk")
VPP = ctypes.POINTER(ctypes.c_void_p)
CTYPES = {"kzg_ctx *": ctypes.c_void_p, "const void *": ctypes.c_void_p, "void *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
          "size_t *": ctypes.POINTER(ctypes.c_size_t), "const kzg_fr_program *": ctypes.c_void_p, "const void *const *": VPP, "void *const *": VPP}


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_call(name):
    hdr = squeeze(text("include", "kzg_mi355x.h"))
    assert SIGNATURES[name] in hdr
    # in a block of their own behind kzg_fr_program_run
    assert hdr.index("int kzg_fr_program_run(") < hdr.index(SIGNATURES[name])


def test_header_has_the_constants_and_documents_options_limits_and_concurrency():
    hdr = squeeze(text("include", "kzg_mi355x.h"))
    assert "enum { KZG_SUMCHECK_MAX_EVAL = 16, KZG_SUMCHECK_MAX_ACC = 32 };" in hdr
    options = hdr[hdr.index('"window_bits"'):hdr.index("int kzg_ctx_set_option(")]      # the comment of kzg_ctx_set_option ends at the prototype
    for opt in OPTIONS:
        assert '"%s"' % opt in options, opt
    limits = hdr[hdr.index("/* Limits"):hdr.index("SRS footprint in HBM")]
    for name in ("kzg_mle_eq", "kzg_mle_bind", "kzg_mle_eval", "kzg_sumcheck_round"):
        assert name in limits, name
    assert "HOST column whole" in limits and "one partial sum of 32 B" in limits and "does not grow with batch" in limits
    concurrent = hdr[hdr.index("The reference's blocking calls"):hdr.index("run CONCURRENTLY")]
    for name in ("kzg_mle_eq", "kzg_mle_bind", "kzg_mle_eval", "kzg_sumcheck_round"):
        assert name in concurrent, name
    # the conventions are in the header comment
    block = hdr[hdr.index("sumcheck rounds on the device"):hdr.index("enum { KZG_SUMCHECK_MAX_EVAL")]
    for phrase in ("bit j of i", "bind the TOP variable", "point[m - 1 - k]", "outs[c] == cols[c] EXACTLY", "b (n - 1) + 2^k - 1", "n_eval = degree + 1",
                   "a rotation has no meaning on the hypercube"):
        assert phrase in block, phrase


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_ctypes_binding_matches_the_header(name):
    import kzg_amd
    lib = kzg_amd.load()
    sig = SIGNATURES[name]
    params = sig[sig.index("(") + 1:sig.index(")")].split(", ")
    want = [CTYPES[re.sub(r"\w+$", "", p).strip()] for p in params]
    restype, argtypes = lib._kzg_signatures[name]
    assert restype is ctypes.c_int and list(argtypes) == want
    assert list(getattr(lib, name).argtypes) == want


def test_python_constants_are_the_headers():
    from kzg_amd import _lib as L
    hdr = text("include", "kzg_mi355x.h")
    for name in ("MAX_EVAL", "MAX_ACC"):
        assert int(re.search(r"\bKZG_SUMCHECK_%s = (\d+)" % name, hdr).group(1)) == getattr(L, "SUMCHECK_" + name), name


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_cpp_and_rust_name_the_call(name):
    assert re.search(r"\b%s\(" % name, text("include", "kzg_mi355x.hpp"))
    assert re.search(r"pub fn %s\(" % name, text("integration", "mi355x_sys.rs"))


def test_rust_and_cpp_mirrors():
    rs = text("integration", "mi355x_sys.rs")
    assert "pub const KZG_SUMCHECK_MAX_EVAL: c_int = 16;" in rs and "pub const KZG_SUMCHECK_MAX_ACC: c_int = 32;" in rs
    assert "pub fn kzg_mle_bind(ctx: *mut kzg_ctx, cols: *const *const c_void, n_cols: usize, n: usize, rho: *const c_void, sfmt: c_int, flags: c_int, outs: *const *mut c_void) -> c_int;" in rs
    assert "pub fn kzg_fr_program_degree(plan: *const kzg_fr_program, degrees: *mut usize) -> c_int;" in rs
    hpp = text("include", "kzg_mi355x.hpp")
    for fn in ("mle_eq", "mle_bind", "mle_eval", "sumcheck_round"):
        assert re.search(r"\binline std::vector<[^;{]*\b%s\(" % fn, hpp), fn
    assert re.search(r"std::vector<size_t> degrees\(\) const", hpp)


def test_python_mirrors_exist():
    import kzg_amd
    for fn in ("mle_eq", "mle_bind", "mle_eval", "sumcheck_round"):
        assert callable(getattr(kzg_amd.Engine, fn)), fn
    assert callable(kzg_amd.FrProgram.degrees) and callable(kzg_amd.FrProgram.sumcheck_round)
    assert callable(kzg_amd.sumcheck.prove) and callable(kzg_amd.sumcheck.verify)
    # the verifier needs no device: s(X) = 3 X^2 + 1 over one round, claim s(0) + s(1) = 5, ending in s(rho)
    rho = 7
    s = [1, 4, 13]
    assert kzg_amd.sumcheck.verify([5], [[s]], [rho], [0], lambda finals: [3 * rho * rho + 1])
    assert not kzg_amd.sumcheck.verify([6], [[s]], [rho], [0], lambda finals: [3 * rho * rho + 1])
    assert not kzg_amd.sumcheck.verify([5], [[s]], [rho], [0], lambda finals: [3 * rho * rho])


def test_the_build_compiles_the_new_translation_unit():
    from kzg_amd import build
    assert "mle.hip" in build.SOURCES
    for f in ("mle.hip", "fr_program.h", "mle_host.h"):
        assert os.path.exists(os.path.join(ROOT, "kzg_amd", "csrc", f)), f
    # the interpreter's shared pieces moved, they were not copied
    hip = text("kzg_amd", "csrc", "fr_program.hip")
    assert '#include "fr_program.h"' in hip and "struct FrpCol {" not in hip and "Fr frp_load(" not in hip


def test_null_context_is_a_shape_error_that_writes_nothing():
    import kzg_amd
    from kzg_amd import _lib as L
    lib = kzg_amd.load()
    one = (1).to_bytes(32, "little")
    out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    col = ctypes.create_string_buffer(b"\x11" * 64, 64)
    cp, op = (ctypes.c_void_p * 1)(ctypes.addressof(col)), (ctypes.c_void_p * 1)(ctypes.addressof(out))
    assert lib.kzg_mle_eq(None, one, 1, L.FR_CANONICAL, 0, out) == L.KZG_ERR_SHAPE
    assert lib.kzg_mle_bind(None, cp, 1, 2, one, L.FR_CANONICAL, 0, op) == L.KZG_ERR_SHAPE
    assert lib.kzg_mle_eval(None, col, 1, 1, one, L.FR_CANONICAL, 0, out, None) == L.KZG_ERR_SHAPE
    assert lib.kzg_sumcheck_round(None, None, cp, None, 2, 3, L.FR_CANONICAL, 0, out) == L.KZG_ERR_SHAPE
    d = (ctypes.c_size_t * 2)(77, 77)
    assert lib.kzg_fr_program_degree(None, d) == L.KZG_ERR_SHAPE
    assert out.raw == b"\xa5" * 64 and col.raw == b"\x11" * 64 and list(d) == [77, 77]


def test_host_code_through_the_stand_alone_program(tmp_path):
    """tests/cpp_mle_test.cpp: the degree bound, the accumulator rule and the aliasing rules of kzg_amd/csrc/mle_host.h, no library linked"""
    exe = str(tmp_path / "cpp_mle_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp_mle_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
