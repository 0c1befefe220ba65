"""kzg_fr_program_setup / _free / _shape / _run: the declarations of the header and their mirrors (ctypes table, C++ header, Rust
binding, Python classes), the integer model on a hand-computed program and the expression compiler of kzg_amd.frp against direct
evaluation through the model.  No GPU: nothing here creates a context."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "kzg_fr_program_setup": "int kzg_fr_program_setup(kzg_ctx *ctx, const uint32_t *words, size_t n_insns, size_t n_cols, size_t n_consts, size_t n_out, "
                            "kzg_fr_program **out);",
    "kzg_fr_program_free": "void kzg_fr_program_free(kzg_ctx *ctx, kzg_fr_program *plan);",
    "kzg_fr_program_shape": "int kzg_fr_program_shape(const kzg_fr_program *plan, size_t *n_insns, size_t *n_cols, size_t *n_consts, size_t *n_out, "
                            "size_t *n_temps, size_t *n_mul);",
    "kzg_fr_program_run": "int kzg_fr_program_run(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const size_t *col_len, "
                          "const void *consts, size_t n, int sfmt, int flags, void *const *outs);",
}
VPP = ctypes.POINTER(ctypes.c_void_p)
CTYPES = {"kzg_ctx *": ctypes.c_void_p, "const void *": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
          "size_t *": ctypes.POINTER(ctypes.c_size_t), "const size_t *": ctypes.POINTER(ctypes.c_size_t), "const uint32_t *": ctypes.POINTER(ctypes.c_uint32),
          "kzg_fr_program *": ctypes.c_void_p, "const kzg_fr_program *": ctypes.c_void_p, "kzg_fr_program **": VPP,
          "const void *const *": VPP, "void *const *": VPP}


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_call(name):
    assert SIGNATURES[name] in squeeze(text("include", "kzg_mi355x.h"))


def test_header_declares_the_type_the_constants_and_documents_options_and_limits():
    hdr = squeeze(text("include", "kzg_mi355x.h"))
    assert "typedef struct kzg_fr_program kzg_fr_program;" in hdr
    assert "enum { KZG_FRP_ADD = 0, KZG_FRP_SUB = 1, KZG_FRP_MUL = 2 };" in hdr
    assert "enum { KZG_FRP_COL = 0, KZG_FRP_CONST = 1, KZG_FRP_TEMP = 2, KZG_FRP_OUT = 3 };" in hdr
    assert "enum { KZG_FRP_WORDS = 6, KZG_FRP_MAX_TEMPS = 16 };" in hdr
    # the option, in the comment of kzg_ctx_set_option (it ends at the prototype)
    assert '"fr_program_block"' in hdr[hdr.index('"window_bits"'):hdr.index("int kzg_ctx_set_option(")]
    # the Limits block ends where the SRS footprint begins
    limits = hdr[hdr.index("/* Limits"):hdr.index("SRS footprint in HBM")]
    assert "kzg_fr_program_setup" in limits and "kzg_fr_program_run" in limits
    assert "24 B per instruction" in limits and "HOST column whole" in limits and "the const table" in limits
    # the call that leases a lane is in the list of calls that run concurrently on one context (it ends at the reference's types)
    assert "kzg_fr_program_run" in hdr[hdr.index("The reference's blocking calls"):hdr.index("run CONCURRENTLY")]


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


def test_python_constants_are_the_headers():
    from kzg_amd import _lib as L
    hdr = text("include", "kzg_mi355x.h")
    for name in ("ADD", "SUB", "MUL", "COL", "CONST", "TEMP", "OUT", "WORDS", "MAX_TEMPS"):
        assert int(re.search(r"\bKZG_FRP_%s = (\d+)" % name, hdr).group(1)) == getattr(L, "FRP_" + name), name


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_cpp_and_rust_name_the_call(name):
    assert re.search(r"\b%s\(" % name, text("include", "kzg_mi355x.hpp"))
    assert re.search(r"pub fn %s\(" % name, text("integration", "mi355x_sys.rs"))


def test_rust_binding_has_the_opaque_type():
    rs = text("integration", "mi355x_sys.rs")
    assert "pub struct kzg_fr_program { _p: [u8; 0] }" in rs and "out: *mut *mut kzg_fr_program" in rs
    assert "cols: *const *const c_void" in rs and "outs: *const *mut c_void" in rs and "pub const KZG_FRP_MAX_TEMPS: c_int = 16;" in rs


def test_cpp_header_has_the_mirrors():
    hpp = text("include", "kzg_mi355x.hpp")
    assert re.search(r"\bclass FrProgram \{", hpp)
    assert "FrProgram(const FrProgram &) = delete;" in hpp and "kzg_fr_program_free(" in hpp      # RAII, like LookupTable
    assert re.search(r"\bfr_program_run\(const FrProgram &plan", hpp)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp_fr_program_test.cpp"))


def test_python_mirrors_exist():
    import kzg_amd
    assert kzg_amd.FrProgram is kzg_amd.api.FrProgram
    for fn in ("run", "shape", "free", "__enter__", "__exit__"):
        assert callable(getattr(kzg_amd.FrProgram, fn))
    assert callable(kzg_amd.Engine.fr_program)
    for fn in ("col", "const", "compile", "insn"):
        assert callable(getattr(kzg_amd.frp, fn))


def test_null_context_is_a_shape_error_that_writes_nothing():
    import kzg_amd
    from kzg_amd import _lib as L
    lib = kzg_amd.load()
    words = (ctypes.c_uint32 * 6)(*kzg_amd.frp.insn(L.FRP_ADD, L.FRP_OUT, 0, L.FRP_COL, 0, L.FRP_COL, 0))
    h = ctypes.c_void_p(0x1234)
    assert lib.kzg_fr_program_setup(None, words, 1, 1, 0, 1, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert h.value == 0x1234
    col, out = ctypes.create_string_buffer(b"\x11" * 32, 32), ctypes.create_string_buffer(b"\xa5" * 32, 32)
    cp, op = (ctypes.c_void_p * 1)(ctypes.addressof(col)), (ctypes.c_void_p * 1)(ctypes.addressof(out))
    cl = (ctypes.c_size_t * 1)(1)
    assert lib.kzg_fr_program_run(None, None, cp, cl, None, 1, L.FR_CANONICAL, 0, op) == L.KZG_ERR_SHAPE
    sizes = (ctypes.c_size_t * 6)(*[77] * 6)
    assert lib.kzg_fr_program_shape(None, *[ctypes.cast(ctypes.byref(sizes, 8 * k), ctypes.POINTER(ctypes.c_size_t)) for k in range(6)]) == L.KZG_ERR_SHAPE
    lib.kzg_fr_program_free(None, None)           # a NULL plan is nothing to free
    assert out.raw == b"\xa5" * 32 and col.raw == b"\x11" * 32 and list(sizes) == [77] * 6


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def test_the_model_on_a_hand_computed_program():
    from tests import fr_program_model as FM
    R = FM.R
    # t0 = col0[i + 1] * col1 (periodic, length 2);  t0 = t0 * t0;  out1 = t0 - const0;  out0 = col0[i - 1] + const1
    words = (FM.insn(FM.MUL, FM.TEMP, 0, FM.COL, 0, FM.COL, 1, 1, 0) + FM.insn(FM.MUL, FM.TEMP, 0, FM.TEMP, 0, FM.TEMP, 0) +
             FM.insn(FM.SUB, FM.OUT, 1, FM.TEMP, 0, FM.CONST, 0) + FM.insn(FM.ADD, FM.OUT, 0, FM.COL, 0, FM.CONST, 1, -1, 0))
    assert FM.validate(words, 2, 2, 2) == (4, 1, 2)
    out = FM.run(words, 2, 2, 2, [[1, 2, 3, R + 4], [10, 20]], [5, R - 1], 4)
    # row i: (col0[i + 1] * col1[i mod 2])^2 - 5;  col0[i - 1] - 1
    assert out[1] == [(2 * 10) ** 2 - 5, (3 * 20) ** 2 - 5, (4 * 10) ** 2 - 5, (1 * 20) ** 2 - 5]
    assert out[0] == [3, 0, 1, 2]
    # a shift of -(2^31) and one of 2^31 - 1 wrap like any other
    words = FM.insn(FM.ADD, FM.OUT, 0, FM.COL, 0, FM.COL, 0, -(1 << 31), (1 << 31) - 1)
    col = [7, 11, 13]
    assert FM.run(words, 1, 0, 1, [col], [], 3)[0] == [col[(i - (1 << 31)) % 3] + col[(i + (1 << 31) - 1) % 3] for i in range(3)]


def test_the_model_rejects_what_the_header_lists():
    from tests import fr_program_model as FM
    for name, words, n_cols, n_consts, n_out in FM.rejected_programs():
        with pytest.raises(FM.ShapeError):
            FM.validate(words, n_cols, n_consts, n_out)
            pytest.fail(name)
    ok = FM.insn(FM.ADD, FM.OUT, 0, FM.COL, 0, FM.CONST, 0)
    for cols, consts, n in (([[1, 2, 3]], [1], 0), ([[1, 2, 3]], [1], 4), ([[1, 2, 3]], [1], 6), ([[]], [1], 4), ([[1, 2, 3]], [FM.R], 3),
                            ([[1, 2, 3]], [1], 999 * 3)):
        with pytest.raises(FM.ShapeError):
            FM.run(ok, 1, 1, 1, cols, consts, n)
    assert FM.run(ok, 1, 1, 1, [[1, 2]], [FM.R - 1], 4) == [[0, 1, 0, 1]]


# ---- the compiler -------------------------------------------------------------------------------------------------------------------
def run_compiled(FM, prog, cols, consts, n):
    assert FM.validate(prog.words, prog.n_cols, prog.n_consts, prog.n_out) == (prog.n_insns, prog.n_temps, prog.n_mul)
    return FM.run(prog.words, prog.n_cols, prog.n_consts, prog.n_out, cols, consts, n)


def test_compiled_standard_gate_agrees_with_direct_evaluation():
    from kzg_amd import frp
    from tests import fr_program_model as FM
    R, rng, n = FM.R, random.Random(71), 12
    a, b, c, ql, qr, qo, qm, qc = (frp.col(k) for k in range(8))
    prog = frp.compile([ql * a + qr * b + qo * c + qm * a * b + qc])
    assert (prog.n_cols, prog.n_consts, prog.n_out, prog.n_mul) == (8, 0, 1, 5) and prog.n_temps <= 2
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(8)]
    A, B, C, QL, QR, QO, QM, QC = cols
    assert run_compiled(FM, prog, cols, [], n) == [[(QL[i] * A[i] + QR[i] * B[i] + QO[i] * C[i] + QM[i] * A[i] * B[i] + QC[i]) % R for i in range(n)]]


def test_compiled_permutation_term_agrees_with_direct_evaluation():
    """z(wX) prod (w_j + beta sigma_j + gamma) - z(X) prod (w_j + beta k_j X + gamma) on an e-fold extended domain, times 1 / Z_H"""
    from kzg_amd import frp
    from tests import fr_program_model as FM
    R, rng, n, e = FM.R, random.Random(72), 16, 4
    w, sig, ident, z, zh_inv = [frp.col(k) for k in range(3)], [frp.col(3 + k) for k in range(3)], frp.col(6), frp.col(7), frp.col(8)
    beta, gamma, ks = frp.const(0), frp.const(1), [frp.const(2 + k) for k in range(3)]
    lhs, rhs = frp.col(7, e), z
    for j in range(3):
        lhs = lhs * (w[j] + beta * sig[j] + gamma)
        rhs = rhs * (w[j] + beta * ks[j] * ident + gamma)
    prog = frp.compile([(lhs - rhs) * zh_inv, lhs])            # the second output is a sub-expression of the first: one more instruction
    assert (prog.n_cols, prog.n_consts, prog.n_out) == (9, 5, 2) and prog.n_mul == 17
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(8)] + [[rng.randrange(R) for _ in range(e)]]
    consts = [rng.randrange(R) for _ in range(5)]
    want = [[], []]
    for i in range(n):
        lv, rv = cols[7][(i + e) % n], cols[7][i]
        for j in range(3):
            lv = lv * (cols[j][i] + consts[0] * cols[3 + j][i] + consts[1]) % R
            rv = rv * (cols[j][i] + consts[0] * consts[2 + j] * cols[6][i] + consts[1]) % R
        want[0].append((lv - rv) * cols[8][i % e] % R)
        want[1].append(lv)
    assert run_compiled(FM, prog, cols, consts, n) == want


def test_a_shared_subexpression_is_emitted_once_and_powers_are_square_and_multiply():
    from kzg_amd import frp
    from tests import fr_program_model as FM
    x, y = frp.col(0), frp.col(1)
    once = frp.compile([(x * y + x) * (y * x + x)])           # x y and y x are one product, the two sums one sum
    assert once.n_mul == 2 and once.n_insns == 3
    assert frp.compile([x * y + x, (x * y) * (x * y)]).n_mul == 2
    p5 = frp.compile([x ** 5])
    assert p5.n_mul == 3 and p5.n_insns == 3
    assert run_compiled(FM, p5, [[2, 3, FM.R - 1]], [], 3) == [[32, 243, FM.R - 1]]
    assert frp.compile([x ** 1 + y]).n_mul == 0 and frp.compile([x ** 16]).n_mul == 4
    with pytest.raises(frp.FrpError):
        x ** 0


def test_sixteen_live_values_compile_and_seventeen_raise():
    from kzg_amd import frp
    from tests import fr_program_model as FM

    def crossed(m, s):    # m values, each used in two different products that lie far apart: all of them are alive at once
        t = [frp.col(k) + frp.const(k) for k in range(m)]
        acc = t[0] * t[s]
        for k in range(1, m):
            acc = acc + t[k] * t[(k + s) % m]
        return acc

    with pytest.raises(frp.FrpError, match=r"more than 16 values are alive at once at \(col\d+ \+ const\d+\)"):
        frp.compile([crossed(17, 8)])
    prog = frp.compile([crossed(15, 7)])                       # the 15 values and the running sum
    assert prog.n_temps == 16 and prog.n_mul == 15
    rng = random.Random(73)
    cols, consts = [[rng.randrange(FM.R) for _ in range(3)] for _ in range(15)], [rng.randrange(FM.R) for _ in range(15)]
    want = [sum((cols[k][i] + consts[k]) * (cols[(k + 7) % 15][i] + consts[(k + 7) % 15]) for k in range(15)) % FM.R for i in range(3)]
    assert run_compiled(FM, prog, cols, consts, 3) == [want]
    # the heavier operand first: a long chain on the right of a product needs no more temporaries than on the left
    chain = frp.col(0)
    for k in range(1, 40):
        chain = chain * frp.col(k % 3) + frp.const(0)
    assert frp.compile([(frp.col(1) * frp.col(2)) * chain]).n_temps == frp.compile([chain * (frp.col(1) * frp.col(2))]).n_temps == 2


def test_the_compiler_refuses_what_is_no_program():
    from kzg_amd import frp
    for bad in ([], [frp.col(0)], [frp.const(1)], [frp.col(0) + frp.col(1)] * 65):
        with pytest.raises(frp.FrpError):
            frp.compile(bad)
    with pytest.raises(TypeError):
        frp.col(0) * 3
    with pytest.raises(frp.FrpError):
        frp.col(-1)
    with pytest.raises(frp.FrpError):
        frp.col(0, 1 << 31)
    # one expression as two outputs is written twice, not moved
    twice = frp.compile([frp.col(0) * frp.col(1)] * 2)
    assert twice.n_out == 2 and twice.n_insns == 2 and twice.n_temps == 0
