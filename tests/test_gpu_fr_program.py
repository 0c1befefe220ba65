"""kzg_fr_program_setup / _run (kzg_amd/csrc/fr_program.hip) on bytes against the Python-integer interpreter of tests/fr_program_model.py.
Every output buffer carries 0xA5 sentinel bytes behind its last element, and they are checked after every call.  Like the FK20 files
this one sorts after the tests that release the session's contexts, so it uses the module-scoped Engine of tests/fk20_common.py."""
import ctypes
import os
import random
import subprocess
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd import frp
from tests import fr_program_model as FM
from tests.fk20_common import MONT_R, dev_buffer, dev_download
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture

pytestmark = pytest.mark.gpu

R = FM.R
CAN, MONT = L.FR_CANONICAL, L.FR_MONT
SH = L.KZG_ERR_SHAPE
PAD = 64
A5 = b"\xa5"
I, ADD, SUB, MUL, COL, CONST, TEMP, OUT = FM.insn, FM.ADD, FM.SUB, FM.MUL, FM.COL, FM.CONST, FM.TEMP, FM.OUT
BLOCKS = (0, 64, 128, 256)
HH, DD, HD, DH = 0, L.IN_DEVICE | L.OUT_DEVICE, L.OUT_DEVICE, L.IN_DEVICE


def enc(vals, sfmt):
    """canonical: the words as they are (a word at or above r stays one); Montgomery: the residue's Montgomery form"""
    if sfmt == MONT:
        return b"".join((v % R * MONT_R % R).to_bytes(32, "little") for v in vals)
    return b"".join(v.to_bytes(32, "little") for v in vals)


def want(outs, sfmt):
    return [enc(o, sfmt) for o in outs]


def option(eng, value):
    assert eng.lib.kzg_ctx_set_option(eng.ctx, b"fr_program_block", value) == 0, eng.last_error()


def setup(eng, prog):
    words, n_cols, n_consts, n_out = prog
    arr = (ctypes.c_uint32 * len(words))(*words)
    h = ctypes.c_void_p()
    assert eng.lib.kzg_fr_program_setup(eng.ctx, arr, len(words) // 6, n_cols, n_consts, n_out, ctypes.byref(h)) == 0, eng.last_error()
    n_insns, n_temps, n_mul = FM.validate(words, n_cols, n_consts, n_out)
    v = [ctypes.c_size_t() for _ in range(6)]
    assert eng.lib.kzg_fr_program_shape(h, *[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [n_insns, n_cols, n_consts, n_out, n_temps, n_mul]
    return h


class Call:
    """the buffers of one kzg_fr_program_run: columns host or device per `flags`, every output behind it 0xA5 sentinels"""

    def __init__(self, eng, n_out, cols, consts, n, sfmt, flags):
        self.eng, self.n, self.flags, self.n_out = eng, n, flags, n_out
        blobs = [enc(c, sfmt) for c in cols]
        self.dev = []
        if flags & L.IN_DEVICE:
            for b in blobs:
                p = ctypes.c_void_p()
                assert eng.lib.kzg_dev_alloc(eng.ctx, max(len(b), 32), ctypes.byref(p)) == 0
                assert eng.lib.kzg_dev_upload(eng.ctx, p, b, len(b)) == 0
                self.dev.append(p)
            self.col_ptrs = [p.value for p in self.dev]
        else:
            self.keep = [ctypes.create_string_buffer(b, len(b)) for b in blobs]
            self.col_ptrs = [ctypes.addressof(b) for b in self.keep]
        self.cp = (ctypes.c_void_p * max(len(cols), 1))(*self.col_ptrs)
        self.cl = (ctypes.c_size_t * max(len(cols), 1))(*[len(c) for c in cols])
        self.kb = enc(consts, sfmt) if consts else None
        if flags & L.OUT_DEVICE:
            self.outs = [dev_buffer(eng, 32 * n + PAD) for _ in range(n_out)]
            self.dev += self.outs
            self.out_ptrs = [p.value for p in self.outs]
        else:
            self.outs = [ctypes.create_string_buffer(A5 * (32 * n + PAD), 32 * n + PAD) for _ in range(n_out)]
            self.out_ptrs = [ctypes.addressof(b) for b in self.outs]
        self.op = (ctypes.c_void_p * n_out)(*self.out_ptrs)

    def run(self, plan, sfmt, n=None):
        return self.eng.lib.kzg_fr_program_run(self.eng.ctx, plan, self.cp, self.cl, self.kb, self.n if n is None else n, sfmt, self.flags, self.op)

    def raw(self):
        if self.flags & L.OUT_DEVICE:
            return [dev_download(self.eng, p, 32 * self.n + PAD) for p in self.outs]
        return [b.raw for b in self.outs]

    def bodies(self):
        """the outputs, after checking that the bytes behind them are untouched"""
        raws = self.raw()
        for r in raws:
            assert r[32 * self.n:] == A5 * PAD, "bytes behind an output were written"
        return [r[:32 * self.n] for r in raws]

    def untouched(self):
        return all(r == A5 * (32 * self.n + PAD) for r in self.raw())

    def free(self):
        for p in self.dev:
            assert self.eng.lib.kzg_dev_free(self.eng.ctx, p) == 0


def run_gpu(eng, plan, n_out, cols, consts, n, sfmt, flags=HH):
    c = Call(eng, n_out, cols, consts, n, sfmt, flags)
    try:
        assert c.run(plan, sfmt) == 0, eng.last_error()
        return c.bodies()
    finally:
        c.free()


def check(eng, prog, cols, consts, n, sfmts=(CAN, MONT), flags=HH, model=None):
    """the program on the GPU against the model, byte for byte; returns the model's outputs"""
    plan = setup(eng, prog)
    try:
        model = model if model is not None else FM.run(prog[0], prog[1], prog[2], prog[3], cols, consts, n)
        for sfmt in sfmts:
            assert run_gpu(eng, plan, prog[3], cols, consts, n, sfmt, flags) == want(model, sfmt), (n, sfmt, flags)
    finally:
        eng.lib.kzg_fr_program_free(eng.ctx, plan)
    return model


def rand_cols(rng, lens):
    return [[rng.randrange(R) for _ in range(ln)] for ln in lens]


# ---- 1. every instruction form ------------------------------------------------------------------------------------------------------
def every_form():
    """every (op, a_kind, b_kind, dst_kind): results to temporaries are read back into outputs of their own"""
    words, out = I(ADD, TEMP, 0, COL, 0, CONST, 0) + I(MUL, TEMP, 1, COL, 1, CONST, 1, -1, 0), 0
    k = 0
    for op in (ADD, SUB, MUL):
        for ak in (COL, CONST, TEMP):
            for bk in (COL, CONST, TEMP):
                a = {COL: k % 3, CONST: k % 2, TEMP: k % 2}[ak]
                b = {COL: (k + 1) % 3, CONST: (k + 1) % 2, TEMP: (k + 1) % 2}[bk]
                sa, sb = (k % 5 - 2 if ak == COL else 0), (3 - k % 7 if bk == COL else 0)
                words += I(op, OUT, out, ak, a, bk, b, sa, sb)
                t = 2 + k % 14
                words += I(op, TEMP, t, ak, a, bk, b, sa, sb) + I(SUB, OUT, out + 1, TEMP, t, COL, 2)
                out += 2
                k += 1
    words += I(MUL, TEMP, 0, TEMP, 0, TEMP, 0) + I(ADD, OUT, out, TEMP, 0, TEMP, 0)      # dst == a == b on one temporary
    return words, 3, 2, out + 1


def test_every_instruction_form(eng):
    rng = random.Random(5100)
    n = 65
    prog = every_form()
    assert prog[3] == 55
    check(eng, prog, rand_cols(rng, [n, n, n]), [rng.randrange(R), rng.randrange(R)], n)
    # no temporaries at all
    check(eng, (I(MUL, OUT, 0, COL, 0, COL, 1, 3, -3), 2, 0, 1), rand_cols(rng, [n, n]), [], n)


# ---- 2. row boundaries ----------------------------------------------------------------------------------------------------------------
def shifts_program(n):
    shifts = [0, 1, -1, n - 1, -(n - 1), n, -n, n + 3, -(n + 3), (1 << 31) - 1, -((1 << 31) - 1)]
    words = []
    for o, s in enumerate(shifts):
        words += I(SUB, OUT, o, COL, 0, COL, 1, s, -s)
    words += I(MUL, TEMP, 0, COL, 0, COL, 1, 1, -1) + I(MUL, OUT, len(shifts), TEMP, 0, COL, 0, 0, -(n + 3))
    return words, 2, 0, len(shifts) + 1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_row_boundaries_and_wrapping_shifts(eng, n):
    rng = random.Random(5200 + n)
    prog, cols = shifts_program(n), rand_cols(rng, [n, n])
    model = None
    try:
        for block in BLOCKS:
            option(eng, block)
            model = check(eng, prog, cols, [], n, sfmts=(MONT,) if block else (CAN, MONT), model=model)
    finally:
        option(eng, 0)


# ---- 3. periodic columns --------------------------------------------------------------------------------------------------------------
def periodic_program(n_per):
    """column 0 is full length, columns 1 .. n_per periodic"""
    words = I(ADD, TEMP, 0, COL, 0, COL, 0, 0, 5)
    for c in range(1, n_per + 1):
        words += I(MUL, TEMP, 0, TEMP, 0, COL, c, 0, 0) + I(ADD, TEMP, 0, TEMP, 0, COL, c, 0, -3) + I(SUB, OUT, c, COL, c, COL, c, 7, -(1 << 31))
    return words + I(ADD, OUT, 0, TEMP, 0, COL, 1, 0, 1), n_per + 1, 0, n_per + 1


def test_periodic_columns(eng):
    rng = random.Random(5300)
    check(eng, periodic_program(3), rand_cols(rng, [1000, 1, 2, 8]), [], 1000)
    check(eng, periodic_program(1), rand_cols(rng, [4096, 4]), [], 4096)
    check(eng, periodic_program(2), rand_cols(rng, [256, 256, 128]), [], 256)      # a power of two: full length and half of it


@pytest.mark.parametrize("n,short", [(1000, 16), (999, 3), (1000, 3), (8, 16)])
def test_a_column_length_that_is_no_period_is_a_shape_error(eng, n, short):
    rng = random.Random(5310)
    prog = periodic_program(1)
    plan = setup(eng, prog)
    for sfmt, flags in ((CAN, HH), (MONT, DD)):
        c = Call(eng, 2, rand_cols(rng, [n, short]), [], n, sfmt, flags)
        assert c.run(plan, sfmt) == SH and c.untouched()
        c.free()
    eng.lib.kzg_fr_program_free(eng.ctx, plan)


# ---- 4. temporaries -----------------------------------------------------------------------------------------------------------------
def sixteen_temps():
    """t_k = col_k + const_k, all sixteen alive at once; out0 = sum_k t_k t_(15 - k), out1 = sum_(k >= 8) t_k const_(k - 8) (no symmetry)"""
    words = []
    for k in range(16):
        words += I(ADD, TEMP, k, COL, k, CONST, k)
    for k in range(8, 16):
        words += I(MUL, OUT, 2 + k - 8, TEMP, k, CONST, k - 8)          # the upper eight, one by one
    for k in range(8):
        words += I(MUL, TEMP, k, TEMP, k, TEMP, 15 - k)
    for k in range(8, 16):
        words += I(MUL, TEMP, k, TEMP, k, CONST, k - 8)
    for k in range(1, 8):
        words += I(ADD, TEMP, 0, TEMP, 0, TEMP, k)
    for k in range(9, 16):
        words += I(ADD, TEMP, 8, TEMP, 8, TEMP, k)
    return words + I(ADD, OUT, 0, TEMP, 0, TEMP, 0) + I(ADD, OUT, 1, TEMP, 8, TEMP, 8, 0, 0), 16, 16, 10


def five_temps():
    words = []
    for k in range(5):
        words += I(ADD, TEMP, k, COL, k, CONST, k)
    words += I(MUL, TEMP, 0, TEMP, 0, TEMP, 1) + I(MUL, TEMP, 2, TEMP, 2, TEMP, 3) + I(SUB, TEMP, 0, TEMP, 0, TEMP, 2)
    return words + I(MUL, OUT, 0, TEMP, 0, TEMP, 4), 5, 5, 1


@pytest.mark.parametrize("name", ["sixteen", "five", "one"])
def test_temporaries_keep_their_slots(eng, name):
    rng = random.Random(5400)
    n = 257
    prog = {"sixteen": sixteen_temps(), "five": five_temps(), "one": (I(MUL, TEMP, 0, COL, 0, COL, 1) + I(SUB, OUT, 0, TEMP, 0, COL, 2), 3, 0, 1)}[name]
    cols, consts = rand_cols(rng, [n] * prog[1]), [rng.randrange(R) for _ in range(prog[2])]
    model = FM.run(prog[0], prog[1], prog[2], prog[3], cols, consts, n)
    if name == "sixteen":
        t = [[(cols[k][i] + consts[k]) % R for i in range(n)] for k in range(16)]
        assert model[0] == [sum(t[k][i] * t[15 - k][i] for k in range(16)) % R for i in range(n)]
    try:
        for block in BLOCKS:
            option(eng, block)
            check(eng, prog, cols, consts, n, sfmts=(MONT, CAN) if block in (0, 256) else (MONT,), model=model)
    finally:
        option(eng, 0)


# ---- 5. values ------------------------------------------------------------------------------------------------------------------------
VALUES_PROGRAM = (I(MUL, OUT, 0, COL, 0, COL, 1) + I(ADD, OUT, 1, COL, 0, COL, 1) + I(SUB, OUT, 2, COL, 0, COL, 1) + I(MUL, OUT, 3, COL, 0, CONST, 2) +
                  I(SUB, OUT, 4, CONST, 0, COL, 1) + I(ADD, OUT, 5, CONST, 2, COL, 0) + I(MUL, OUT, 6, CONST, 2, CONST, 2) + I(ADD, OUT, 7, CONST, 1, CONST, 2) +
                  I(MUL, TEMP, 0, COL, 0, CONST, 1) + I(SUB, OUT, 8, TEMP, 0, CONST, 1), 2, 3, 9)


def test_values_at_the_edges(eng):
    for sfmt, vals in ((MONT, [0, 1, R - 1]), (CAN, [0, 1, R - 1, R, R + 1, (1 << 256) - 1])):
        m = len(vals)
        cols = [[vals[i // m] for i in range(m * m)], [vals[i % m] for i in range(m * m)]]      # every pair of values
        check(eng, VALUES_PROGRAM, cols, [0, 1, R - 1], m * m, sfmts=(sfmt,))


def test_a_const_equal_to_r_is_a_shape_error(eng):
    plan = setup(eng, VALUES_PROGRAM)
    for sfmt in (CAN, MONT):
        for flags in (HH, DD):
            c = Call(eng, 9, [[1, 2], [3, 4]], [0, 1, 2], 2, sfmt, flags)
            c.kb = enc([0, 1], sfmt) + R.to_bytes(32, "little")
            assert c.run(plan, sfmt) == SH and c.untouched()
            c.kb = enc([0, 1], sfmt) + b"\xff" * 32
            assert c.run(plan, sfmt) == SH and c.untouched()
            c.free()
    eng.lib.kzg_fr_program_free(eng.ctx, plan)


# ---- 6. long and random programs ------------------------------------------------------------------------------------------------------
def test_a_chain_of_4096_instructions(eng):
    rng = random.Random(5600)
    n = 64
    words = I(ADD, TEMP, 0, COL, 0, CONST, 0)
    for k in range(2047):
        words += I(MUL, TEMP, 0, TEMP, 0, COL, k % 3, 0, k % 5 - 2) + I(ADD, TEMP, 0, TEMP, 0, CONST, k % 2)
    words += I(ADD, OUT, 0, TEMP, 0, COL, 1)
    assert len(words) == 6 * 4096
    check(eng, (words, 3, 2, 1), rand_cols(rng, [n, n, 2]), [rng.randrange(R), rng.randrange(R)], n)


def random_program(rng, n_cols, n_consts, n_out, max_insns=64):
    count = rng.randrange(n_out, max_insns + 1)
    out_at = dict(zip(rng.sample(range(count), n_out), range(n_out)))
    written, words = [], []
    for k in range(count):
        ops = []
        for _ in range(2):
            kind = rng.choice([COL, COL, CONST, TEMP] if written else [COL, COL, CONST])
            if kind == COL:
                ops.append((COL, rng.randrange(n_cols), rng.choice([0, 0, 1, -1, 2, -5, 256, 257, -258, 1 << 20, -(1 << 31)])))
            elif kind == CONST:
                ops.append((CONST, rng.randrange(n_consts), 0))
            else:
                ops.append((TEMP, rng.choice(written), 0))
        (ak, a, sa), (bk, b, sb) = ops
        if k in out_at:
            words += I(rng.randrange(3), OUT, out_at[k], ak, a, bk, b, sa, sb)
        else:
            t = rng.randrange(16)
            words += I(rng.randrange(3), TEMP, t, ak, a, bk, b, sa, sb)
            if t not in written:
                written.append(t)
    return words, n_cols, n_consts, n_out


def test_sixty_random_programs(eng):
    n = 257
    for seed in range(60):
        rng = random.Random(5700 + seed)
        prog = random_program(rng, 6, 3, 3)
        cols = rand_cols(rng, [n, n, 1, n, 1, n])
        check(eng, prog, cols, [rng.randrange(R) for _ in range(3)], n, sfmts=(MONT if seed % 2 else CAN,), flags=DD if seed % 3 == 0 else HH)


def test_random_programs_over_periodic_columns(eng):
    """n = 257 is prime and leaves only the period 1: the same generator at n = 256 with periods 2 and 8 beside full-length columns"""
    n = 256
    for seed in range(12):
        rng = random.Random(5800 + seed)
        prog = random_program(rng, 6, 3, 3)
        cols = rand_cols(rng, [n, 2, 8, n, 1, 128])
        check(eng, prog, cols, [rng.randrange(R) for _ in range(3)], n, sfmts=(MONT if seed % 2 else CAN,), flags=DD if seed % 3 == 0 else HH)


# ---- 7. residence ---------------------------------------------------------------------------------------------------------------------
TWO_OUT = (I(MUL, TEMP, 0, COL, 0, COL, 1, 1, 0) + I(ADD, OUT, 1, TEMP, 0, CONST, 0) + I(SUB, OUT, 0, TEMP, 0, COL, 2, 0, -1), 3, 1, 2)


@pytest.mark.parametrize("flags", [HH, DD, HD, DH])
def test_residence(eng, flags):
    rng = random.Random(5800)
    n = 1000
    check(eng, TWO_OUT, rand_cols(rng, [n, 8, n]), [rng.randrange(R)], n, flags=flags)


@pytest.mark.parametrize("flags", [HH, DD])
def test_an_output_that_is_a_column_or_another_output_is_rejected(eng, flags):
    rng = random.Random(5810)
    n = 64
    plan = setup(eng, TWO_OUT)
    cols = rand_cols(rng, [n, n, n])
    c = Call(eng, 2, cols, [5], n, CAN, flags)
    first = c.out_ptrs[0]
    for bad in ((c.col_ptrs[2], c.out_ptrs[1]), (c.out_ptrs[0], c.col_ptrs[0]), (c.out_ptrs[1], c.out_ptrs[1])):
        c.op[0], c.op[1] = bad
        assert c.run(plan, CAN) == SH, bad
        assert c.untouched()
        if flags == DD:
            assert [dev_download(eng, p, 32 * n) for p in c.dev[:3]] == [enc(col, CAN) for col in cols]
        else:
            assert [b.raw for b in c.keep] == [enc(col, CAN) for col in cols]
    c.op[0], c.op[1] = first, c.out_ptrs[1]
    assert c.run(plan, CAN) == 0 and c.bodies() == want(FM.run(TWO_OUT[0], 3, 1, 2, cols, [5], n), CAN)
    c.free()
    eng.lib.kzg_fr_program_free(eng.ctx, plan)


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_every_setup_error_leaves_out_as_it_was(eng):
    lib = eng.lib
    for name, words, n_cols, n_consts, n_out in FM.rejected_programs():
        arr = (ctypes.c_uint32 * max(len(words), 6))(*words)
        h = ctypes.c_void_p(0x1234)
        assert lib.kzg_fr_program_setup(eng.ctx, arr, len(words) // 6, n_cols, n_consts, n_out, ctypes.byref(h)) == SH, name
        assert h.value == 0x1234, name
    arr = (ctypes.c_uint32 * 6)(*I(ADD, OUT, 0, COL, 0, COL, 0))
    h = ctypes.c_void_p(0x1234)
    assert lib.kzg_fr_program_setup(eng.ctx, None, 1, 1, 0, 1, ctypes.byref(h)) == SH and h.value == 0x1234
    assert lib.kzg_fr_program_setup(eng.ctx, arr, 1, 1, 0, 1, None) == SH
    assert lib.kzg_fr_program_setup(eng.ctx, arr, 1, 1, 0, 1, ctypes.byref(h)) == 0 and h.value != 0x1234
    lib.kzg_fr_program_free(eng.ctx, h)


@pytest.mark.parametrize("flags", [HH, DD])
def test_every_run_error_writes_nothing(eng, flags):
    n = 8
    plan = setup(eng, TWO_OUT)
    cols = [[1] * n, [2] * n, [3] * n]
    c = Call(eng, 2, cols, [5], n, CAN, flags)
    lib, ctx = eng.lib, eng.ctx

    def refused(rc):
        assert rc == SH and c.untouched()

    # (the header's "plan of another GPU" needs a second device: the one context of this suite cannot reach it)
    refused(lib.kzg_fr_program_run(ctx, None, c.cp, c.cl, c.kb, n, CAN, flags, c.op))                  # a NULL plan
    refused(c.run(plan, CAN, n=0))
    refused(c.run(plan, CAN, n=(1 << 28) + 1))
    refused(c.run(plan, CAN, n=1 << 29))                                                               # (8 divides it: n itself is refused)
    refused(c.run(plan, 2))                                                                            # an unknown sfmt
    refused(c.run(plan, -1))
    refused(lib.kzg_fr_program_run(ctx, plan, None, c.cl, c.kb, n, CAN, flags, c.op))                  # the arrays themselves
    refused(lib.kzg_fr_program_run(ctx, plan, c.cp, None, c.kb, n, CAN, flags, c.op))
    refused(lib.kzg_fr_program_run(ctx, plan, c.cp, c.cl, None, n, CAN, flags, c.op))
    refused(lib.kzg_fr_program_run(ctx, plan, c.cp, c.cl, c.kb, n, CAN, flags, None))
    for bad in (0, 3, 16, 6):                                                                          # 0; no power of two; does not divide; neither
        c.cl[1] = bad
        refused(c.run(plan, CAN))
    c.cl[1] = n
    keep = c.cp[2]
    c.cp[2] = None
    refused(c.run(plan, CAN))                                                                          # a NULL column
    c.cp[2] = keep
    keep = c.op[1]
    c.op[1] = None
    refused(c.run(plan, CAN))                                                                          # a NULL output
    c.op[1] = keep
    assert c.run(plan, CAN) == 0 and c.bodies() == want(FM.run(TWO_OUT[0], 3, 1, 2, cols, [5], n), CAN)
    c.free()
    eng.lib.kzg_fr_program_free(eng.ctx, plan)


# ---- 9. concurrency -------------------------------------------------------------------------------------------------------------------
def test_two_threads_run_different_plans_on_one_context(eng):
    rng = random.Random(5900)
    n = 4097
    jobs = []
    for prog, lens, flags, sfmt in ((five_temps(), [n] * 5, DD, MONT), (TWO_OUT, [n, 1, n], HH, CAN)):
        cols, consts = rand_cols(rng, lens), [rng.randrange(R) for _ in range(prog[2])]
        jobs.append((setup(eng, prog), prog, cols, consts, flags, sfmt, want(FM.run(prog[0], prog[1], prog[2], prog[3], cols, consts, n), sfmt)))
    errors = []

    def worker(job):
        plan, prog, cols, consts, flags, sfmt, expect = job
        try:
            for _ in range(20):
                got = run_gpu(eng, plan, prog[3], cols, consts, n, sfmt, flags)
                if got != expect:
                    errors.append("wrong bytes")
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for j in jobs:
        eng.lib.kzg_fr_program_free(eng.ctx, j[0])
    assert not errors, errors[:3]


# ---- 10. the quotient round -----------------------------------------------------------------------------------------------------------
def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def poly_add(a, b, sign=1):
    m = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + sign * (b[i] if i < len(b) else 0)) % R for i in range(m)]


def test_the_quotient_round_end_to_end(eng):
    """d = 8 rows on an e = 4-fold extended coset: the standard gate and a one-wire copy constraint through kzg_fr_grand_product's z
    column and a rotation by e, times the periodic 1 / Z_H, all in one compiled program between the coset transforms"""
    rng = random.Random(6000)
    d, e, log_d, log_n = 8, 4, 3, 5
    n = d * e
    root = pow(7, (R - 1) >> 32, R)
    w_d, w_n = pow(root, 1 << (32 - log_d), R), pow(root, 1 << (32 - log_n), R)
    alpha, beta, gamma = (rng.randrange(1, R) for _ in range(3))
    sigma_of = list(range(d))
    sigma_of[2], sigma_of[5] = 5, 2                                  # the copy constraint: a_2 = a_5

    def quotient(tamper):
        a, b = [rng.randrange(R) for _ in range(d)], [rng.randrange(R) for _ in range(d)]
        a[5] = a[2]
        ql, qr, qm, qc = ([rng.randrange(R) for _ in range(d)] for _ in range(4))
        qo = [R - 1] * d
        c = [(ql[i] * a[i] + qr[i] * b[i] + qm[i] * a[i] * b[i] + qc[i]) % R for i in range(d)]
        ident, sigma = [pow(w_d, i, R) for i in range(d)], [pow(w_d, sigma_of[i], R) for i in range(d)]
        num = [(a[i] + beta * ident[i] + gamma) % R for i in range(d)]
        den = [(a[i] + beta * sigma[i] + gamma) % R for i in range(d)]
        z, totals, zero_den = eng.grand_product(num, den, d, 1)
        assert totals == [1] and zero_den == [0] and z[0] == 1
        if tamper:
            c[3] = (c[3] + 1) % R
        evals = [a, b, c, ql, qr, qo, qm, qc, sigma, ident, z]
        coeffs = [eng.ntt(v, log_d, inverse=True) for v in evals]
        on_coset = [eng.coset_ntt(p + [0] * (n - d), log_n) for p in coeffs]
        zh_inv = [pow((pow(7, d, R) * pow(w_n, d * i, R) - 1) % R, -1, R) for i in range(e)]
        A, B, C, QL, QR, QO, QM, QC, S, ID, Z = (frp.col(k) for k in range(11))
        al, be, ga = frp.const(0), frp.const(1), frp.const(2)
        gate = QL * A + QR * B + QO * C + QM * A * B + QC
        perm = frp.col(10, e) * (A + be * S + ga) - Z * (A + be * ID + ga)
        prog = frp.compile([(gate + al * perm) * frp.col(11)])
        cols, consts = on_coset + [zh_inv], [alpha, beta, gamma]
        model = FM.run(prog.words, prog.n_cols, prog.n_consts, prog.n_out, cols, consts, n)
        with eng.fr_program(prog) as plan:
            assert plan.shape() == (prog.n_insns, 12, 3, 1, prog.n_temps, prog.n_mul)
            bufs = [eng.alloc_scalars(len(col)).upload(kzg_amd.pack_scalars(col)) for col in cols]
            out = eng.alloc_scalars(n)
            plan.run(bufs, consts, n=n, outs=[out])
            got = kzg_amd.unpack_scalars(out.download())
            for buf in bufs + [out]:
                buf.free()
            assert got == plan.run(cols, consts)[0] == model[0]
        t = eng.coset_ntt(got, log_n, inverse=True)
        # the same quotient by polynomial arithmetic on the coefficients
        pa, pb, pc, pql, pqr, pqo, pqm, pqc, ps, pid, pz = coeffs
        g = poly_add(poly_add(poly_add(poly_mul(pql, pa), poly_mul(pqr, pb)), poly_add(poly_mul(pqo, pc), poly_mul(pqm, poly_mul(pa, pb)))), pqc)
        z_next = [pz[k] * pow(w_d, k, R) % R for k in range(d)]                       # z(w X)
        lin = lambda p: poly_add(poly_add(pa, [beta * x % R for x in p]), [gamma])  # noqa: E731
        pp = poly_add(poly_mul(z_next, lin(ps)), poly_mul(pz, lin(pid)), -1)
        numer = poly_add(g, [alpha * x % R for x in pp])
        return t, numer

    t, numer = quotient(False)
    numer += [0] * (n + d - len(numer))
    q = [0] * n
    rem = list(numer)
    for k in range(len(rem) - 1, d - 1, -1):                                          # division by X^d - 1
        q[k - d] = rem[k]
        rem[k - d] = (rem[k - d] + rem[k]) % R
        rem[k] = 0
    assert not any(rem), "the witness does not satisfy the constraints"
    assert t == q
    bound = 3 * (d - 1) - d + 1
    assert not any(t[bound:]) and any(t[:bound])
    t_bad, _ = quotient(True)
    assert any(t_bad[bound:])


# ---- 11. the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_wrapper(tmp_path):
    """FrProgram and fr_program_run of include/kzg_mi355x.hpp: tests/cpp_fr_program_test.cpp against the shared library"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_fr_program_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp_fr_program_test.cpp"), "-L" + os.path.join(root, "kzg_amd"),
                           "-lkzg_mi355x", "-Wl,-rpath," + os.path.join(root, "kzg_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
