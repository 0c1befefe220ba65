"""kzg_sumcheck_round and kzg_fr_program_degree (kzg_amd/csrc/mle.hip) on bytes against the Python-integer model of tests/mle_model.py, and
kzg_amd.sumcheck.prove end to end against the model verifier.  sums_out has 0xA5 sentinel bytes behind it, checked after every call.
Like the FK20 files this one sorts after the tests that release the session's contexts, so it uses the module-scoped Engine of
tests/fk20_common.py."""
import ctypes
import hashlib
import random
import threading

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd import frp
from tests import fr_program_model as FM
from tests import mle_model as MM
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture
from tests.mle_gpu_common import CAN, MONT, SH, Buf, Options, data, enc, ptrs

pytestmark = pytest.mark.gpu

R = MM.R
I, ADD, SUB, MUL, COL, CONST, TEMP, OUT = FM.insn, FM.ADD, FM.SUB, FM.MUL, FM.COL, FM.CONST, FM.TEMP, FM.OUT


def setup(eng, prog):
    words, n_cols, n_consts, n_out = prog
    arr = (ctypes.c_uint32 * len(words))(*words)
    h = ctypes.c_void_p()
    assert eng.lib.kzg_fr_program_setup(eng.ctx, arr, len(words) // 6, n_cols, n_consts, n_out, ctypes.byref(h)) == 0, eng.last_error()
    d = (ctypes.c_size_t * n_out)()
    assert eng.lib.kzg_fr_program_degree(h, d) == 0 and list(d) == MM.degrees(*prog)
    return h


class Round:
    """the buffers of one kzg_sumcheck_round"""

    def __init__(self, eng, prog, cols, consts, n_eval, sfmt, dev):
        self.eng, self.n, self.n_eval, self.sfmt, self.dev = eng, len(cols[0]), n_eval, sfmt, dev
        self.cols = [Buf(eng, 32 * len(c), dev, enc(c, sfmt)) for c in cols]
        self.cp = ptrs(self.cols)
        self.kb = enc(consts, sfmt) if consts else None
        self.sums = Buf(eng, 32 * max(prog[3] * n_eval, 1), False)

    def run(self, plan, **kw):
        a = dict(cp=self.cp, kb=self.kb, n=self.n, n_eval=self.n_eval, sfmt=self.sfmt, sums=self.sums.addr)
        a.update(kw)
        return self.eng.lib.kzg_sumcheck_round(self.eng.ctx, plan, a["cp"], a["kb"], a["n"], a["n_eval"], a["sfmt"], L.IN_DEVICE if self.dev else 0, a["sums"])

    def free(self):
        for b in self.cols + [self.sums]:
            b.free()


def round_gpu(eng, plan, prog, cols, consts, n_eval, sfmt, dev):
    r = Round(eng, prog, cols, consts, n_eval, sfmt, dev)
    try:
        assert r.run(plan) == 0, eng.last_error()
        assert all(c.untouched() for c in r.cols), "the columns were written"
        return r.sums.body()
    finally:
        r.free()


def want(sums, sfmt):
    return enc([v for s in sums for v in s], sfmt)


def check(eng, prog, n, n_eval, seed, combos=((CAN, False), (MONT, True)), consts=None):
    """the round on the GPU against the model, byte for byte, per (format, residence); returns (columns, model) of the last combination"""
    rng = random.Random(seed)
    plan = setup(eng, prog)
    consts = [rng.randrange(R) for _ in range(prog[2])] if consts is None else consts
    try:
        for sfmt, dev in combos:
            cols = [data(rng, n, sfmt) for _ in range(prog[1])]
            model = MM.round_sums(*prog, cols, consts, n_eval)
            assert round_gpu(eng, plan, prog, cols, consts, n_eval, sfmt, dev) == want(model, sfmt), (n, n_eval, sfmt, dev)
    finally:
        eng.lib.kzg_fr_program_free(eng.ctx, plan)
    return cols, model


def two_degrees_program():
    """out0 = col0 col1 col2 - const0 (degree 3), out1 = col0 + const1 (degree 1), out2 = const0 const1 (degree 0)"""
    return (I(MUL, TEMP, 0, COL, 0, COL, 1) + I(MUL, TEMP, 0, TEMP, 0, COL, 2) + I(SUB, OUT, 0, TEMP, 0, CONST, 0) + I(ADD, OUT, 1, COL, 0, CONST, 1) +
            I(MUL, OUT, 2, CONST, 0, CONST, 1)), 3, 2, 3


def const_program():
    """out0 = const0 + const1: degree 0, the sum is h times it (the second instruction only gives the plan its column)"""
    return I(ADD, OUT, 0, CONST, 0, CONST, 1) + I(SUB, TEMP, 0, COL, 0, COL, 0), 1, 2, 1


def sixteen_temps_program():
    """the sixteen-live-values program of tests/test_fr_program_abi.py"""
    t = [frp.col(k) + frp.const(k) for k in range(15)]
    acc = t[0] * t[7]
    for k in range(1, 15):
        acc = acc + t[k] * t[(k + 7) % 15]
    p = frp.compile([acc])
    assert p.n_temps == 16
    return list(p.words), p.n_cols, p.n_consts, p.n_out


PROGRAMS = {"product": MM.product_program, "eq_gate": MM.eq_gate_program, "two_degrees": two_degrees_program, "const": const_program,
            "sixteen_temps": sixteen_temps_program}


# ---- 1. programs and points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_eval", [("product", 3), ("product", 1), ("product", 2), ("product", 16), ("eq_gate", 5), ("two_degrees", 5),
                                         ("two_degrees", 4), ("const", 2), ("const", 5), ("sixteen_temps", 3), ("sixteen_temps", 16)])
def test_programs_and_points(eng, name, n_eval):
    prog = PROGRAMS[name]()
    check(eng, prog, 256, n_eval, 9100 + n_eval)


def test_the_constant_output_sums_to_h_times_the_constant(eng):
    prog = const_program()
    cols, model = check(eng, prog, 64, 2, 9150, consts=[3, 4])
    assert model == [[32 * 7, 32 * 7]]


def test_thirty_two_accumulators_are_accepted_and_thirty_three_refused(eng):
    two = I(MUL, OUT, 0, COL, 0, COL, 1) + I(SUB, OUT, 1, COL, 0, COL, 1)
    check(eng, (two, 2, 0, 2), 128, 16, 9200)
    three = two + I(ADD, OUT, 2, COL, 0, COL, 1)
    prog = (three, 2, 0, 3)
    plan = setup(eng, prog)
    r = Round(eng, prog, [[1] * 8, [2] * 8], [], 11, CAN, False)
    assert r.run(plan) == SH and r.sums.untouched()
    assert r.run(plan, n_eval=10) == 0 and r.sums.body()[:32 * 30] == want(MM.round_sums(*prog, [[1] * 8, [2] * 8], [], 10), CAN)
    r.free()
    eng.lib.kzg_fr_program_free(eng.ctx, plan)


# ---- 2. pair counts, workgroup sizes, grids -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 2, 32, 64, 128, 512])
def test_pair_counts_and_workgroup_sizes(eng, h):
    """fewer pairs than a wave (dead lanes add nothing), exactly one wave, and h = 128 as two waves of one workgroup, two workgroups of
    one wave, or half a workgroup"""
    for block in (0, 64, 128, 256):
        with Options(eng, sumcheck_block=block):
            check(eng, MM.eq_gate_program(), 2 * h, 5, 9300 + h, combos=((MONT, True),) if block else ((CAN, False), (MONT, True), (CAN, True)))
            check(eng, two_degrees_program(), 2 * h, 4, 9350 + h, combos=((MONT, False),))


@pytest.mark.parametrize("grid,h", [(1, 512), (3, 512), (1, 64), (2, 4096)])
def test_bounded_grids_stride_over_the_pairs(eng, grid, h):
    """one workgroup of 64 walks 8 strides; three walk 3, 3 and 2: an uneven last stride"""
    with Options(eng, sumcheck_block=64, sumcheck_grid=grid):
        check(eng, MM.eq_gate_program(), 2 * h, 5, 9400 + grid)
        check(eng, sixteen_temps_program(), 2 * h, 3, 9450 + grid, combos=((MONT, True),))


# ---- 3. against the existing call ---------------------------------------------------------------------------------------------------------
def test_s0_plus_s1_is_the_sum_of_fr_program_run_over_all_rows(eng):
    rng = random.Random(9500)
    n = 1 << 10
    prog = MM.eq_gate_program()
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(9)]
    with eng.fr_program(prog[0], prog[1], prog[2], prog[3]) as plan:
        assert plan.degrees() == [4]
        rows = plan.run(cols, [], n=n)[0]
        s = plan.sumcheck_round(cols, [])
        assert len(s) == 1 and len(s[0]) == 5 and s == eng.sumcheck_round(plan, cols, [], 5)
        assert (s[0][0] + s[0][1]) % R == sum(rows) % R
        assert s[0][0] == sum(rows[:n // 2]) % R and s[0][1] == sum(rows[n // 2:]) % R


# ---- 4. concurrency -------------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_the_single_thread_bytes(eng):
    rng = random.Random(9600)
    jobs = []
    for prog, n, n_eval, sfmt, dev in ((MM.eq_gate_program(), 2048, 5, MONT, True), (two_degrees_program(), 1024, 4, CAN, False)):
        cols = [data(rng, n, sfmt) for _ in range(prog[1])]
        consts = [rng.randrange(R) for _ in range(prog[2])]
        plan = setup(eng, prog)
        jobs.append((plan, prog, cols, consts, n_eval, sfmt, dev, round_gpu(eng, plan, prog, cols, consts, n_eval, sfmt, dev)))
    assert jobs[0][-1] == want(MM.round_sums(*jobs[0][1], jobs[0][2], jobs[0][3], 5), MONT)
    errors = []

    def worker(job):
        plan, prog, cols, consts, n_eval, sfmt, dev, single = job
        try:
            for _ in range(10):
                if round_gpu(eng, plan, prog, cols, consts, n_eval, sfmt, dev) != single:
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


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True])
def test_every_refusal_leaves_the_sums_untouched(eng, dev):
    prog = two_degrees_program()
    plan = setup(eng, prog)
    shifted = setup(eng, (I(MUL, OUT, 0, COL, 0, COL, 1, 0, 1), 2, 0, 1))
    n = 8
    r = Round(eng, prog, [[1] * n, [2] * n, [3] * n], [5, 6], 4, CAN, dev)
    lib, ctx = eng.lib, eng.ctx

    def refused(rc):
        assert rc == SH and r.sums.untouched() and all(c.untouched() for c in r.cols)

    # (the header's "plan of another GPU" needs a second device: the one context of this suite cannot reach it)
    refused(r.run(shifted))                                            # a rotation
    refused(r.run(None))
    for bad in (0, 17, 11, 1 << 40):                                   # 3 x 11 = 33 accumulators
        refused(r.run(plan, n_eval=bad))
    for bad in (0, 1, 6, 12, (1 << 28) + 1, 1 << 29):
        refused(r.run(plan, n=bad))
    refused(r.run(plan, kb=enc([5, R], CAN)))                          # a const not below r
    refused(r.run(plan, kb=enc([(1 << 256) - 1, 0], CAN), sfmt=MONT))
    refused(r.run(plan, kb=None))
    refused(r.run(plan, cp=None))
    refused(r.run(plan, sums=None))
    refused(r.run(plan, cp=ptrs([r.cols[0], None, r.cols[2]])))
    refused(r.run(plan, sfmt=2))
    refused(r.run(plan, sfmt=-1))
    d = (ctypes.c_size_t * 3)(7, 7, 7)
    assert lib.kzg_fr_program_degree(None, d) == SH and lib.kzg_fr_program_degree(plan, None) == SH and list(d) == [7, 7, 7]
    assert r.run(plan) == 0 and r.sums.body() == want(MM.round_sums(*prog, [[1] * n, [2] * n, [3] * n], [5, 6], 4), CAN)
    r.free()
    eng.lib.kzg_fr_program_free(ctx, plan)
    eng.lib.kzg_fr_program_free(ctx, shifted)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def fiat_shamir(k, sums):
    h = hashlib.sha256(b"sumcheck round %d" % k)
    for s in sums:
        for v in s:
            h.update(v.to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "little") % R


@pytest.mark.parametrize("on_device", [True, False])
def test_prove_on_the_gpu_is_accepted_by_the_model_verifier(eng, on_device):
    rng = random.Random(9700)
    m = 10
    n = 1 << m
    prog = MM.eq_gate_program()
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(8)] + [MM.eq([rng.randrange(R) for _ in range(m)])]
    claim = [sum(FM.run(*prog, cols, [], n)[0]) % R]
    ev = lambda v: [MM.eq_gate_value(v)]  # noqa: E731

    def prove(columns):
        with eng.fr_program(prog[0], prog[1], prog[2], prog[3]) as plan:
            if not on_device:
                return kzg_amd.sumcheck.prove(eng, plan, columns, [], fiat_shamir)
            bufs = [eng.alloc_scalars(n, L.FR_MONT).upload(enc(c, MONT)) for c in columns]
            try:
                return kzg_amd.sumcheck.prove(eng, plan, bufs, [], fiat_shamir)
            finally:
                for b in bufs:
                    b.free()

    rounds, point, finals = prove(cols)
    assert len(rounds) == m and all(len(s) == 1 and len(s[0]) == 5 for s in rounds)
    assert point == [fiat_shamir(k, rounds[k]) for k in range(m)][::-1]
    assert MM.verify(claim, rounds, point, finals, ev) and kzg_amd.sumcheck.verify(claim, rounds, point, finals, ev)
    # the columns' final values are their multilinear extensions at the point
    assert finals == eng.mle_eval([v for c in cols for v in c], point, batch=9)
    assert rounds[0] == MM.round_sums(*prog, cols, [], 5)
    # one element flipped, the old claim kept
    cols[1][777] ^= 1
    rounds2, point2, finals2 = prove(cols)
    assert not MM.verify(claim, rounds2, point2, finals2, ev)
    assert not MM.verify(claim, rounds, point, finals2, ev)
