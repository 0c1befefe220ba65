"""include/kzg_mi355x.h, Conventions: "scalars in KZG_FR_CANONICAL_LE_32 that are >= r are taken mod r (single host scalars such
as x, y, tau must be < r: KZG_ERR_SHAPE)".  Both halves of that rule, call by call.

First half.  For every call below a base input V (every value < r) gives the expected bytes E through the oracle (oracle/c_oracle.py,
oracle/kzg_model.py, or the model of the call's own test file); the oracle only ever sees V.  Then call(V) == E and, for the three
modes of tests/residue_lift.py ("all", "sparse", "edges": other 256-bit representatives of the same residues, among them the words
r, 2r, r + 1, 2r + 1, 2r - 1 and 2^256 - 1), call(lift(V, mode)) == E byte for byte, with the input in host memory and, where the
call takes KZG_IN_DEVICE, resident in HBM (the staging paths differ).  Byte equality also says that every canonical output is < r.
Calls that other files already feed such values (kzg_msm_g1 at widths 0 and 17 and the NAF tables, kzg_poly_multi_eval,
kzg_interpolate, kzg_fr_fold, kzg_fr_lincomb, the open_fold calls off the domain, the multiopen calls, kzg_poly_divide) are not
repeated.  The extra level of kzg_ntt_fr above 2^24 is in tests/test_gpu_ntt_large.py::test_ntt_above_2_24.

Second half.  test_host_scalar_out_of_range_*: a single host scalar of r or 2^256 - 1 is KZG_ERR_SHAPE, no output buffer is
touched, and the context still gives E afterwards.

KZG_FR_MONT_LE_32 is out of this contract: a Montgomery word is a * 2^256 mod r by definition, hence < r; no lifted Montgomery
words are fed here.

Like the FK20 files this one sorts after the tests that release the session's contexts (tests/conftest.py ORDER), so it opens and
closes a module-scoped Engine of its own (tests/fk20_common.py) instead of the session's `engine`."""
import ctypes
import itertools
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import open_eval_model as OM
from tests import residue_lift as RL
from tests.fk20_common import eng  # noqa: F401 -- this module's fixture
# the base inputs, oracle expectations and fixtures shared with tests/test_gpu_scalar_formats.py
from tests.scalar_call_cases import (AFF, CAN, D, M_INDICES, M_ON, NC, NM, R, TAU, Z_OFF, g1, le, ok, omega, quotient_on_domain,  # noqa: F401
                                     witness_at, evals, group, kit, poly)
from tests.scalar_call_cases import coset_scale as _coset_scale, group_call as _group_call, vec_pair as _vec_pair
from tests.scalar_call_cases import FK_LOG_L, FK_LOG_N, fk20_cosets_expect as _fk20_cosets_expect, fk20_points_expect as _fk20_points_expect

pytestmark = pytest.mark.gpu

MODES = RL.MODES
SENTINEL = b"\xa5"
BAD_SCALARS = (R, (1 << 256) - 1)


class Buf:
    """`data` where a call wants it: a host buffer, or (dev) an allocation in HBM; read() gives back what is there now"""

    def __init__(self, e, data, dev):
        self.e, self.dev = e, dev
        if dev:
            self.d = e.alloc_scalars(len(data) // 32).upload(data)
            self.ptr, self.flags = self.d.ptr, L.IN_DEVICE
        else:
            self.ptr, self.flags = ctypes.create_string_buffer(data, len(data)), 0

    def read(self):
        return self.d.download() if self.dev else self.ptr.raw

    def free(self):
        if self.dev:
            self.d.free()


def check_lifts(what, V, E, call, devs=(False, True), modes=MODES):
    """call(blob, dev) == E for the canonical V and for every lift of it, host- and device-resident; all the lifted cases run
    before the verdict so that one failure names every mode and placement that fails"""
    failed = []
    for dev in devs:
        where = "device" if dev else "host"
        same = call(RL.pack(V), dev) == E      # (compared outside the assert: no diff of kilobytes of bytes in the report)
        assert same, "%s: the canonical input itself (%s-resident) does not give the oracle's bytes" % (what, where)
        for mode in modes:
            got = call(RL.pack(RL.lift(V, mode)), dev)
            if got != E:
                failed.append("%s/%s" % (mode, where))
    assert not failed, "%s: inputs >= r give other bytes than their residues: %s" % (what, ", ".join(failed))


# ---- element-wise vector operations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["sub", "mul"])
def test_fr_vec_sub_and_mul(eng, op):
    """kzg_fr_vec_sub / kzg_fr_vec_mul at n = 777 (four blocks, the last one ragged): every pairing of a canonical, fully lifted,
    sparsely lifted and edge-lifted a with such a b -- (a < r, b >= r), (a >= r, b < r), both >= r, position by position."""
    n = 777
    a, b = _vec_pair(random.Random(1), n)
    fn = eng.lib.kzg_fr_vec_sub if op == "sub" else eng.lib.kzg_fr_vec_mul
    E = RL.pack([(x - y) % R if op == "sub" else x * y % R for x, y in zip(a, b)])
    assert E[:64] == bytes(64)              # 0 - 0 in both forms of 0 (r - 2r, 2r - r under "edges" / "all"): zero bytes
    failed = []
    for dev in (False, True):
        for ma, mb in itertools.product((None,) + MODES, repeat=2):
            A = Buf(eng, RL.pack(RL.lift(a, ma) if ma else a), dev)
            B = Buf(eng, RL.pack(RL.lift(b, mb) if mb else b), dev)
            ok(eng, fn(eng.ctx, A.ptr, B.ptr, n, CAN, A.flags))
            got = A.read()
            A.free(), B.free()
            if ma is None and mb is None:
                same = got == E
                assert same, "canonical operands"
            elif got != E:
                bad = [i for i in range(n) if got[32 * i:32 * i + 32] != E[32 * i:32 * i + 32]]
                failed.append("a:%s b:%s %s (%d elements, first %d)" % (ma, mb, "device" if dev else "host", len(bad), bad[0]))
    assert not failed, "kzg_fr_vec_%s: operands >= r give other bytes than their residues: %s" % (op, "; ".join(failed))


def test_divide_by_z_on_coset(eng):
    """kzg_divide_by_z_on_coset takes log_n, not a length: 2^10 elements (four blocks)"""
    log_n = 10
    V = RL.base(random.Random(2), 1 << log_n)
    zi = pow(pow(7, 1 << log_n, R) - 1, -1, R)
    E = RL.pack([v * zi % R for v in V])

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        ok(eng, eng.lib.kzg_divide_by_z_on_coset(eng.ctx, A.ptr, log_n, CAN, A.flags))
        got = A.read()
        A.free()
        return got
    check_lifts("kzg_divide_by_z_on_coset", V, E, call)


# ---- evaluation form on the domain: k_eval_quotient -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", M_INDICES)
def test_quotient_eval(eng, evals, m):
    V = evals[0]
    E = quotient_on_domain(V, m)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(32 * D)
        ok(eng, eng.lib.kzg_quotient_eval(eng.ctx, A.ptr, D, m, CAN, A.flags, out))
        A.free()
        return out.raw
    check_lifts("kzg_quotient_eval(m=%d)" % m, V, E, call)


@pytest.mark.parametrize("m", M_INDICES)
def test_witness_eval(eng, kit, evals, m):
    V = evals[0]
    lag = kit("lag", D)
    E = witness_at(evals, pow(omega(D), m, R), V[m])

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(96)
        ok(eng, eng.lib.kzg_witness_eval(eng.ctx, lag.handle, A.ptr, D, m, CAN, A.flags, out, AFF))
        A.free()
        return out.raw
    check_lifts("kzg_witness_eval(m=%d)" % m, V, E, call)


def test_witness_eval_many(eng, kit, evals):
    V = evals[0]
    lag = kit("lag", D)
    idx = list(M_INDICES) + [7, 512]
    E = b"".join(witness_at(evals, pow(omega(D), m, R), V[m]) for m in idx)
    arr = (ctypes.c_size_t * len(idx))(*idx)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(96 * len(idx))
        ok(eng, eng.lib.kzg_witness_eval_many(eng.ctx, lag.handle, A.ptr, D, arr, len(idx), CAN, A.flags, out, AFF))
        A.free()
        return out.raw
    check_lifts("kzg_witness_eval_many", V, E, call)


# ---- evaluation form at any point: one z off the domain and one z = w^m in the same batch -----------------------------------------
def test_eval_form_eval(eng, evals):
    V, coeffs, _ = evals
    zs = [Z_OFF, pow(omega(D), M_ON, R)]
    E = le(C.poly_eval(coeffs, Z_OFF)) + le(V[M_ON])

    def call(blob, dev):
        A = Buf(eng, blob + blob, dev)     # the same vector twice: one polynomial per point
        out = ctypes.create_string_buffer(64)
        ok(eng, eng.lib.kzg_eval_form_eval(eng.ctx, A.ptr, D, 2, le(zs[0]) + le(zs[1]), CAN, A.flags, out))
        A.free()
        return out.raw
    check_lifts("kzg_eval_form_eval", V, E, call)


@pytest.mark.parametrize("on_domain", [False, True], ids=["off-domain", "z=w^m"])
def test_quotient_eval_at(eng, evals, on_domain):
    V, coeffs, _ = evals
    z = pow(omega(D), M_ON, R) if on_domain else Z_OFF
    y, q = OM.quotient_at(V, z)
    assert y == C.poly_eval(coeffs, z)
    if on_domain:
        assert RL.pack(q) == quotient_on_domain(V, M_ON), "the two oracles of the quotient on the domain disagree"
    E = (le(y), RL.pack(q))

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        yo, qo = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * D)
        ok(eng, eng.lib.kzg_quotient_eval_at(eng.ctx, A.ptr, D, le(z), CAN, A.flags, yo, qo))
        A.free()
        return yo.raw, qo.raw
    check_lifts("kzg_quotient_eval_at", V, E, call)


def test_open_eval(eng, kit, evals):
    V, coeffs, _ = evals
    lag = kit("lag", D)
    zs = [Z_OFF, pow(omega(D), M_ON, R)]
    ys = [C.poly_eval(coeffs, Z_OFF), V[M_ON]]
    E = (le(ys[0]) + le(ys[1]), witness_at(evals, zs[0], ys[0]) + witness_at(evals, zs[1], ys[1]))

    def call(blob, dev):
        A = Buf(eng, blob + blob, dev)
        yo, wo = ctypes.create_string_buffer(64), ctypes.create_string_buffer(192)
        ok(eng, eng.lib.kzg_open_eval(eng.ctx, lag.handle, A.ptr, D, 2, le(zs[0]) + le(zs[1]), CAN, A.flags, yo, wo, AFF))
        A.free()
        return yo.raw, wo.raw
    check_lifts("kzg_open_eval", V, E, call)


def test_open_fold_eval_on_the_domain(eng, kit):
    """one group of t = 3 vectors at z = w^m (the off-domain route is in tests/test_gpu_open_fold.py): the fold reduces on load,
    the folded vector then takes k_eval_quotient"""
    t, rng = 3, random.Random(4)
    lag = kit("lag", D)
    V = RL.base(rng, t * D)
    vecs = [V[i * D:(i + 1) * D] for i in range(t)]
    gamma = rng.randrange(1, R)
    z = pow(omega(D), M_ON, R)
    F = [sum(pow(gamma, i, R) * vecs[i][j] for i in range(t)) % R for j in range(D)]
    Fc = C.fft(F, inverse=True)
    E = (b"".join(le(v[M_ON]) for v in vecs), g1((C.poly_eval(Fc, TAU) - F[M_ON]) * pow(TAU - z, -1, R)))

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        yo, wo = ctypes.create_string_buffer(32 * t), ctypes.create_string_buffer(96)
        ok(eng, eng.lib.kzg_open_fold_eval(eng.ctx, lag.handle, A.ptr, D, t, 1, le(z), le(gamma), CAN, A.flags, yo, wo, AFF))
        A.free()
        return yo.raw, wo.raw
    check_lifts("kzg_open_fold_eval", V, E, call)


# ---- transforms -------------------------------------------------------------------------------------------------------------------
# 2^0: one word; 2^10: k_ntt_single; 2^13: the smallest two-pass size
@pytest.mark.parametrize("log_n", [0, 10, 13])
def test_ntt_fr(eng, log_n):
    n = 1 << log_n
    V = RL.base(random.Random(50 + log_n), n)
    for inverse in (0, 1):
        E = C.fft_bytes(RL.pack(V), log_n, inverse=bool(inverse))

        def call(blob, dev):
            A = Buf(eng, blob, dev)
            ok(eng, eng.lib.kzg_ntt_fr(eng.ctx, A.ptr, log_n, inverse, A.flags))
            got = A.read()
            A.free()
            return got
        check_lifts("kzg_ntt_fr(2^%d, inverse=%d)" % (log_n, inverse), V, E, call)


@pytest.mark.limit(300)
def test_ntt_fr_three_passes_2_23(eng):
    """2^23, the smallest three-pass size: the oracle's FFT there costs what tests/test_gpu_ntt_large.py::test_ntt_bit_exact_vs_oracle
    spends on it (one run per direction), so the input comes from kzg_fill_random_fr with the planted residues written over its
    head, stays device-resident, and takes the "sparse" and "edges" lifts (every 7th word and the six edge words)."""
    log_n = 23
    n = 1 << log_n
    buf = eng.alloc_scalars(n).fill_random(2323)
    V = RL.pack(RL.PLANTED) + buf.download()[32 * len(RL.PLANTED):]
    lifted = {mode: RL.lift_bytes(V, mode) for mode in ("sparse", "edges")}
    for inverse in (0, 1):
        E = C.fft_bytes(V, log_n, inverse=bool(inverse))
        buf.upload(V)
        ok(eng, eng.lib.kzg_ntt_fr(eng.ctx, buf.ptr, log_n, inverse, L.IN_DEVICE))
        same = buf.download() == E
        assert same, "canonical input"
        failed = []
        for mode, blob in lifted.items():
            buf.upload(blob)
            ok(eng, eng.lib.kzg_ntt_fr(eng.ctx, buf.ptr, log_n, inverse, L.IN_DEVICE))
            if buf.download() != E:
                failed.append(mode)
        assert not failed, "kzg_ntt_fr(2^23, inverse=%d): words >= r give other bytes than their residues: %s" % (inverse, failed)
    buf.free()


@pytest.mark.parametrize("log_n", [10, 13])
def test_coset_ntt_fr(eng, log_n):
    n = 1 << log_n
    V = RL.base(random.Random(60 + log_n), n)
    for inverse in (0, 1):
        if inverse:
            E = RL.pack(_coset_scale(C.fft(V, inverse=True), pow(7, -1, R)))
        else:
            E = C.fft_bytes(RL.pack(_coset_scale(V, 7)), log_n)

        def call(blob, dev):
            A = Buf(eng, blob, dev)
            ok(eng, eng.lib.kzg_coset_ntt_fr(eng.ctx, A.ptr, log_n, inverse, CAN, A.flags))
            got = A.read()
            A.free()
            return got
        check_lifts("kzg_coset_ntt_fr(2^%d, inverse=%d)" % (log_n, inverse), V, E, call)


# ---- coefficient form: the Horner scan (one coefficient past a block of 2048) -----------------------------------------------------
def test_poly_eval(eng, poly):
    V, x, y, _ = poly

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(32)
        ok(eng, eng.lib.kzg_poly_eval(eng.ctx, A.ptr, NC, le(x), CAN, A.flags, out))
        A.free()
        return out.raw
    check_lifts("kzg_poly_eval", V, le(y), call)


def test_quotient_linear(eng, poly):
    V, x, y, _ = poly
    E, nz = C.witness_quotient_bytes(RL.pack(V), NC, x, y)
    assert not nz

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(32 * (NC - 1))
        ok(eng, eng.lib.kzg_quotient_linear(eng.ctx, A.ptr, NC, le(x), le(y), CAN, A.flags, out))
        A.free()
        return out.raw
    check_lifts("kzg_quotient_linear", V, E, call)


def test_witness_coeff(eng, kit, poly):
    V, x, y, ptau = poly
    gs = kit("gs", 4096)
    E = g1((ptau - y) * pow(TAU - x, -1, R))

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(96)
        ok(eng, eng.lib.kzg_witness_coeff(eng.ctx, gs.handle, A.ptr, NC, le(x), le(y), CAN, A.flags, out, AFF))
        A.free()
        return out.raw
    check_lifts("kzg_witness_coeff", V, E, call)


def test_witness_coeff_many(eng, kit, poly):
    V, x, y, ptau = poly
    gs = kit("gs", 4096)
    rng = random.Random(6)
    xs = [x, rng.randrange(R), 0]
    ys = [y, C.poly_eval(V, xs[1]), V[0]]
    E = (b"".join(g1((ptau - b) * pow(TAU - a, -1, R)) for a, b in zip(xs, ys)), [0, 0, 0])

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out, st = ctypes.create_string_buffer(96 * 3), (ctypes.c_int * 3)(9, 9, 9)
        ok(eng, eng.lib.kzg_witness_coeff_many(eng.ctx, gs.handle, A.ptr, NC, RL.pack(xs), RL.pack(ys), 3, CAN, A.flags, out, AFF, st))
        A.free()
        return out.raw, list(st)
    check_lifts("kzg_witness_coeff_many", V, E, call)


def test_witness_coeff_batched(eng, kit):
    """n = 300, k = 7 (a shape of test_create_witness_batched): w = [(p - I)/Z]_1 and r = I through the python model"""
    n, k = 300, 7
    rng = random.Random(7)
    gs = kit("gs", 4096)
    V = RL.base(rng, n)
    xs = [rng.randrange(R) for _ in range(k)]
    ys = [C.poly_eval(V, x) for x in xs]
    I = M.Polynomial.lagrange_interpolation_with_tree(xs, ys, M.SubProductTree.new_from_points(xs))
    Z = 1
    for v in xs:
        Z = Z * (TAU - v) % R
    E = (g1((C.poly_eval(V, TAU) - I.eval(TAU)) * pow(Z, -1, R)), RL.pack(I.coeffs[:k]), k)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out, rbuf, rlen = ctypes.create_string_buffer(96), ctypes.create_string_buffer(32 * k), ctypes.c_size_t()
        ok(eng, eng.lib.kzg_witness_coeff_batched(eng.ctx, gs.handle, A.ptr, n, RL.pack(xs), RL.pack(ys), k, CAN, A.flags, out, AFF, rbuf,
                                                  ctypes.byref(rlen)))
        A.free()
        return out.raw, rbuf.raw, rlen.value
    check_lifts("kzg_witness_coeff_batched", V, E, call)


@pytest.mark.parametrize("na,nb", [(50, 50), (300, 7)])
def test_poly_mul(eng, na, nb):
    rng = random.Random(8 + na)
    a, b = RL.base(rng, na), RL.base(rng, nb)
    E = RL.pack(M.Polynomial(a, na - 1).mul_naive(M.Polynomial(b, nb - 1)).coeffs[:na + nb - 1])

    def call(blob, dev):
        A, B = Buf(eng, blob[:32 * na], dev), Buf(eng, blob[32 * na:], dev)
        out = ctypes.create_string_buffer(32 * (na + nb - 1))
        ok(eng, eng.lib.kzg_poly_mul(eng.ctx, A.ptr, na, B.ptr, nb, CAN, A.flags, out))
        A.free(), B.free()
        return out.raw
    check_lifts("kzg_poly_mul", a + b, E, call)


# ---- commitments and MSMs at 2^12 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scalars():
    """V (NM values) and [sum V_i TAU^i]G, the commitment of V as coefficients"""
    V = RL.base(random.Random(9), NM)
    return V, g1(C.poly_eval(V, TAU))


def test_commit_coeff_and_verify_poly_coeff(eng, kit, scalars):
    V, E = scalars
    gs = kit("gs", 4096)
    off_by_one = g1(C.poly_eval(V, TAU) + 1)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out, good, bad = ctypes.create_string_buffer(96), ctypes.c_int(-1), ctypes.c_int(-1)
        ok(eng, eng.lib.kzg_commit_coeff(eng.ctx, gs.handle, A.ptr, NM, CAN, A.flags, out, AFF))
        ok(eng, eng.lib.kzg_verify_poly_coeff(eng.ctx, gs.handle, E, AFF, A.ptr, NM, CAN, A.flags, ctypes.byref(good)))
        ok(eng, eng.lib.kzg_verify_poly_coeff(eng.ctx, gs.handle, off_by_one, AFF, A.ptr, NM, CAN, A.flags, ctypes.byref(bad)))
        A.free()
        return out.raw, good.value, bad.value
    check_lifts("kzg_commit_coeff / kzg_verify_poly_coeff", V, (E, 1, 0), call)


def test_commit_eval_and_verify_poly_eval(eng, kit):
    V = RL.base(random.Random(10), NM)
    gs, lag = kit("gs", 4096), kit("lag", NM)
    ptau = C.poly_eval(C.fft(V, inverse=True), TAU)
    E, off_by_one = g1(ptau), g1(ptau + 1)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out, good, bad = ctypes.create_string_buffer(96), ctypes.c_int(-1), ctypes.c_int(-1)
        ok(eng, eng.lib.kzg_commit_eval(eng.ctx, lag.handle, A.ptr, NM, CAN, A.flags, out, AFF))
        ok(eng, eng.lib.kzg_verify_poly_eval(eng.ctx, gs.handle, E, AFF, A.ptr, NM, CAN, A.flags, ctypes.byref(good)))
        ok(eng, eng.lib.kzg_verify_poly_eval(eng.ctx, gs.handle, off_by_one, AFF, A.ptr, NM, CAN, A.flags, ctypes.byref(bad)))
        A.free()
        return out.raw, good.value, bad.value
    check_lifts("kzg_commit_eval / kzg_verify_poly_eval", V, (E, 1, 0), call)


def test_msm_g1_batch(eng, kit):
    batch = 3
    V = RL.base(random.Random(11), batch * NM)
    gs = kit("gs", 4096)
    E = b"".join(g1(C.poly_eval(V[b * NM:(b + 1) * NM], TAU)) for b in range(batch))

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(96 * batch)
        ok(eng, eng.lib.kzg_msm_g1_batch(eng.ctx, gs.handle, 0, A.ptr, NM, batch, CAN, A.flags, out, AFF))
        A.free()
        return out.raw
    check_lifts("kzg_msm_g1_batch", V, E, call)


# the widths the other files do not feed values >= r: a narrow one, 20 bits at the size tests/test_gpu_fullsize.py::test_wide_windows
# takes it (2^16), and both sort implementations of the 17-bit mode
@pytest.mark.parametrize("wb,single_pass,n", [(8, 0, NM), (17, 0, NM), (17, 1, NM), (20, 0, 1 << 16)])
def test_msm_g1_window_widths(eng, wb, single_pass, n):
    V = RL.base(random.Random(12 + wb), n)
    pw, acc = 1, 0
    for v in V:
        acc = (acc + v * pw) % R
        pw = pw * TAU % R
    E = g1(acc)
    eng.set_option("window_bits", wb)
    eng.set_option("sort_single_pass", single_pass)
    try:
        gs = kzg_amd.setup(eng, TAU, n, g2_len=0).gs
        assert gs.window_info()[0] == wb

        def call(blob, dev):
            A = Buf(eng, blob, dev)
            out = ctypes.create_string_buffer(96)
            ok(eng, eng.lib.kzg_msm_g1(eng.ctx, gs.handle, 0, A.ptr, n, CAN, A.flags, out, AFF))
            A.free()
            return out.raw
        check_lifts("kzg_msm_g1(window_bits=%d, sort_single_pass=%d)" % (wb, single_pass), V, E, call)
        gs.free()
    finally:
        eng.set_option("sort_single_pass", 0)
        eng.set_option("window_bits", 0)


def test_msm_g2(eng, kit):
    """host-resident scalars only (the call has no flags)"""
    from oracle import pairing_model as P
    n = 33
    V = RL.base(random.Random(13), n)
    hs = kit("hs", n)
    E = P.g2_to_uncompressed(P.g2_mul(P.G2, C.poly_eval(V, TAU)))

    def call(blob, dev):
        out = ctypes.create_string_buffer(192)
        ok(eng, eng.lib.kzg_msm_g2(eng.ctx, hs.handle, 0, blob, n, CAN, out, L.G2_UNCOMPRESSED))
        return out.raw
    check_lifts("kzg_msm_g2", V, E, call, devs=(False,))


# ---- FK20: every opening over the domain, points and cosets (the smallest plans of their own files) ---------------------------------
@pytest.mark.parametrize("form", ["coeff", "eval"])
def test_witness_all(eng, kit, form):
    N = 1 << FK_LOG_N
    V = RL.base(random.Random(20), N)
    plan = kzg_amd.FK20Plan(eng, kit("gs", 4096), FK_LOG_N)
    fn = eng.lib.kzg_witness_all_coeff if form == "coeff" else eng.lib.kzg_witness_all_eval
    E = _fk20_points_expect(V if form == "coeff" else C.fft(V, inverse=True), FK_LOG_N)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out = ctypes.create_string_buffer(96 * N)
        ok(eng, fn(eng.ctx, plan.handle, A.ptr, N, 1, CAN, A.flags, out, AFF))
        A.free()
        return out.raw
    try:
        check_lifts("kzg_witness_all_" + form, V, E, call)
    finally:
        plan.free()


@pytest.mark.parametrize("form", ["coeff", "eval"])
def test_witness_cosets(eng, kit, form):
    N, K = 1 << FK_LOG_N, 1 << (FK_LOG_N - FK_LOG_L)
    V = RL.base(random.Random(21), N)
    plan = kzg_amd.FK20CosetPlan(eng, kit("gs", 4096), FK_LOG_N, FK_LOG_L)
    fn = eng.lib.kzg_witness_cosets_coeff if form == "coeff" else eng.lib.kzg_witness_cosets_eval
    E = _fk20_cosets_expect(V if form == "coeff" else C.fft(V, inverse=True), FK_LOG_N, FK_LOG_L)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        out, rb = ctypes.create_string_buffer(96 * K), ctypes.create_string_buffer(32 * N)
        ok(eng, fn(eng.ctx, plan.handle, A.ptr, N, 1, CAN, A.flags, out, AFF, rb))
        A.free()
        return out.raw, rb.raw
    try:
        check_lifts("kzg_witness_cosets_" + form, V, E, call)
    finally:
        plan.free()


# ---- cells: recovery and the coset verifiers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cells():
    """one polynomial of 16 coefficients over the size-16 domain in cosets of 4: (coefficients, evaluations, cells, [q_i(tau)], p(tau))"""
    from tests import verify_cosets_model as VM
    P = [random.Random(22).randrange(R) for _ in range(16)]
    ev = C.fft(P)
    K = 4
    cs = [[ev[i + t * K] for t in range(4)] for i in range(K)]
    qs = [VM.quotient_at(P, VM.interpolant(cs[i], i, FK_LOG_N, FK_LOG_L), i, FK_LOG_N, FK_LOG_L, TAU) for i in range(K)]
    assert None not in qs
    return P, ev, cs, qs, C.poly_eval(P, TAU)


def test_recover_cosets(eng):
    """8 coefficients from 3 of the 4 cosets (12 values: one wrong value is detectable); the cells are the scalar input"""
    n, ids = 8, [3, 0, 2]
    P = [random.Random(23).randrange(R) for _ in range(n)]
    ev = C.fft(P + [0] * (16 - n))
    V = [ev[i + t * 4] for i in ids for t in range(4)]
    wrong = list(V)
    wrong[5] = (wrong[5] + 1) % R
    id_arr = (ctypes.c_size_t * 3)(*ids)

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        co, evs, st = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * 16), (ctypes.c_int * 1)(9)
        ok(eng, eng.lib.kzg_recover_cosets(eng.ctx, FK_LOG_N, FK_LOG_L, n, id_arr, 3, A.ptr, 1, CAN, A.flags, co, evs, st))
        A.free()
        return (co.raw, evs.raw, st[0]) if st[0] == 0 else st[0]
    check_lifts("kzg_recover_cosets", V, (RL.pack(P), RL.pack(ev), 0), call)
    check_lifts("kzg_recover_cosets (one value off by one)", wrong, 1, call)


@pytest.fixture(scope="module")
def vparams(eng):
    p = kzg_amd.setup(eng, TAU, 16, g2_len=17)
    yield p
    p.gs.free()
    p.hs.free()


@pytest.mark.parametrize("batch", [False, True], ids=["kzg_verify_cosets", "kzg_verify_cosets_batch"])
def test_verify_cosets(eng, vparams, cells, batch):
    _, _, cs, qs, ptau = cells
    K = 4
    ver = kzg_amd.CosetVerifier(eng, vparams, FK_LOG_N, FK_LOG_L)
    commitment, proofs = g1(ptau), b"".join(g1(q) for q in qs)
    idx, ids = (ctypes.c_uint32 * K)(0, 0, 0, 0), (ctypes.c_size_t * K)(0, 1, 2, 3)
    V = [v for c in cs for v in c]
    wrong = list(V)
    wrong[9] = (wrong[9] + 1) % R           # cell 2, value 1
    challenge = le(random.Random(24).randrange(1, R))

    def call(blob, dev):
        A = Buf(eng, blob, dev)
        if batch:
            res = ctypes.c_int(-1)
            ok(eng, eng.lib.kzg_verify_cosets_batch(eng.ctx, ver.handle, commitment, 1, idx, ids, A.ptr, proofs, K, challenge, CAN, AFF, A.flags,
                                                    ctypes.byref(res)))
            got = res.value
        else:
            res = ctypes.create_string_buffer(SENTINEL * K, K)
            ok(eng, eng.lib.kzg_verify_cosets(eng.ctx, ver.handle, commitment, 1, idx, ids, A.ptr, proofs, K, CAN, AFF, A.flags, res))
            got = list(res.raw)
        A.free()
        return got
    try:
        check_lifts("honest cells", V, 1 if batch else [1, 1, 1, 1], call)
        check_lifts("one value off by one", wrong, 0 if batch else [1, 1, 0, 1], call)
    finally:
        ver.free()


# ---- the pairing verifiers: the values (ys, the interpolant's coefficients) are the scalar input; host memory only ----------------------
def _openings(rng, count):
    """count openings as discrete logs: C_k = [v_k (tau - x_k) + y_k]G, w_k = [v_k]G, with the planted residues among the y_k"""
    xs = [rng.randrange(R) for _ in range(count)]
    ys = RL.base(rng, count)
    vs = [rng.randrange(1, R) for _ in range(count)]
    cm = b"".join(g1(v * (TAU - x) + y) for x, y, v in zip(xs, ys, vs))
    return xs, ys, cm, b"".join(g1(v) for v in vs)


def test_verify_eval(eng, vparams):
    count = 8
    xs, ys, cm, ws = _openings(random.Random(25), count)
    wrong = list(ys)
    wrong[3] = (wrong[3] + 1) % R

    def call(blob, dev):
        res = ctypes.create_string_buffer(SENTINEL * count, count)
        ok(eng, eng.lib.kzg_verify_eval(eng.ctx, vparams.gs.handle, vparams.hs.handle, RL.pack(xs), blob, CAN, cm, ws, AFF, count, res))
        return list(res.raw)
    check_lifts("kzg_verify_eval, honest", ys, [1] * count, call, devs=(False,))
    check_lifts("kzg_verify_eval, y_3 off by one", wrong, [int(k != 3) for k in range(count)], call, devs=(False,))


def test_verify_eval_batch(eng, vparams):
    count = 8
    xs, ys, cm, ws = _openings(random.Random(26), count)
    wrong = list(ys)
    wrong[7] = (wrong[7] + 1) % R           # position 7: lifted by "sparse"
    challenge = le(random.Random(27).randrange(1, R))

    def call(blob, dev):
        res = ctypes.c_int(-1)
        ok(eng, eng.lib.kzg_verify_eval_batch(eng.ctx, vparams.gs.handle, vparams.hs.handle, RL.pack(xs), blob, CAN, cm, count, None, ws, AFF, count,
                                              challenge, ctypes.byref(res)))
        return res.value
    check_lifts("kzg_verify_eval_batch, honest", ys, 1, call, devs=(False,))
    check_lifts("kzg_verify_eval_batch, y_7 off by one", wrong, 0, call, devs=(False,))


def test_verify_eval_batched(eng, vparams):
    """C = [v z(tau) + r(tau)]G, w = [v]G with z = prod (X - x_i): the interpolant's coefficients r are what the call feeds its MSM"""
    k, rng = 3, random.Random(28)
    xs = [rng.randrange(R) for _ in range(k)]
    r = RL.base(rng, k)
    r[2] = R - 1
    v, z = rng.randrange(1, R), 1
    for x in xs:
        z = z * (TAU - x) % R
    cm, w = g1(v * z + C.poly_eval(r, TAU)), g1(v)
    wrong = list(r)
    wrong[0] = (wrong[0] + 1) % R

    def call(blob, dev):
        res = ctypes.c_int(-1)
        ok(eng, eng.lib.kzg_verify_eval_batched(eng.ctx, vparams.gs.handle, vparams.hs.handle, RL.pack(xs), k, blob, k, CAN, cm, w, AFF, ctypes.byref(res)))
        return res.value
    check_lifts("kzg_verify_eval_batched, honest", r, 1, call, devs=(False,))
    check_lifts("kzg_verify_eval_batched, r_0 off by one", wrong, 0, call, devs=(False,))


def test_verify_eval_all(eng, kit, vparams):
    """the formula as written upstream (tests/test_gpu_verify.py::test_verify_eval_all_integer_reference): true exactly when
    v (L_{d-1}(tau) - L_0(tau)) = c - sum_i y_i L_i(tau)"""
    d, rng = 16, random.Random(29)
    w = omega(d)
    lag = [(pow(TAU, d, R) - 1) * pow(w, i, R) % R * pow(d * (TAU - pow(w, i, R)), -1, R) % R for i in range(d)]
    ys = RL.base(rng, d)
    v = rng.randrange(1, R)
    cm, wit = g1(v * (lag[d - 1] - lag[0]) + sum(y * l for y, l in zip(ys, lag))), g1(v)
    wrong = list(ys)
    wrong[14] = (wrong[14] + 1) % R         # position 14: lifted by "sparse"
    lag_g = kit("lag", d)
    lag_h = kzg_amd.setup_lagrange_g2(eng, TAU, d)

    def call(blob, dev):
        res = ctypes.c_int(-1)
        ok(eng, eng.lib.kzg_verify_eval_all(eng.ctx, lag_g.handle, lag_h.handle, vparams.hs.handle, blob, d, CAN, cm, wit, AFF, ctypes.byref(res)))
        return res.value
    try:
        check_lifts("kzg_verify_eval_all, honest", ys, 1, call, devs=(False,))
        check_lifts("kzg_verify_eval_all, y_14 off by one", wrong, 0, call, devs=(False,))
    finally:
        lag_h.free()


# ---- the device group (one GPU, no collective needed): n = d = 1024 -------------------------------------------------------------------
def test_sharded_commit_and_witness_coeff(group):
    n, rng = 1024, random.Random(30)
    V = RL.base(rng, n)
    x = rng.randrange(R)
    y, ptau = C.poly_eval(V, x), C.poly_eval(V, TAU)
    srs = group.setup(TAU, n)
    try:
        check_lifts("kzg_commit_coeff_sharded", V, g1(ptau),
                    lambda blob, dev: _group_call(group, lambda a: group.commit_batch(srs, a, n, 1)[0], blob, dev))
        check_lifts("kzg_witness_coeff_sharded", V, g1((ptau - y) * pow(TAU - x, -1, R)),
                    lambda blob, dev: _group_call(group, lambda a: group.create_witness(srs, a, (x, y)), blob, dev))
    finally:
        srs.free()


def test_sharded_witness_eval(group, kit, evals):
    V = evals[0]
    lag = group.upload(kit("lag", D).download(), D)
    try:
        for m in (0, D - 1):
            check_lifts("kzg_witness_eval_sharded(m=%d)" % m, V, witness_at(evals, pow(omega(D), m, R), V[m]),
                        lambda blob, dev: _group_call(group, lambda a: group.create_witness_eval(lag, a, m), blob, dev))
    finally:
        lag.free()


# ---- the other half of the rule: single host scalars must be < r ------------------------------------------------------------------------
def _sent(n):
    return ctypes.create_string_buffer(SENTINEL * n, n)


def _swap(words, which, j, word):
    """the packed host scalars `words` with entry j replaced by `word` when `which` names this array"""
    w = list(words)
    if which:
        w[j] = word
    return RL.pack(w)


def _host_scalar_cases(eng, kit, poly, evals):
    """(name, scalar arguments, run, expected): run(which, word) makes the call with the host scalar named `which` (None: none)
    replaced by `word` and returns (status, [every output buffer, filled with a sentinel beforehand]); expected = the good call's outputs"""
    V, x, y, ptau = poly
    EV, coeffs, _ = evals
    vb, eb = RL.pack(V), RL.pack(EV)
    gs, lag = kit("gs", 4096), kit("lag", D)
    lib, ctx = eng.lib, eng.ctx
    rng = random.Random(40)
    wit = g1((ptau - y) * pow(TAU - x, -1, R))
    cases = []

    def witness_coeff(which, word):
        out = _sent(96)
        rc = lib.kzg_witness_coeff(ctx, gs.handle, vb, NC, le(word if which == "x" else x), le(word if which == "y" else y), CAN, 0, out, AFF)
        return rc, [out.raw]
    cases.append(("kzg_witness_coeff", ("x", "y"), witness_coeff, [wit]))

    xs3 = [rng.randrange(R), x, 0]
    ys3 = [C.poly_eval(V, xs3[0]), y, V[0]]
    wit3 = b"".join(g1((ptau - b) * pow(TAU - a, -1, R)) for a, b in zip(xs3, ys3))

    def witness_coeff_many(which, word):
        out, st = _sent(96 * 3), (ctypes.c_int * 3)(-7, -7, -7)
        rc = lib.kzg_witness_coeff_many(ctx, gs.handle, vb, NC, _swap(xs3, which == "xs", 1, word), _swap(ys3, which == "ys", 1, word), 3, CAN, 0,
                                        out, AFF, st)
        return rc, [out.raw, list(st)]
    cases.append(("kzg_witness_coeff_many", ("xs", "ys"), witness_coeff_many, [wit3, [0, 0, 0]]))

    n, k = 300, 7
    bv = V[:n - 1] + [1]
    bxs = [rng.randrange(R) for _ in range(k)]
    bys = [C.poly_eval(bv, a) for a in bxs]
    I = M.Polynomial.lagrange_interpolation_with_tree(bxs, bys, M.SubProductTree.new_from_points(bxs))
    Z = 1
    for a in bxs:
        Z = Z * (TAU - a) % R
    bw = g1((C.poly_eval(bv, TAU) - I.eval(TAU)) * pow(Z, -1, R))

    def witness_coeff_batched(which, word):
        out, rb, rl = _sent(96), _sent(32 * k), ctypes.c_size_t(12345)
        rc = lib.kzg_witness_coeff_batched(ctx, gs.handle, RL.pack(bv), n, _swap(bxs, which == "xs", 2, word), _swap(bys, which == "ys", 2, word), k,
                                           CAN, 0, out, AFF, rb, ctypes.byref(rl))
        return rc, [out.raw, rb.raw, rl.value]
    cases.append(("kzg_witness_coeff_batched", ("xs", "ys"), witness_coeff_batched, [bw, RL.pack(I.coeffs[:k]), k]))

    def witness_coeff_batched_k1(which, word):
        out, rb, rl = _sent(96), _sent(64), ctypes.c_size_t(12345)
        rc = lib.kzg_witness_coeff_batched(ctx, gs.handle, vb, NC, le(word if which == "xs" else x), le(word if which == "ys" else y), 1, CAN, 0, out, AFF,
                                           rb, ctypes.byref(rl))
        return rc, [out.raw, rb.raw, rl.value]
    # k = 1, the reference's quirk: r = X + (y - x), w = [(p - r)/(X - x)]_1 = [(p(tau) - tau - y + x) / (tau - x)]G
    cases.append(("kzg_witness_coeff_batched(k=1)", ("xs", "ys"), witness_coeff_batched_k1,
                  [g1((ptau - TAU - y + x) * pow(TAU - x, -1, R)), le((y - x) % R) + le(1), 2]))

    def poly_eval(which, word):
        out = _sent(32)
        return lib.kzg_poly_eval(ctx, vb, NC, le(word if which else x), CAN, 0, out), [out.raw]
    cases.append(("kzg_poly_eval", ("x",), poly_eval, [le(y)]))

    def quotient_linear(which, word):
        out = _sent(32 * (NC - 1))
        rc = lib.kzg_quotient_linear(ctx, vb, NC, le(word if which == "x" else x), le(word if which == "y" else y), CAN, 0, out)
        return rc, [out.raw]
    cases.append(("kzg_quotient_linear", ("x", "y"), quotient_linear, [C.witness_quotient_bytes(vb, NC, x, y)[0]]))

    zs = [Z_OFF, pow(omega(D), M_ON, R)]
    yz = [C.poly_eval(coeffs, Z_OFF), EV[M_ON]]

    def eval_form_eval(which, word):
        out = _sent(64)
        return lib.kzg_eval_form_eval(ctx, eb + eb, D, 2, _swap(zs, which, 1, word), CAN, 0, out), [out.raw]
    cases.append(("kzg_eval_form_eval", ("zs",), eval_form_eval, [le(yz[0]) + le(yz[1])]))

    def quotient_eval_at(which, word):
        yo, qo = _sent(32), _sent(32 * D)
        return lib.kzg_quotient_eval_at(ctx, eb, D, le(word if which else zs[1]), CAN, 0, yo, qo), [yo.raw, qo.raw]
    cases.append(("kzg_quotient_eval_at", ("z",), quotient_eval_at, [le(yz[1]), quotient_on_domain(EV, M_ON)]))

    def open_eval(which, word):
        yo, wo = _sent(64), _sent(192)
        return lib.kzg_open_eval(ctx, lag.handle, eb + eb, D, 2, _swap(zs, which, 0, word), CAN, 0, yo, wo, AFF), [yo.raw, wo.raw]
    cases.append(("kzg_open_eval", ("zs",), open_eval, [le(yz[0]) + le(yz[1]), witness_at(evals, zs[0], yz[0]) + witness_at(evals, zs[1], yz[1])]))

    def domain_z(which, word):
        out = _sent(32)
        return lib.kzg_domain_z(D, le(word if which else x), CAN, out), [out.raw]
    cases.append(("kzg_domain_z", ("tau",), domain_z, [le((pow(x, D, R) - 1) % R)]))
    return cases


def test_host_scalar_out_of_range_is_a_shape_error(eng, kit, poly, evals):
    """x, y of kzg_witness_coeff; xs, ys of kzg_witness_coeff_many and _batched; x of kzg_poly_eval; x, y of kzg_quotient_linear; the zs
    of the three open-at-any-point calls; tau of kzg_domain_z: r and 2^256 - 1 are KZG_ERR_SHAPE, every output keeps its sentinel
    bytes, and the same context then gives the good call's outputs."""
    failed = []
    for name, scalar_args, run, expected in _host_scalar_cases(eng, kit, poly, evals):
        rc, outs = run(None, None)
        good = rc == 0 and outs == expected
        assert good, "%s: the good call itself (%d, %s)" % (name, rc, eng.last_error())
        for which in scalar_args:
            for word in BAD_SCALARS:
                rc, outs = run(which, word)
                # the sentinels: 0xA5 bytes, -7 in a status array, 12345 in a length
                kept = all(o == SENTINEL * len(o) if isinstance(o, bytes) else (o == [-7] * len(o) if isinstance(o, list) else o == 12345) for o in outs)
                if rc != L.KZG_ERR_SHAPE or not kept:
                    failed.append("%s(%s = %s): status %d%s" % (name, which, "r" if word == R else "2^256 - 1", rc, "" if kept else ", an output was written"))
                rc2, outs2 = run(None, None)
                good = rc2 == 0 and outs2 == expected
                assert good, "%s: the context after the refused call" % name
    assert not failed, "host scalars >= r that are not refused with KZG_ERR_SHAPE before memory is touched: " + "; ".join(failed)


def test_srs_setup_secret_out_of_range_is_a_shape_error(eng):
    """s of the five kzg_srs_setup_* calls: r and 2^256 - 1 are KZG_ERR_SHAPE and the handle is not written; the good call then gives
    setup(s, n) of the oracle"""
    from oracle import pairing_model as P
    n, first = 4, 3
    lib, ctx = eng.lib, eng.ctx
    mark = 0x5A5A5A5A5A5A
    g1_points = C.setup_g1(TAU, first + n)
    g2_points = P.setup_g2(TAU, n)
    calls = {
        "kzg_srs_setup_g1": (lambda s, h: lib.kzg_srs_setup_g1(ctx, s, CAN, n, h), "g1", g1_points[:96 * n]),
        "kzg_srs_setup_g1_shard": (lambda s, h: lib.kzg_srs_setup_g1_shard(ctx, s, CAN, first, n, h), "g1", g1_points[96 * first:]),
        "kzg_srs_setup_lagrange_g1": (lambda s, h: lib.kzg_srs_setup_lagrange_g1(ctx, s, CAN, n, h), "g1",
                                      b"".join(M.g1_to_affine_mont(p) for p in M.lagrange_basis_g1_known_tau(TAU, n))),
        "kzg_srs_setup_g2": (lambda s, h: lib.kzg_srs_setup_g2(ctx, s, CAN, n, h), "g2", b"".join(P.g2_to_affine_mont(p) for p in g2_points)),
        "kzg_srs_setup_lagrange_g2": (lambda s, h: lib.kzg_srs_setup_lagrange_g2(ctx, s, CAN, n, h), "g2",
                                      b"".join(P.g2_to_affine_mont(p) for p in P.lagrange_basis_g2_known_tau(TAU, n))),
    }
    for name, (fn, kind, expected) in calls.items():
        for word in BAD_SCALARS:
            h = ctypes.c_void_p(mark)
            assert fn(le(word), ctypes.byref(h)) == L.KZG_ERR_SHAPE, (name, hex(word))
            assert h.value == mark, (name, "the handle was written")
        h = ctypes.c_void_p()
        ok(eng, fn(le(TAU), ctypes.byref(h)))
        srs = kzg_amd.Srs(eng, h) if kind == "g1" else kzg_amd.SrsG2(eng, h)
        try:
            assert srs.download() == expected, name
        finally:
            srs.free()
