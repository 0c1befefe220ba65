"""include/kzg_mi355x.h: every scalar-carrying entry point takes `sfmt`, KZG_FR_CANONICAL_LE_32 or KZG_FR_MONT_LE_32, and `flags` says
where buffers live.  tests/test_gpu_scalar_residues.py walks the older core of the library call by call in canonical form; this file is
the other axis of the same table: the same calls at the same shapes (tests/scalar_call_cases.py) in BOTH formats and in every placement.

Per call a base input V (every value < r) gives the expected result E through the oracle (oracle/c_oracle.py, oracle/kzg_model.py or
the model of the call's own file); the oracle only ever sees canonical V and no expectation is taken from a GPU run.  With
mont(v) = v * 2^256 mod r, check_formats() runs the call
  * in canonical form -- every scalar output must be E, byte for byte -- and, after that verdict, with every scalar input (vectors and
    single host scalars alike) replaced by its Montgomery word under KZG_FR_MONT_LE_32: every scalar output must be mont(E) byte for
    byte (so Montgomery outputs are below r), every point, verdict, status array and length the canonical expectation;
  * each format with all inputs in host memory, with the inputs resident in HBM (KZG_IN_DEVICE) and host outputs and, where the call
    has a device output, with KZG_IN_DEVICE | KZG_OUT_DEVICE into a buffer filled with 0xA5: the bytes behind the documented length
    of every output (host outputs too) must still be 0xA5;
  * and after every run each input the header declares const is read back and compared with what was handed in.  Exempt is only the
    argument an in-place call transforms: the data of kzg_coset_ntt_fr and kzg_divide_by_z_on_coset, `a` of kzg_fr_vec_mul / _sub.
All failing (format, placement) pairs of one format are collected before the assertion, which names them and what differed.
Montgomery words of r or above are outside the contract ("in KZG_FR_MONT_LE_32 inputs are below r") and are not fed.

The table: every prototype of include/kzg_mi355x.h with an sfmt parameter (73) and the test that compares it with an oracle or a model
in Montgomery form and with device-resident buffers.  "here" is this file; another file is named where its test already does both.  A call
whose own file runs Montgomery form in host memory only, or holds it against the library's own canonical output only, has its case here.

  kzg_srs_setup_g1, _g1_shard, _lagrange_g1, kzg_srs_setup_g2, _lagrange_g2     here::test_srs_setups (one host scalar; no flags)
  kzg_srs_setup_g1_sharded                  here::test_sharded_srs_setup
  kzg_msm_g1, kzg_msm_g1_batch              here::test_msm_g1, test_msm_g1_batch, test_alternating_formats_on_one_context
  kzg_commit_coeff_sharded, _sharded_batch  here::test_sharded_commit
  kzg_witness_coeff_sharded, kzg_witness_coeff_batched_sharded, kzg_witness_eval_sharded
                                            here::test_sharded_witness_coeff, test_sharded_witness_coeff_batched, test_sharded_witness_eval
                                            (the sharded calls refuse KZG_OUT_DEVICE: host results)
  kzg_compute_omega, kzg_domain_z           here::test_host_helpers_in_both_formats (host-only: runs without a GPU)
  kzg_coset_ntt_fr                          here::test_coset_ntt_fr
  kzg_coset_ntt_fr_batch                    tests/test_gpu_ntt_batch.py::test_coset (Montgomery words in place in HBM, against the oracle's FFT)
  kzg_divide_by_z_on_coset                  here::test_divide_by_z_on_coset
  kzg_fr_vec_mul, kzg_fr_vec_sub            here::test_fr_vec_sub_and_mul, test_alternating_formats_on_one_context
  kzg_commit_coeff, kzg_verify_poly_coeff   here::test_commit_coeff_and_verify_poly_coeff
  kzg_commit_eval, kzg_verify_poly_eval     here::test_commit_eval_and_verify_poly_eval
  kzg_witness_coeff, kzg_witness_coeff_many here::test_witness_coeff, test_witness_coeff_many
  kzg_witness_coeff_batched                 here::test_witness_coeff_batched, test_point_set_cache_keeps_the_formats_apart
  kzg_witness_eval, kzg_witness_eval_many   here::test_witness_eval, test_witness_eval_many
  kzg_eval_form_eval, kzg_quotient_eval_at  here::test_eval_form_eval, test_quotient_eval_at
  kzg_open_eval                             here::test_open_eval (tests/test_gpu_open_eval.py runs Montgomery form in host memory only)
  kzg_fr_fold                               tests/test_gpu_open_fold.py::test_fold_formats_and_device_buffers
  kzg_open_fold_eval, kzg_open_fold_coeff   here::test_open_fold_eval, test_open_fold_coeff (their file: Montgomery form in host memory, eval form only)
  kzg_fr_lincomb                            tests/test_gpu_multiopen.py::test_lincomb_formats_device_buffers_and_residues
  kzg_fr_batch_inverse                      tests/test_gpu_fr_scan.py::test_batch_inverse (the model), ::test_batch_inverse_in_place_on_the_device_and_against_vec_mul
                                            (HBM, in place and out of place: in * out == 1 element by element)
  kzg_fr_scan                               tests/test_gpu_fr_scan.py::test_scan_device_buffers
  kzg_fr_grand_product                      here::test_fr_grand_product (its file runs device buffers in canonical form only)
  kzg_multiopen_eval_commit, _eval_finish, kzg_multiopen_coeff_commit, _coeff_finish
                                            here::test_multiopen_eval, test_multiopen_coeff (their file takes its expectation from the library's
                                            single-polynomial calls in canonical form)
  kzg_witness_all_coeff, _all_eval          here::test_witness_all (tests/test_gpu_fk20.py compares with the library's canonical output)
  kzg_witness_cosets_coeff, _cosets_eval    here::test_witness_cosets (tests/test_gpu_fk20_cosets.py: likewise)
  kzg_recover_cosets                        tests/test_gpu_recover.py::test_formats_and_residency
  kzg_msm_g2                                here::test_msm_g2 (host scalars; no flags)
  kzg_msm_g2_bucket                         tests/test_gpu_g2_msm.py::test_scalar_formats_residency_and_output_formats
  kzg_verify_eval                           tests/test_gpu_verify.py::test_verify_eval_by_the_wave            (the verifiers take host memory only,
  kzg_verify_eval_batched                   tests/test_gpu_verify.py::test_verify_eval_batched_integer_reference   but for the cells of the coset calls)
  kzg_verify_eval_all                       tests/test_gpu_verify.py::test_verify_eval_all_integer_reference
  kzg_verify_eval_tree                      tests/test_gpu_witness_tree.py::test_formats_count_zero_and_errors_leave_ok_untouched
  kzg_witness_coeff_tree                    here::test_witness_coeff_tree (its file compares with the library's canonical output)
  kzg_verify_cosets                         tests/test_gpu_verify_cosets.py::test_formats_flags_and_chunks
  kzg_verify_cosets_batch                   tests/test_gpu_verify_cosets_batch.py::test_host_pairing_formats_and_device_cells
  kzg_verify_eval_batch                     tests/test_gpu_verify_eval_batch.py::test_formats_host_pairing_and_trusted_points
  kzg_verify_fold, kzg_verify_multiopen     here::test_verify_fold, test_verify_multiopen (their files: no Montgomery verdict / the honest one only)
  kzg_poly_eval, kzg_quotient_linear        here::test_poly_eval, test_quotient_linear
  kzg_quotient_eval, kzg_poly_mul           here::test_quotient_eval, test_poly_mul, test_alternating_formats_on_one_context
  kzg_poly_multi_eval                       tests/test_gpu_multi_eval.py::test_formats_buffers_and_a_batch_of_three
  kzg_interpolate                           tests/test_gpu_multi_eval.py::test_interpolation_of_three_value_vectors_both_formats_and_a_device_output
                                            (xs and ys are host scalars; the output in HBM)
  kzg_point_tree_setup, _product, _eval, _combine, _interpolate   tests/test_gpu_point_tree.py::test_formats_and_residency
  kzg_poly_divide                           tests/test_gpu_poly_divide.py::test_flag_combinations_and_single_outputs
  kzg_fill_random_fr                        here::test_fill_random_fr (a device output and nothing else)

Like the residues file this one sorts after the tests that release the session's contexts (tests/conftest.py ORDER), so it opens and
closes a module-scoped Engine of its own (tests/fk20_common.py)."""
import ctypes
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import open_eval_model as OM
from tests import residue_lift as RL
from tests.fk20_common import dev_buffer, dev_download, eng  # noqa: F401 -- eng: this module's fixture
from tests.scalar_call_cases import (AFF, CAN, D, FK_LOG_L, FK_LOG_N, M_INDICES, M_ON, MONT, NC, NM, R, TAU, Z_OFF, batched_opening, coset_scale,  # noqa: F401
                                     fk20_cosets_expect, fk20_points_expect, g1, le, omega, quotient_on_domain, vec_pair, witness_at, evals, group,
                                     kit, poly)

gpu = pytest.mark.gpu          # per test: test_host_helpers_in_both_formats runs without a GPU

SENTINEL = b"\xa5"
PAD = 64                       # sentinel bytes behind the documented length of every output


def mont(v):
    return v * M.FR_MONT_R % R


class Fmt:
    def __init__(self, name, sfmt, conv):
        self.name, self.sfmt, self.conv = name, sfmt, conv

    def word(self, v):
        return le(self.conv(v))

    def pack(self, values):
        return RL.pack([self.conv(v) for v in values])


CANONICAL = Fmt("canonical", CAN, lambda v: v)
MONTGOMERY = Fmt("montgomery", MONT, mont)
FORMATS = (CANONICAL, MONTGOMERY)          # canonical first: its verdict comes before the Montgomery runs
assert MONTGOMERY.word(1) == M.fr_to_mont_le(1)

# (name, inputs resident in HBM, outputs in HBM)
HOST, IN_DEV, IN_OUT_DEV = ("host", False, False), ("in-device", True, False), ("in+out-device", True, True)
NO_DEV_OUT = (HOST, IN_DEV)
ALL_PLACES = (HOST, IN_DEV, IN_OUT_DEV)


def unpack(blob):
    return [int.from_bytes(blob[i:i + 32], "little") for i in range(0, len(blob), 32)]


class Mem:
    """`data` followed by PAD sentinel bytes, in host memory or (dev) in HBM"""

    def __init__(self, e, data, dev):
        self.e, self.dev, self.data = e, dev, bytes(data)
        whole = self.data + SENTINEL * PAD
        if dev:
            self.ptr = dev_buffer(e, len(whole))
            assert e.lib.kzg_dev_upload(e.ctx, self.ptr, whole, len(whole)) == 0
        else:
            self.ptr = ctypes.create_string_buffer(whole, len(whole))

    def read(self):
        """(what lies where `data` was put, whether the bytes behind it are still the sentinel)"""
        n = len(self.data)
        raw = dev_download(self.e, self.ptr, n + PAD) if self.dev else self.ptr.raw
        return raw[:n], raw[n:] == SENTINEL * PAD

    def free(self):
        if self.dev and self.ptr:
            self.e.lib.kzg_dev_free(self.e.ctx, self.ptr)
            self.ptr = None


class Run:
    """one (format, placement) of a call: makes its buffers, and afterwards reads the outputs and looks at what must not have changed"""

    def __init__(self, e, fmt, place, last_error=None):
        self.e, self.f, self.last_error = e, fmt, last_error or e.last_error
        self.where, self.in_dev, self.out_dev = place
        self.sfmt = fmt.sfmt
        self.flags = (L.IN_DEVICE if self.in_dev else 0) | (L.OUT_DEVICE if self.out_dev else 0)
        self.consts, self.outs, self.notes, self.got = [], [], [], {}

    def inp(self, name, values):
        """a const scalar vector in this run's format and placement"""
        return self.raw_inp(name, self.f.pack(values), self.in_dev)

    def raw_inp(self, name, data, dev=False):
        m = Mem(self.e, data, dev)
        self.consts.append((name, m))
        return m.ptr

    def host(self, name, values):
        """const host scalars (x, y, xs, zs ..): never device-resident"""
        return self.raw_inp(name, self.f.pack(values), False)

    def inout(self, name, values):
        """the argument an in-place call transforms: an output that starts as the input, where the inputs live"""
        m = Mem(self.e, self.f.pack(values), self.in_dev)
        self.outs.append((name, m))
        return m.ptr

    def out(self, name, nbytes, dev=None):
        """an output of nbytes documented bytes, filled with the sentinel; dev=False: a host-only output (values, verdicts)"""
        m = Mem(self.e, SENTINEL * nbytes, self.out_dev if dev is None else dev)
        self.outs.append((name, m))
        return m.ptr

    def ok(self, rc, want=0):
        if rc != want:
            self.notes.append("status %d instead of %d (%s)" % (rc, want, self.last_error()))

    def finish(self):
        for name, m in self.outs:
            self.got[name], clean = m.read()
            if not clean:
                self.notes.append("bytes behind the end of %s were written" % name)
        for name, m in self.consts:
            now, clean = m.read()
            if now != m.data or not clean:
                self.notes.append("the const input %s was changed" % name)
        self.free()

    def free(self):
        for _, m in self.consts + self.outs:
            m.free()


def check_formats(e, what, call, E, places=ALL_PLACES, formats=FORMATS, last_error=None):
    """call(run) makes the raw library call through run's buffers (and may put further results into run.got).  E: name -> ("fr", the
    canonical values of a scalar output) or ("is", the bytes / value every format must give).  One verdict per format, canonical first,
    over all placements."""
    for fmt in formats:
        failed = []
        for place in places:
            run = Run(e, fmt, place, last_error)
            try:
                call(run)
                run.finish()
            finally:
                run.free()
            for name, (kind, want) in E.items():
                same = run.got[name] == (fmt.pack(want) if kind == "fr" else want)   # (compared here: no kilobytes in the report)
                if not same:
                    failed.append("%s/%s: %s differs" % (fmt.name, run.where, name))
            failed += ["%s/%s: %s" % (fmt.name, run.where, note) for note in run.notes]
        assert not failed, "%s, against the oracle's %s result: %s" % (what, "canonical" if fmt is CANONICAL else "mont()", "; ".join(failed))


# ---- host-only helpers: no GPU needed ---------------------------------------------------------------------------------------------
def test_host_helpers_in_both_formats():
    """kzg_domain_z converts tau on the way in and z on the way out; kzg_compute_omega writes omega in sfmt"""
    lib = kzg_amd.load()
    failed = []
    x = random.Random(41).randrange(R)
    for fmt in FORMATS:
        for d in (1, 5, 1024):
            for tau in (0, 1, x, R - 1):
                src = ctypes.create_string_buffer(fmt.word(tau), 32)
                out = ctypes.create_string_buffer(SENTINEL * (32 + PAD), 32 + PAD)
                rc = lib.kzg_domain_z(d, src, fmt.sfmt, out)
                if rc != 0 or out.raw != fmt.word((pow(tau, d, R) - 1) % R) + SENTINEL * PAD or src.raw != fmt.word(tau):
                    failed.append("kzg_domain_z(d=%d, tau=%#x)/%s" % (d, tau, fmt.name))
        for d in (1, 2, 3, 1000, 1 << 13):
            m, exp, w = M.compute_omega(d)
            mo, eo = ctypes.c_size_t(), ctypes.c_uint32()
            out = ctypes.create_string_buffer(SENTINEL * (32 + PAD), 32 + PAD)
            rc = lib.kzg_compute_omega(d, ctypes.byref(mo), ctypes.byref(eo), out, fmt.sfmt)
            if rc != 0 or (mo.value, eo.value) != (m, exp) or out.raw != fmt.word(w) + SENTINEL * PAD:
                failed.append("kzg_compute_omega(%d)/%s" % (d, fmt.name))
    assert not failed, failed


# ---- element-wise vector operations -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("op", ["sub", "mul"])
def test_fr_vec_sub_and_mul(eng, op):
    """n = 777: four blocks, the last one ragged; a < b, a = b, a > b (tests/scalar_call_cases.py).  a is transformed, b is const."""
    n = 777
    a, b = vec_pair(random.Random(1), n)
    fn = eng.lib.kzg_fr_vec_sub if op == "sub" else eng.lib.kzg_fr_vec_mul
    E = {"a": ("fr", [(x - y) % R if op == "sub" else x * y % R for x, y in zip(a, b)])}

    def call(run):
        pa, pb = run.inout("a", a), run.inp("b", b)
        run.ok(fn(eng.ctx, pa, pb, n, run.sfmt, run.flags))
    check_formats(eng, "kzg_fr_vec_" + op, call, E, NO_DEV_OUT)


@gpu
def test_divide_by_z_on_coset(eng):
    log_n = 10
    V = RL.base(random.Random(2), 1 << log_n)
    zi = pow(pow(7, 1 << log_n, R) - 1, -1, R)

    def call(run):
        run.ok(eng.lib.kzg_divide_by_z_on_coset(eng.ctx, run.inout("data", V), log_n, run.sfmt, run.flags))
    check_formats(eng, "kzg_divide_by_z_on_coset", call, {"data": ("fr", [v * zi % R for v in V])}, NO_DEV_OUT)


@gpu
@pytest.mark.parametrize("u64_valued", [0, 1])
def test_fill_random_fr(eng, u64_valued):
    """every word of both fills against the generator's definition (oracle/kzg_model.py: canonical v, Montgomery mont(v)), one of them
    against kzg_amd.splitmix_scalar as well; n = 2049: one element past eight blocks"""
    n, seed = 2049, 0xC0FFEE
    V = [M.splitmix_scalar(seed, i, bool(u64_valued)) for i in range(n)]
    assert V[n - 1] == kzg_amd.splitmix_scalar(seed, n - 1, bool(u64_valued))
    assert not u64_valued or max(V) < 1 << 64

    def call(run):
        run.ok(eng.lib.kzg_fill_random_fr(eng.ctx, run.out("dst", 32 * n, dev=True), n, seed, u64_valued, run.sfmt))
    check_formats(eng, "kzg_fill_random_fr(u64_valued=%d)" % u64_valued, call, {"dst": ("fr", V)}, (IN_OUT_DEV,))


# ---- transforms -------------------------------------------------------------------------------------------------------------------
# 2^10: k_ntt_single; 2^13: the smallest two-pass size
@gpu
@pytest.mark.parametrize("log_n", [10, 13])
def test_coset_ntt_fr(eng, log_n):
    n = 1 << log_n
    V = RL.base(random.Random(60 + log_n), n)
    for inverse in (0, 1):
        if inverse:
            E = coset_scale(C.fft(V, inverse=True), pow(7, -1, R))
        else:
            E = C.fft(coset_scale(V, 7))

        def call(run):
            run.ok(eng.lib.kzg_coset_ntt_fr(eng.ctx, run.inout("data", V), log_n, inverse, run.sfmt, run.flags))
        check_formats(eng, "kzg_coset_ntt_fr(2^%d, inverse=%d)" % (log_n, inverse), call, {"data": ("fr", E)}, NO_DEV_OUT)


# ---- coefficient form ---------------------------------------------------------------------------------------------------------------
@gpu
def test_poly_eval(eng, poly):
    V, x, y, _ = poly

    def call(run):
        run.ok(eng.lib.kzg_poly_eval(eng.ctx, run.inp("coeffs", V), NC, run.host("x", [x]), run.sfmt, run.flags, run.out("y", 32, dev=False)))
    check_formats(eng, "kzg_poly_eval", call, {"y": ("fr", [y])}, NO_DEV_OUT)


@gpu
def test_quotient_linear(eng, poly):
    """the call ends by comparing the device's p(x), which has the form of the coefficients, with the caller's y bytes: in Montgomery
    form a y one off and the right y handed over as its canonical bytes are both KZG_ERR_POINT_NOT_ON_POLY"""
    V, x, y, _ = poly
    q, nz = C.witness_quotient_bytes(RL.pack(V), NC, x, y)
    assert not nz

    def call(run):
        run.ok(eng.lib.kzg_quotient_linear(eng.ctx, run.inp("coeffs", V), NC, run.host("x", [x]), run.host("y", [y]), run.sfmt, run.flags,
                                           run.out("q", 32 * (NC - 1))))
    check_formats(eng, "kzg_quotient_linear", call, {"q": ("fr", unpack(q))})

    for what, ybytes in (("y + 1", MONTGOMERY.word((y + 1) % R)), ("mont(y) + 1", le((mont(y) + 1) % R)), ("the canonical bytes of y", le(y))):
        def wrong(run):
            run.ok(eng.lib.kzg_quotient_linear(eng.ctx, run.inp("coeffs", V), NC, run.host("x", [x]), run.raw_inp("y", ybytes), run.sfmt, run.flags,
                                               run.out("q", 32 * (NC - 1), dev=False)), want=L.KZG_ERR_POINT_NOT_ON_POLY)
        check_formats(eng, "kzg_quotient_linear with %s for y" % what, wrong, {}, NO_DEV_OUT, (MONTGOMERY,))


@gpu
@pytest.mark.parametrize("na,nb", [(50, 50), (300, 7)])
def test_poly_mul(eng, na, nb):
    rng = random.Random(8 + na)
    a, b = RL.base(rng, na), RL.base(rng, nb)
    E = M.Polynomial(a, na - 1).mul_naive(M.Polynomial(b, nb - 1)).coeffs[:na + nb - 1]

    def call(run):
        run.ok(eng.lib.kzg_poly_mul(eng.ctx, run.inp("a", a), na, run.inp("b", b), nb, run.sfmt, run.flags, run.out("out", 32 * (na + nb - 1))))
    check_formats(eng, "kzg_poly_mul(%d, %d)" % (na, nb), call, {"out": ("fr", list(E))})


@gpu
def test_witness_coeff(eng, kit, poly):
    V, x, y, ptau = poly
    gs = kit("gs", 4096)

    def call(run):
        run.ok(eng.lib.kzg_witness_coeff(eng.ctx, gs.handle, run.inp("coeffs", V), NC, run.host("x", [x]), run.host("y", [y]), run.sfmt, run.flags,
                                         run.out("w", 96), AFF))
    check_formats(eng, "kzg_witness_coeff", call, {"w": ("is", g1((ptau - y) * pow(TAU - x, -1, R)))})


@gpu
def test_witness_coeff_many(eng, kit, poly):
    """three openings, one of them at 0"""
    V, x, y, ptau = poly
    gs = kit("gs", 4096)
    xs = [x, random.Random(6).randrange(R), 0]
    ys = [y, C.poly_eval(V, xs[1]), V[0]]
    E = {"w": ("is", b"".join(g1((ptau - b) * pow(TAU - a, -1, R)) for a, b in zip(xs, ys))), "status": ("is", [0, 0, 0])}

    def call(run):
        st = (ctypes.c_int * 3)(9, 9, 9)
        run.ok(eng.lib.kzg_witness_coeff_many(eng.ctx, gs.handle, run.inp("coeffs", V), NC, run.host("xs", xs), run.host("ys", ys), 3, run.sfmt,
                                              run.flags, run.out("w", 96 * 3), AFF, st))
        run.got["status"] = list(st)
    check_formats(eng, "kzg_witness_coeff_many", call, E)


@gpu
def test_witness_coeff_batched(eng, kit):
    """n = 300, k = 7: xs and ys are host scalars in sfmt and out_r, the interpolant, comes back in sfmt (always host memory)"""
    n, k = 300, 7
    rng = random.Random(7)
    gs = kit("gs", 4096)
    V = RL.base(rng, n)
    xs = [rng.randrange(R) for _ in range(k)]
    ys = [C.poly_eval(V, x) for x in xs]
    w, I = batched_opening(V, xs, ys)

    def call(run):
        rlen = ctypes.c_size_t()
        run.ok(eng.lib.kzg_witness_coeff_batched(eng.ctx, gs.handle, run.inp("coeffs", V), n, run.host("xs", xs), run.host("ys", ys), k, run.sfmt,
                                                 run.flags, run.out("w", 96), AFF, run.out("r", 32 * k, dev=False), ctypes.byref(rlen)))
        run.got["r_len"] = rlen.value
    check_formats(eng, "kzg_witness_coeff_batched", call, {"w": ("is", w), "r": ("fr", I), "r_len": ("is", k)})


# ---- evaluation form on the domain ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("m", M_INDICES)
def test_quotient_eval(eng, evals, m):
    V = evals[0]

    def call(run):
        run.ok(eng.lib.kzg_quotient_eval(eng.ctx, run.inp("evals", V), D, m, run.sfmt, run.flags, run.out("q", 32 * D)))
    check_formats(eng, "kzg_quotient_eval(m=%d)" % m, call, {"q": ("fr", unpack(quotient_on_domain(V, m)))})


@gpu
def test_eval_form_eval(eng, evals):
    """two polynomials (the same vector twice), one opened off the domain and one at z = w^m"""
    V, coeffs, _ = evals
    zs = [Z_OFF, pow(omega(D), M_ON, R)]

    def call(run):
        run.ok(eng.lib.kzg_eval_form_eval(eng.ctx, run.inp("evals", V + V), D, 2, run.host("zs", zs), run.sfmt, run.flags, run.out("ys", 64, dev=False)))
    check_formats(eng, "kzg_eval_form_eval", call, {"ys": ("fr", [C.poly_eval(coeffs, Z_OFF), V[M_ON]])}, NO_DEV_OUT)


@gpu
@pytest.mark.parametrize("on_domain", [False, True], ids=["off-domain", "z=w^m"])
def test_quotient_eval_at(eng, evals, on_domain):
    V, coeffs, _ = evals
    z = pow(omega(D), M_ON, R) if on_domain else Z_OFF
    y, q = OM.quotient_at(V, z)
    assert y == C.poly_eval(coeffs, z)

    def call(run):
        run.ok(eng.lib.kzg_quotient_eval_at(eng.ctx, run.inp("evals", V), D, run.host("z", [z]), run.sfmt, run.flags, run.out("y", 32, dev=False),
                                            run.out("q", 32 * D)))
    check_formats(eng, "kzg_quotient_eval_at", call, {"y": ("fr", [y]), "q": ("fr", list(q))})


# ---- commitments, MSMs and eval-form witnesses at 2^12 ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def evals12():
    """V (NM values), its coefficients, p(TAU)"""
    V = RL.base(random.Random(10), NM)
    coeffs = C.fft(V, inverse=True)
    return V, coeffs, C.poly_eval(coeffs, TAU)


def _one_off(V):
    W = list(V)
    W[5] = (W[5] + 1) % R
    return W


@gpu
def test_commit_coeff_and_verify_poly_coeff(eng, kit):
    """honest coefficients verify (1); one coefficient off by one does not (0)"""
    V = RL.base(random.Random(9), NM)
    gs = kit("gs", 4096)
    E = g1(C.poly_eval(V, TAU))

    def call(run):
        good, bad = ctypes.c_int(-1), ctypes.c_int(-1)
        pv = run.inp("coeffs", V)
        run.ok(eng.lib.kzg_commit_coeff(eng.ctx, gs.handle, pv, NM, run.sfmt, run.flags, run.out("c", 96), AFF))
        run.ok(eng.lib.kzg_verify_poly_coeff(eng.ctx, gs.handle, E, AFF, pv, NM, run.sfmt, run.flags & L.IN_DEVICE, ctypes.byref(good)))
        run.ok(eng.lib.kzg_verify_poly_coeff(eng.ctx, gs.handle, E, AFF, run.inp("coeffs, one off", _one_off(V)), NM, run.sfmt, run.flags & L.IN_DEVICE,
                                             ctypes.byref(bad)))
        run.got["honest"], run.got["one off"] = good.value, bad.value
    check_formats(eng, "kzg_commit_coeff / kzg_verify_poly_coeff", call, {"c": ("is", E), "honest": ("is", 1), "one off": ("is", 0)})


@gpu
def test_commit_eval_and_verify_poly_eval(eng, kit, evals12):
    V, _, ptau = evals12
    gs, lag = kit("gs", 4096), kit("lag", NM)
    E = g1(ptau)

    def call(run):
        good, bad = ctypes.c_int(-1), ctypes.c_int(-1)
        pv = run.inp("evals", V)
        run.ok(eng.lib.kzg_commit_eval(eng.ctx, lag.handle, pv, NM, run.sfmt, run.flags, run.out("c", 96), AFF))
        run.ok(eng.lib.kzg_verify_poly_eval(eng.ctx, gs.handle, E, AFF, pv, NM, run.sfmt, run.flags & L.IN_DEVICE, ctypes.byref(good)))
        run.ok(eng.lib.kzg_verify_poly_eval(eng.ctx, gs.handle, E, AFF, run.inp("evals, one off", _one_off(V)), NM, run.sfmt, run.flags & L.IN_DEVICE,
                                            ctypes.byref(bad)))
        run.got["honest"], run.got["one off"] = good.value, bad.value
    check_formats(eng, "kzg_commit_eval / kzg_verify_poly_eval", call, {"c": ("is", E), "honest": ("is", 1), "one off": ("is", 0)})


@gpu
def test_msm_g1(eng, kit):
    V = RL.base(random.Random(12), NM)
    gs = kit("gs", 4096)

    def call(run):
        run.ok(eng.lib.kzg_msm_g1(eng.ctx, gs.handle, 0, run.inp("scalars", V), NM, run.sfmt, run.flags, run.out("out", 96), AFF))
    check_formats(eng, "kzg_msm_g1", call, {"out": ("is", g1(C.poly_eval(V, TAU)))})


@gpu
def test_msm_g1_batch(eng, kit):
    batch = 3
    V = RL.base(random.Random(11), batch * NM)
    gs = kit("gs", 4096)
    E = b"".join(g1(C.poly_eval(V[b * NM:(b + 1) * NM], TAU)) for b in range(batch))

    def call(run):
        run.ok(eng.lib.kzg_msm_g1_batch(eng.ctx, gs.handle, 0, run.inp("scalars", V), NM, batch, run.sfmt, run.flags, run.out("out", 96 * batch), AFF))
    check_formats(eng, "kzg_msm_g1_batch", call, {"out": ("is", E)})


@gpu
def test_msm_g2(eng, kit):
    """host-resident scalars only (the call has no flags)"""
    from oracle import pairing_model as P
    n = 20
    V = RL.base(random.Random(13), n)
    hs = kit("hs", n)
    E = P.g2_to_uncompressed(P.g2_mul(P.G2, C.poly_eval(V, TAU)))

    def call(run):
        run.ok(eng.lib.kzg_msm_g2(eng.ctx, hs.handle, 0, run.inp("scalars", V), n, run.sfmt, run.out("out", 192), L.G2_UNCOMPRESSED))
    check_formats(eng, "kzg_msm_g2", call, {"out": ("is", E)}, (HOST,))


@gpu
@pytest.mark.parametrize("m", (0, 1, 7, NM - 1))
def test_witness_eval(eng, kit, evals12, m):
    V = evals12[0]
    lag = kit("lag", NM)
    E = witness_at(evals12, pow(omega(NM), m, R), V[m])

    def call(run):
        run.ok(eng.lib.kzg_witness_eval(eng.ctx, lag.handle, run.inp("evals", V), NM, m, run.sfmt, run.flags, run.out("w", 96), AFF))
    check_formats(eng, "kzg_witness_eval(m=%d)" % m, call, {"w": ("is", E)})


@gpu
def test_witness_eval_many(eng, kit, evals12):
    V = evals12[0]
    lag = kit("lag", NM)
    idx = [0, 1, 7, NM - 1, 7, 2048]
    E = b"".join(witness_at(evals12, pow(omega(NM), m, R), V[m]) for m in idx)
    arr = (ctypes.c_size_t * len(idx))(*idx)

    def call(run):
        run.ok(eng.lib.kzg_witness_eval_many(eng.ctx, lag.handle, run.inp("evals", V), NM, arr, len(idx), run.sfmt, run.flags, run.out("w", 96 * len(idx)),
                                             AFF))
    check_formats(eng, "kzg_witness_eval_many", call, {"w": ("is", E)})
    assert list(arr) == idx


# ---- SRS setups: the secret is one host scalar in sfmt ---------------------------------------------------------------------------------
@gpu
def test_srs_setups(eng):
    """the secret as a Montgomery word gives the SRS bytes the canonical secret gives: the oracle's chain"""
    from oracle import pairing_model as P
    n, first, d, n2 = 130, 3, 16, 5
    lib, ctx = eng.lib, eng.ctx
    g1_points = C.setup_g1(TAU, first + n)
    calls = {
        "kzg_srs_setup_g1": (lambda s, f, h: lib.kzg_srs_setup_g1(ctx, s, f, n, h), "g1", g1_points[:96 * n]),
        "kzg_srs_setup_g1_shard": (lambda s, f, h: lib.kzg_srs_setup_g1_shard(ctx, s, f, first, n, h), "g1", g1_points[96 * first:]),
        "kzg_srs_setup_lagrange_g1": (lambda s, f, h: lib.kzg_srs_setup_lagrange_g1(ctx, s, f, d, h), "g1",
                                      b"".join(M.g1_to_affine_mont(p) for p in M.lagrange_basis_g1_known_tau(TAU, d))),
        "kzg_srs_setup_g2": (lambda s, f, h: lib.kzg_srs_setup_g2(ctx, s, f, n2, h), "g2", b"".join(P.g2_to_affine_mont(p) for p in P.setup_g2(TAU, n2))),
        "kzg_srs_setup_lagrange_g2": (lambda s, f, h: lib.kzg_srs_setup_lagrange_g2(ctx, s, f, d, h), "g2",
                                      b"".join(P.g2_to_affine_mont(p) for p in P.lagrange_basis_g2_known_tau(TAU, d))),
    }
    for fmt in FORMATS:
        failed = []
        for name, (fn, kind, expected) in calls.items():
            secret = ctypes.create_string_buffer(fmt.word(TAU), 32)
            h = ctypes.c_void_p()
            rc = fn(secret, fmt.sfmt, ctypes.byref(h))
            if rc != 0:
                failed.append("%s: status %d (%s)" % (name, rc, eng.last_error()))
                continue
            srs = kzg_amd.Srs(eng, h) if kind == "g1" else kzg_amd.SrsG2(eng, h)
            try:
                if srs.download() != expected or secret.raw != fmt.word(TAU):
                    failed.append(name)
            finally:
                srs.free()
        assert not failed, "the %s secret does not give the oracle's SRS: %s" % (fmt.name, failed)


# ---- the device group (one GPU, no collective needed): n = d = 1024 -----------------------------------------------------------------------
GN = 1024


def check_group(group, what, call, E):
    """check_formats for the sharded calls: the polynomial as a host blob, or resident on the group's GPU, where the argument is an array
    of one device pointer per local GPU.  These calls refuse KZG_OUT_DEVICE: their results are host memory."""
    e = group.engine(0)

    def shim(run):
        def whole(name, values):
            p = run.inp(name, values)
            return (ctypes.c_void_p * 1)(p.value) if run.in_dev else p
        call(run, whole)
    check_formats(e, what, shim, E, NO_DEV_OUT, last_error=group.last_error)


@gpu
def test_sharded_srs_setup(group):
    want = C.setup_g1(TAU, GN)
    for fmt in FORMATS:
        h = ctypes.c_void_p()
        rc = group.lib.kzg_srs_setup_g1_sharded(group.handle, fmt.word(TAU), fmt.sfmt, GN, ctypes.byref(h))
        assert rc == 0, (fmt.name, rc, group.last_error())
        srs = kzg_amd.ShardedSrs(group, h)
        try:
            shard, first = srs.shard(0)
            same = shard.download() == want
            assert same and first == 0 and len(srs) == GN, "kzg_srs_setup_g1_sharded: the %s secret does not give the oracle's SRS" % fmt.name
        finally:
            srs.free()


@pytest.fixture(scope="module")
def gsrs(group):
    s = group.setup(TAU, GN)
    yield s
    s.free()


@gpu
def test_sharded_commit(group, gsrs):
    batch = 3
    V = RL.base(random.Random(30), batch * GN)
    E = [g1(C.poly_eval(V[b * GN:(b + 1) * GN], TAU)) for b in range(batch)]

    def one(run, whole):
        run.ok(group.lib.kzg_commit_coeff_sharded(group.handle, gsrs.handle, whole("coeffs", V[:GN]), GN, run.sfmt, run.flags, run.out("c", 96), AFF))
    check_group(group, "kzg_commit_coeff_sharded", one, {"c": ("is", E[0])})

    def many(run, whole):
        run.ok(group.lib.kzg_commit_coeff_sharded_batch(group.handle, gsrs.handle, whole("coeffs", V), GN, batch, run.sfmt, run.flags,
                                                        run.out("c", 96 * batch), AFF))
    check_group(group, "kzg_commit_coeff_sharded_batch", many, {"c": ("is", b"".join(E))})


@gpu
def test_sharded_witness_coeff(group, gsrs):
    rng = random.Random(31)
    V = RL.base(rng, GN)
    x = rng.randrange(R)
    y, ptau = C.poly_eval(V, x), C.poly_eval(V, TAU)

    def call(run, whole):
        run.ok(group.lib.kzg_witness_coeff_sharded(group.handle, gsrs.handle, whole("coeffs", V), GN, run.host("x", [x]), run.host("y", [y]), run.sfmt,
                                                   run.flags, run.out("w", 96), AFF))
    check_group(group, "kzg_witness_coeff_sharded", call, {"w": ("is", g1((ptau - y) * pow(TAU - x, -1, R)))})


@gpu
def test_sharded_witness_coeff_batched(group, gsrs):
    k, rng = 7, random.Random(32)
    V = RL.base(rng, GN)
    xs = [rng.randrange(R) for _ in range(k)]
    ys = [C.poly_eval(V, x) for x in xs]
    w, I = batched_opening(V, xs, ys)

    def call(run, whole):
        rlen = ctypes.c_size_t()
        run.ok(group.lib.kzg_witness_coeff_batched_sharded(group.handle, gsrs.handle, whole("coeffs", V), GN, run.host("xs", xs), run.host("ys", ys), k,
                                                           run.sfmt, run.flags, run.out("w", 96), AFF, run.out("r", 32 * k), ctypes.byref(rlen)))
        run.got["r_len"] = rlen.value
    check_group(group, "kzg_witness_coeff_batched_sharded", call, {"w": ("is", w), "r": ("fr", I), "r_len": ("is", k)})


@gpu
def test_sharded_witness_eval(group, kit, evals):
    V = evals[0]
    assert D == GN
    lag = group.upload(kit("lag", D).download(), D)
    try:
        for m in (0, D - 1):
            def call(run, whole):
                run.ok(group.lib.kzg_witness_eval_sharded(group.handle, lag.handle, whole("evals", V), D, m, run.sfmt, run.flags, run.out("w", 96), AFF))
            check_group(group, "kzg_witness_eval_sharded(m=%d)" % m, call, {"w": ("is", witness_at(evals, pow(omega(D), m, R), V[m]))})
    finally:
        lag.free()


# ---- calls whose own files run Montgomery form only in host memory, or only against the library's canonical output ------------------------
@gpu
def test_open_eval(eng, kit, evals):
    """two polynomials, one opened off the domain and one at z = w^m"""
    V, coeffs, _ = evals
    lag = kit("lag", D)
    zs = [Z_OFF, pow(omega(D), M_ON, R)]
    ys = [C.poly_eval(coeffs, Z_OFF), V[M_ON]]

    def call(run):
        run.ok(eng.lib.kzg_open_eval(eng.ctx, lag.handle, run.inp("evals", V + V), D, 2, run.host("zs", zs), run.sfmt, run.flags,
                                     run.out("ys", 64, dev=False), run.out("w", 192), AFF))
    check_formats(eng, "kzg_open_eval", call, {"ys": ("fr", ys), "w": ("is", witness_at(evals, zs[0], ys[0]) + witness_at(evals, zs[1], ys[1]))})


def _folded(vecs, gamma):
    return [sum(pow(gamma, i, R) * v[j] for i, v in enumerate(vecs)) % R for j in range(len(vecs[0]))]


@gpu
def test_open_fold_eval(eng, kit):
    """two groups of t = 3 vectors: one opened off the domain, one at z = w^m"""
    t, rng = 3, random.Random(35)
    lag = kit("lag", D)
    V = RL.base(rng, 2 * t * D)
    zs, gammas = [Z_OFF, pow(omega(D), M_ON, R)], [rng.randrange(1, R), rng.randrange(1, R)]
    ys, ws = [], b""
    for g in range(2):
        vecs = [V[(g * t + i) * D:(g * t + i + 1) * D] for i in range(t)]
        ys += [C.poly_eval(C.fft(v, inverse=True), zs[g]) for v in vecs]
        Fc = C.fft(_folded(vecs, gammas[g]), inverse=True)
        ws += g1((C.poly_eval(Fc, TAU) - C.poly_eval(Fc, zs[g])) * pow(TAU - zs[g], -1, R))

    def call(run):
        run.ok(eng.lib.kzg_open_fold_eval(eng.ctx, lag.handle, run.inp("evals", V), D, t, 2, run.host("zs", zs), run.host("gammas", gammas), run.sfmt,
                                          run.flags, run.out("ys", 32 * 2 * t, dev=False), run.out("w", 192), AFF))
    check_formats(eng, "kzg_open_fold_eval", call, {"ys": ("fr", ys), "w": ("is", ws)})


@gpu
def test_open_fold_coeff(eng, kit):
    """two groups of t = 3 polynomials of 300 coefficients; the second group is opened at 0"""
    n, t, rng = 300, 3, random.Random(36)
    gs = kit("gs", 4096)
    V = RL.base(rng, 2 * t * n)
    zs, gammas = [rng.randrange(R), 0], [rng.randrange(1, R), rng.randrange(1, R)]
    ys, ws = [], b""
    for g in range(2):
        polys = [V[(g * t + i) * n:(g * t + i + 1) * n] for i in range(t)]
        ys += [C.poly_eval(p, zs[g]) for p in polys]
        F = _folded(polys, gammas[g])
        ws += g1((C.poly_eval(F, TAU) - C.poly_eval(F, zs[g])) * pow(TAU - zs[g], -1, R))

    def call(run):
        run.ok(eng.lib.kzg_open_fold_coeff(eng.ctx, gs.handle, run.inp("coeffs", V), n, t, 2, run.host("zs", zs), run.host("gammas", gammas), run.sfmt,
                                           run.flags, run.out("ys", 32 * 2 * t, dev=False), run.out("w", 192), AFF))
    check_formats(eng, "kzg_open_fold_coeff", call, {"ys": ("fr", ys), "w": ("is", ws)})


@gpu
def test_verify_fold(eng):
    """two groups of t = 3 claims as discrete logs: C_i = [c_i]G, pi_g = [sum_i gamma_g^i (c_i - y_i) / (tau - z_g)]G.  Honest: 1; one value
    off by one: 0.  Every scalar (zs, ys, gammas, r) travels in sfmt; host memory only."""
    t, groups, rng = 3, 2, random.Random(37)
    params = kzg_amd.setup(eng, TAU, 4, g2_len=2)
    try:
        zs = [rng.randrange(R) for _ in range(groups)]
        gammas = [rng.randrange(1, R) for _ in range(groups)]
        r = rng.randrange(1, R)
        cs, ys = [rng.randrange(R) for _ in range(groups * t)], RL.base(rng, groups * t)
        cm = b"".join(g1(c) for c in cs)
        ws = b"".join(g1(sum(pow(gammas[g], i, R) * (cs[g * t + i] - ys[g * t + i]) for i in range(t)) * pow(TAU - zs[g], -1, R)) for g in range(groups))
        wrong = list(ys)
        wrong[4] = (wrong[4] + 1) % R

        def call(run):
            for name, vals in (("honest", ys), ("one off", wrong)):
                res = ctypes.c_int(-1)
                run.ok(eng.lib.kzg_verify_fold(eng.ctx, params.gs.handle, params.hs.handle, run.host("zs", zs), run.host("ys, " + name, vals), run.sfmt, cm,
                                               groups * t, None, ws, AFF, t, groups, run.host("gammas", gammas), run.host("r", [r]), ctypes.byref(res)))
                run.got[name] = res.value
        check_formats(eng, "kzg_verify_fold", call, {"honest": ("is", 1), "one off": ("is", 0)}, (HOST,))
    finally:
        params.gs.free()
        params.hs.free()


def _u32s(values):
    return (ctypes.c_uint32 * len(values))(*values)


def _multiopen_claims(rng, points):
    """seven claims on three polynomials at three distinct points, r, and a t that is none of the points"""
    zs, idx = [points[k % 3] for k in range(7)], [0, 1, 2, 2, 1, 0, 0]
    return zs, idx, rng.randrange(1, R), rng.randrange(R)


@gpu
def test_multiopen_coeff(eng, kit):
    """both phases through tests/multiopen_model.py: g and g_out live where the inputs live (KZG_IN_DEVICE), D and pi follow KZG_OUT_DEVICE"""
    from tests import multiopen_model as MO
    n, rng = 50, random.Random(38)
    gs = kit("gs", 4096)
    V = RL.base(rng, 3 * n)
    polys = [V[i * n:(i + 1) * n] for i in range(3)]
    zs, idx, r, t = _multiopen_claims(rng, [rng.randrange(R), 0, R - 1])
    ys, g = MO.commit_coeff(polys, idx, zs, r)
    vt, q = MO.finish_coeff(polys, idx, zs, r, t, g)

    def commit(run):
        run.ok(eng.lib.kzg_multiopen_coeff_commit(eng.ctx, gs.handle, run.inp("coeffs", V), n, 3, _u32s(idx), run.host("zs", zs), len(zs), run.host("r", [r]),
                                                  run.sfmt, run.flags, run.out("ys", 32 * len(zs), dev=False), run.out("g", 32 * (n - 1), dev=run.in_dev),
                                                  run.out("D", 96), AFF))
    check_formats(eng, "kzg_multiopen_coeff_commit", commit, {"ys": ("fr", ys), "g": ("fr", g), "D": ("is", g1(C.poly_eval(g, TAU)))})

    def finish(run):
        run.ok(eng.lib.kzg_multiopen_coeff_finish(eng.ctx, gs.handle, run.inp("coeffs", V), n, 3, _u32s(idx), run.host("zs", zs), len(zs), run.host("r", [r]),
                                                  run.host("t", [t]), run.inp("g", g), run.sfmt, run.flags, run.out("v(t)", 32, dev=False), run.out("pi", 96), AFF))
    check_formats(eng, "kzg_multiopen_coeff_finish", finish, {"v(t)": ("fr", [vt]), "pi": ("is", g1(C.poly_eval(q, TAU)))})


@gpu
def test_multiopen_eval(eng, kit):
    """the same in evaluation form over a domain of 64: claims off the domain and at w^m"""
    from tests import multiopen_model as MO
    d, rng = 64, random.Random(39)
    lag = kit("lag", d)
    V = RL.base(rng, 3 * d)
    vecs = [V[i * d:(i + 1) * d] for i in range(3)]
    zs, idx, r, t = _multiopen_claims(rng, [rng.randrange(R), pow(omega(d), 5, R), 1])
    ys, g = MO.commit_eval(vecs, idx, zs, r)
    _, vt, q = MO.finish_eval(vecs, idx, zs, r, t, g)

    def at_tau(values):
        return g1(C.poly_eval(C.fft(list(values), inverse=True), TAU))

    def commit(run):
        run.ok(eng.lib.kzg_multiopen_eval_commit(eng.ctx, lag.handle, run.inp("evals", V), d, 3, _u32s(idx), run.host("zs", zs), len(zs), run.host("r", [r]),
                                                 run.sfmt, run.flags, run.out("ys", 32 * len(zs), dev=False), run.out("g", 32 * d, dev=run.in_dev),
                                                 run.out("D", 96), AFF))
    check_formats(eng, "kzg_multiopen_eval_commit", commit, {"ys": ("fr", ys), "g": ("fr", g), "D": ("is", at_tau(g))})

    def finish(run):
        run.ok(eng.lib.kzg_multiopen_eval_finish(eng.ctx, lag.handle, run.inp("evals", V), d, 3, _u32s(idx), run.host("zs", zs), len(zs), run.host("r", [r]),
                                                 run.host("t", [t]), run.inp("g", g), run.sfmt, run.flags, run.out("v(t)", 32, dev=False), run.out("pi", 96), AFF))
    check_formats(eng, "kzg_multiopen_eval_finish", finish, {"v(t)": ("fr", [vt]), "pi": ("is", at_tau(q))})


@gpu
def test_verify_multiopen(eng):
    """the proof of tests/multiopen_model.py as discrete logs; honest: 1, one value off by one: 0; zs, ys, r and t travel in sfmt (host only)"""
    from tests import multiopen_model as MO
    n, rng = 12, random.Random(42)
    params = kzg_amd.setup(eng, TAU, 4, g2_len=2)
    try:
        polys = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
        zs, idx, r, t = _multiopen_claims(rng, [rng.randrange(R), 0, R - 1])
        ys, Dk, pik = MO.prove(polys, idx, zs, r, t, TAU)
        assert MO.verdict(TAU, [C.poly_eval(p, TAU) for p in polys], idx, zs, ys, r, t, Dk, pik)
        cm, Dp, pi = b"".join(g1(C.poly_eval(p, TAU)) for p in polys), g1(Dk), g1(pik)
        wrong = list(ys)
        wrong[3] = (wrong[3] + 1) % R

        def call(run):
            for name, vals in (("honest", ys), ("one off", wrong)):
                res = ctypes.c_int(-1)
                run.ok(eng.lib.kzg_verify_multiopen(eng.ctx, params.gs.handle, params.hs.handle, run.host("zs", zs), run.host("ys, " + name, vals), run.sfmt, cm,
                                                    3, _u32s(idx), len(zs), run.host("r", [r]), run.host("t", [t]), Dp, pi, AFF, ctypes.byref(res)))
                run.got[name] = res.value
        check_formats(eng, "kzg_verify_multiopen", call, {"honest": ("is", 1), "one off": ("is", 0)}, (HOST,))
    finally:
        params.gs.free()
        params.hs.free()


@gpu
def test_fr_grand_product(eng):
    """n = 2049 (one element past a tile), t = 2 columns: num, den and z_out on the device in Montgomery form"""
    from tests import fr_scan_model as FM
    n, t, rng = 2049, 2, random.Random(43)
    num, den = RL.base(rng, t * n), [rng.randrange(1, R) for _ in range(t * n)]
    z, total, zero_den = FM.grand_product(num, den, n, t)
    assert not zero_den

    def call(run):
        zd = (ctypes.c_int * 1)(9)
        run.ok(eng.lib.kzg_fr_grand_product(eng.ctx, run.inp("num", num), run.inp("den", den), n, t, 1, run.sfmt, run.flags, run.out("z", 32 * n),
                                            run.out("total", 32, dev=False), zd))
        run.got["zero_den"] = list(zd)
    check_formats(eng, "kzg_fr_grand_product", call, {"z": ("fr", list(z)), "total": ("fr", [total]), "zero_den": ("is", [0])})


@gpu
@pytest.mark.parametrize("form", ["coeff", "eval"])
def test_witness_all(eng, kit, form):
    N = 1 << FK_LOG_N
    V = RL.base(random.Random(20), N)
    plan = kzg_amd.FK20Plan(eng, kit("gs", 4096), FK_LOG_N)
    fn = eng.lib.kzg_witness_all_coeff if form == "coeff" else eng.lib.kzg_witness_all_eval
    E = fk20_points_expect(V if form == "coeff" else C.fft(V, inverse=True), FK_LOG_N)

    def call(run):
        run.ok(fn(eng.ctx, plan.handle, run.inp("input", V), N, 1, run.sfmt, run.flags, run.out("w", 96 * N), AFF))
    try:
        check_formats(eng, "kzg_witness_all_" + form, call, {"w": ("is", E)})
    finally:
        plan.free()


@gpu
@pytest.mark.parametrize("form", ["coeff", "eval"])
def test_witness_cosets(eng, kit, form):
    """out_r, the interpolants, is in sfmt and follows KZG_OUT_DEVICE like the witnesses"""
    N, K = 1 << FK_LOG_N, 1 << (FK_LOG_N - FK_LOG_L)
    V = RL.base(random.Random(21), N)
    plan = kzg_amd.FK20CosetPlan(eng, kit("gs", 4096), FK_LOG_N, FK_LOG_L)
    fn = eng.lib.kzg_witness_cosets_coeff if form == "coeff" else eng.lib.kzg_witness_cosets_eval
    ws, rs = fk20_cosets_expect(V if form == "coeff" else C.fft(V, inverse=True), FK_LOG_N, FK_LOG_L)

    def call(run):
        run.ok(fn(eng.ctx, plan.handle, run.inp("input", V), N, 1, run.sfmt, run.flags, run.out("w", 96 * K), AFF, run.out("r", 32 * N)))
    try:
        check_formats(eng, "kzg_witness_cosets_" + form, call, {"w": ("is", ws), "r": ("fr", unpack(rs))})
    finally:
        plan.free()


@gpu
def test_witness_coeff_tree(eng, kit):
    """n = 300 at a plan of k = 7 points: the bytes of kzg_witness_coeff_batched, so the same oracle; the plan's points are host scalars
    in sfmt, ys (the claimed values) live where the coefficients live, out_r follows KZG_OUT_DEVICE"""
    n, k = 300, 7
    rng = random.Random(7)
    gs = kit("gs", 4096)
    V = RL.base(rng, n)
    xs = [rng.randrange(R) for _ in range(k)]
    ys = [C.poly_eval(V, x) for x in xs]
    w, I = batched_opening(V, xs, ys)

    def call(run):
        plan, st = ctypes.c_void_p(), (ctypes.c_int * 1)(9)
        run.ok(eng.lib.kzg_point_tree_setup(eng.ctx, run.host("xs", xs), k, run.sfmt, ctypes.byref(plan)))
        try:
            run.ok(eng.lib.kzg_witness_coeff_tree(eng.ctx, gs.handle, plan, run.inp("coeffs", V), n, 1, run.inp("ys", ys), run.sfmt, run.flags,
                                                  run.out("w", 96), AFF, run.out("r", 32 * k), st))
        finally:
            eng.lib.kzg_point_tree_free(eng.ctx, plan)
        run.got["status"] = list(st)
    check_formats(eng, "kzg_witness_coeff_tree", call, {"w": ("is", w), "r": ("fr", I), "status": ("is", [0])})


# ---- state: what a context keeps between calls must not carry a format over ------------------------------------------------------------------
@gpu
def test_point_set_cache_keeps_the_formats_apart():
    """witness.hip keeps what depends on the opening points alone per (xs bytes, sfmt, log_N).  The same 256 bytes B are the points X in
    canonical form and the points X * 2^-256 in Montgomery form: (B, canonical), (B, Montgomery), (B, canonical) on a fresh context must
    give the oracle's witness and interpolant each time, the second call must not find the first one's entry, and the third must."""
    n, k = 300, 8
    rng = random.Random(33)
    X = [rng.randrange(R) for _ in range(k)]
    B = RL.pack(X)
    V = RL.base(rng, n)
    points = {CANONICAL: X, MONTGOMERY: [x * pow(M.FR_MONT_R, -1, R) % R for x in X]}
    assert MONTGOMERY.pack(points[MONTGOMERY]) == B
    e = kzg_amd.Engine(0)
    try:
        gs = kzg_amd.setup(e, TAU, 512, g2_len=0).gs

        def stats():
            h, m = ctypes.c_uint64(), ctypes.c_double()
            assert e.lib.kzg_prof_get(e.ctx, b"point_set_cache", ctypes.byref(h), ctypes.byref(m)) == 0
            return h.value, int(m.value)
        failed, seen = [], []
        for step, fmt in enumerate((CANONICAL, MONTGOMERY, CANONICAL)):
            xs = points[fmt]
            ys = [C.poly_eval(V, x) for x in xs]
            w, I = batched_opening(V, xs, ys)
            out, rbuf, rlen = ctypes.create_string_buffer(96), ctypes.create_string_buffer(32 * k), ctypes.c_size_t()
            before = stats()
            rc = e.lib.kzg_witness_coeff_batched(e.ctx, gs.handle, fmt.pack(V), n, B, fmt.pack(ys), k, fmt.sfmt, 0, out, AFF, rbuf, ctypes.byref(rlen))
            after = stats()
            seen.append((after[0] - before[0], after[1] - before[1]))
            if rc != 0:
                failed.append("call %d (%s): status %d (%s)" % (step, fmt.name, rc, e.last_error()))
            elif out.raw != w or rbuf.raw != fmt.pack(I) or rlen.value != k:
                failed.append("call %d (%s): %s" % (step, fmt.name, "the witness differs" if out.raw != w else "the interpolant differs"))
        assert not failed, "; ".join(failed)
        # (the first call of a context finds no cache at all, which is not counted as a miss)
        assert [h for h, _ in seen] == [0, 0, 1] and seen[1][1] == 1, "(hits, misses) per call: %s" % seen
        gs.free()
    finally:
        e.close()


@gpu
def test_alternating_formats_on_one_context(eng, kit):
    """canonical, Montgomery, canonical of kzg_fr_vec_mul, kzg_poly_mul and kzg_msm_g1, back to back on one context (sequential calls
    lease the same lane): a format flag that sticks in the context or in a cached plan shows in one of the nine results"""
    rng = random.Random(34)
    n = 777
    a, b = vec_pair(rng, n)
    pa, pb = RL.base(rng, 300), RL.base(rng, 7)
    V = RL.base(rng, NM)
    gs = kit("gs", 4096)
    E_vec = [x * y % R for x, y in zip(a, b)]
    E_mul = list(M.Polynomial(pa, 299).mul_naive(M.Polynomial(pb, 6)).coeffs[:306])
    E_msm = g1(C.poly_eval(V, TAU))
    failed = []
    for step, fmt in enumerate((CANONICAL, MONTGOMERY, CANONICAL)):
        tag = "call %d (%s)" % (step, fmt.name)
        va = ctypes.create_string_buffer(fmt.pack(a), 32 * n)
        rc = eng.lib.kzg_fr_vec_mul(eng.ctx, va, fmt.pack(b), n, fmt.sfmt, 0)
        if rc != 0 or va.raw != fmt.pack(E_vec):
            failed.append("kzg_fr_vec_mul, " + tag)
        out = ctypes.create_string_buffer(32 * 306)
        rc = eng.lib.kzg_poly_mul(eng.ctx, fmt.pack(pa), 300, fmt.pack(pb), 7, fmt.sfmt, 0, out)
        if rc != 0 or out.raw != fmt.pack(E_mul):
            failed.append("kzg_poly_mul, " + tag)
        pt = ctypes.create_string_buffer(96)
        rc = eng.lib.kzg_msm_g1(eng.ctx, gs.handle, 0, fmt.pack(V), NM, fmt.sfmt, 0, pt, AFF)
        if rc != 0 or pt.raw != E_msm:
            failed.append("kzg_msm_g1, " + tag)
    assert not failed, "; ".join(failed)
