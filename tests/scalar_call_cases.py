"""What tests/test_gpu_scalar_residues.py and tests/test_gpu_scalar_formats.py share: the base inputs V (every value < r) of the
scalar-taking calls, their expected results through the oracle, and the module-scoped fixtures both files build on.  The two files
walk the same table of calls along two axes (other representatives of the residues; the other scalar format and the placement flags),
so shapes and seeds are said once, here.  The fixtures are imported by name, which makes them fixtures of the importing module; `kit`
takes the importing module's own `eng` (tests/fk20_common.py)."""
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests import residue_lift as RL

R = M.R
CAN = L.FR_CANONICAL
MONT = L.FR_MONT
AFF = L.G1_AFFINE_MONT
TAU = 0x0123456789ABCDEF0FEDCBA987654321


def le(v):
    return int(v).to_bytes(32, "little")


def g1(k):
    return C.g1_mul(C.g1_generator(), k % R)


def omega(d):
    return M.compute_omega(d)[2]


def ok(e, rc):
    assert rc == 0, (rc, e.last_error())


@pytest.fixture(scope="module")
def kit(eng):
    """the SRSs the module shares, built on first use: kit("gs", n) = setup(TAU, n).gs, kit("lag", d) = the Lagrange SRS, kit("hs", n)"""
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            if kind == "gs":
                cache[kind, n] = kzg_amd.setup(eng, TAU, n, g2_len=0).gs
            elif kind == "lag":
                cache[kind, n] = kzg_amd.setup_lagrange(eng, TAU, n)
            else:
                cache[kind, n] = kzg_amd.setup_g2(eng, TAU, n)
        return cache[kind, n]
    yield get
    for s in cache.values():
        s.free()


# ---- element-wise vector operations -----------------------------------------------------------------------------------------------
def vec_pair(rng, n):
    """a, b with a mod r below, above and equal to b mod r at lifted and at untouched positions alike"""
    a = RL.base(rng, n)
    b = RL.base(rng, n)
    for i in range(n):
        if i % 3 == 0:
            b[i] = a[i]                     # equal residues: the difference is 0, never the word r
        elif i % 3 == 1 and a[i] > b[i]:
            a[i], b[i] = b[i], a[i]         # a < b: the subtraction borrows
    return a, b


def coset_scale(vals, g):
    out, pw = [], 1
    for v in vals:
        out.append(v * pw % R)
        pw = pw * g % R
    return out


# ---- evaluation form on the domain: k_eval_quotient -------------------------------------------------------------------------------
D = 1024
# 0 and 7 are lifted by every mode / by "sparse"; 1 by "all" and "edges" only; D - 1 by "all" only: evals[m] itself is >= r or not
M_INDICES = (0, 1, 7, D - 1)
# evaluation form at any point: one z off the domain and one z = w^m
Z_OFF = 0x1F2E3D4C5B6A79881726354453627180AABBCCDDEEFF00112233445566778899 % R
M_ON = 7                                   # evals[7] is lifted by "sparse" and "all"


@pytest.fixture(scope="module")
def evals():
    """V (D values), its coefficients, p(TAU): computed once"""
    V = RL.base(random.Random(3), D)
    coeffs = C.fft(V, inverse=True)
    assert C.fft(coeffs) == V
    return V, coeffs, C.poly_eval(coeffs, TAU)


def quotient_on_domain(V, m):
    """the oracle's div_by_omega_i, which takes the numerator evals - evals[m]"""
    return C.div_by_omega_i_bytes(RL.pack([(v - V[m]) % R for v in V]), len(V), m)


def witness_at(evals, z, y):
    """the known-tau identity of the eval-form tests: [(p(tau) - y) / (tau - z)]G"""
    return g1((evals[2] - y) * pow(TAU - z, -1, R))


# ---- coefficient form: the Horner scan (one coefficient past a block of 2048) -----------------------------------------------------
NC = 2049


@pytest.fixture(scope="module")
def poly():
    """V (NC coefficients), an opening point, p(x), p(TAU)"""
    rng = random.Random(5)
    V = RL.base(rng, NC)
    x = rng.randrange(R)
    return V, x, C.poly_eval(V, x), C.poly_eval(V, TAU)


def batched_opening(V, xs, ys):
    """create_witness_batched through the python model: ([(p - I)/Z]_1, the coefficients of I = the interpolant through (xs, ys))"""
    I = M.Polynomial.lagrange_interpolation_with_tree(xs, ys, M.SubProductTree.new_from_points(xs))
    Z = 1
    for v in xs:
        Z = Z * (TAU - v) % R
    return g1((C.poly_eval(V, TAU) - I.eval(TAU)) * pow(Z, -1, R)), list(I.coeffs[:len(xs)])


# ---- commitments and MSMs at 2^12 -------------------------------------------------------------------------------------------------
NM = 1 << 12


# ---- FK20: every opening over the domain, points and cosets (the smallest plans of their own files) ---------------------------------
FK_LOG_N, FK_LOG_L = 4, 2


def fk20_points_expect(coeffs, log_n):
    """witness m = [(p(tau) - p(w^m)) / (tau - w^m)]G"""
    N, w, ptau = 1 << log_n, omega(1 << log_n), C.poly_eval(coeffs, TAU)
    return b"".join(g1((ptau - C.poly_eval(coeffs, pow(w, m, R))) * pow(TAU - pow(w, m, R), -1, R)) for m in range(N))


def fk20_cosets_expect(coeffs, log_n, log_l):
    """coset i: r = p mod (X^l - w^(il)) (its l coefficients), witness = [(p(tau) - r(tau)) / (tau^l - w^(il))]G"""
    N, l = 1 << log_n, 1 << log_l
    w, ptau = omega(N), C.poly_eval(coeffs, TAU)
    ws, rs = [], []
    for i in range(N // l):
        c = pow(w, i * l, R)
        r = [sum(coeffs[j + k * l] * pow(c, k, R) for k in range((len(coeffs) - j + l - 1) // l)) % R for j in range(l)]
        ws.append(g1((ptau - C.poly_eval(r, TAU)) * pow(pow(TAU, l, R) - c, -1, R)))
        rs += r
    return b"".join(ws), RL.pack(rs)


# ---- the device group (one GPU, no collective needed) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def group():
    g = kzg_amd.DeviceGroup([0])
    yield g
    g.close()


def group_call(group, fn, blob, dev):
    """fn(argument) with the polynomial as a host blob, or resident on the group's one GPU"""
    if not dev:
        return fn(blob)
    buf = group.engine(0).alloc_scalars(len(blob) // 32).upload(blob)
    try:
        return fn([buf])
    finally:
        buf.free()
