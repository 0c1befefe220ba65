"""
ORACLE (test infrastructure, NOT product code) -- pure-Python restatement of the verifier half of
proxima-one/kzg: G2 arithmetic, the BLS12-381 optimal ate pairing and KZGVerifier / KZGVerifierEvalForm
(src/coeff_form.rs:114-183, src/eval_form.rs:149-218).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package.

PARITY STATUS: "parity unpinned" by the reference -- `pairing()` and the G2 group live in third-party crates
absent from /root/reference (blstrs git rev b98fc83 -> blst; pairing 0.21.0; Cargo.toml:23,27) and no reference
test holds a literal G2 or Gt value; the verifier only ever exposes booleans.  The published definition is
restated (twist y^2 = x^3 + 4(1+u) over Fq2 = Fq[u]/(u^2+1), standard G2 generator, Fq12 = Fq2[w]/(w^6 - (1+u)),
ate loop over |z| = 0xd201000000010000) and pinned by: generator on the twist, r*G2 = infinity, bilinearity
e(aP, bQ) = e(P, Q)^(ab), non-degeneracy, e(P,Q)^r = 1, the final-exponentiation chain against a plain
square-and-multiply with the integer exponent, and the reference's own verifier tests restated with a known tau
(src/coeff_form.rs:198-400, src/eval_form.rs:290-420: honest witnesses verify, wrong values do not).
The value of e(P, Q) itself is fixed only up to the (r-coprime) power 3 used by the final-exponentiation chain;
every boolean the verifier returns is independent of that choice.

G2 points are affine tuples ((x0, x1), (y0, y1)) of ints (x = x0 + x1*u) or None for the identity.
"""
from . import kzg_model as M

Q, R = M.Q, M.R
BLS_Z_ABS = 0xd201000000010000  # the curve parameter z is -BLS_Z_ABS

# --------------------------------------------------------------------------------------
# Fq2 = Fq[u]/(u^2 + 1)
# --------------------------------------------------------------------------------------
F2_ZERO, F2_ONE = (0, 0), (1, 0)
XI = (1, 1)  # the sextic non-residue 1 + u


def f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2_neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_scale(a, k):
    return (a[0] * k % Q, a[1] * k % Q)


def f2_conj(a):
    return (a[0], (-a[1]) % Q)


def f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % Q, Q - 2, Q)
    return (a[0] * n % Q, (-a[1]) * n % Q)


def f2_pow(a, e):
    out = F2_ONE
    while e:
        if e & 1:
            out = f2_mul(out, a)
        a = f2_sqr(a)
        e >>= 1
    return out


def f2_sqrt(a):
    """square root in Fq2 for q = 3 mod 4 (Adj & Rodriguez-Henriquez, alg. 9); None if a is a non-residue"""
    if a == F2_ZERO:
        return F2_ZERO
    a1 = f2_pow(a, (Q - 3) // 4)
    alpha = f2_mul(f2_sqr(a1), a)
    x0 = f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        x = f2_mul((0, 1), x0)
    else:
        b = f2_pow(f2_add(F2_ONE, alpha), (Q - 1) // 2)
        x = f2_mul(b, x0)
    return x if f2_sqr(x) == a else None


# --------------------------------------------------------------------------------------
# G2: y^2 = x^3 + 4(1 + u) over Fq2
# --------------------------------------------------------------------------------------
G2_B = (4, 4)
G2_X = (0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
        0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e)
G2_Y = (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
        0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)
G2 = (G2_X, G2_Y)


def g2_is_on_curve(P):
    if P is None:
        return True
    x, y = P
    return f2_sqr(y) == f2_add(f2_mul(f2_sqr(x), x), G2_B)


def g2_neg(P):
    return None if P is None else (P[0], f2_neg(P[1]))


def g2_add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    (x1, y1), (x2, y2) = P, S
    if x1 == x2:
        if y1 != y2 or y1 == F2_ZERO:
            return None
        lam = f2_mul(f2_scale(f2_sqr(x1), 3), f2_inv(f2_scale(y1, 2)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_sqr(lam), x1), x2)
    return (x3, f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1))


def g2_mul(P, k):
    k %= R
    out = None
    while k:
        if k & 1:
            out = g2_add(out, P)
        P = g2_add(P, P)
        k >>= 1
    return out


def g2_multi_exp(points, scalars):
    """G2Projective::multi_exp (src/coeff_form.rs:156) -- value semantics only"""
    assert len(points) == len(scalars)
    out = None
    for P, k in zip(points, scalars):
        out = g2_add(out, g2_mul(P, k))
    return out


def setup_g2(s, num_coeffs):
    """hs[i] = hs[i-1] * s  (src/lib.rs:48-52)"""
    out, acc = [], 1
    for _ in range(num_coeffs):
        out.append(g2_mul(G2, acc))
        acc = acc * s % R
    return out


# zcash serialisation of G2: x = c1 || c0 big-endian 48 B each; flag bits as for G1
def _f2_lex_largest(y):
    ny = f2_neg(y)
    return (y[1], y[0]) > (ny[1], ny[0])


def g2_to_uncompressed(P):
    if P is None:
        return bytes([0x40]) + bytes(191)
    (x0, x1), (y0, y1) = P
    return b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))


def g2_from_uncompressed(b):
    """strict (oracle/decode.py), on-curve level: the tests parse the engine's own outputs with it"""
    from . import decode
    return decode.decode_point("g2", decode.UNCOMPRESSED, b, decode.ON_CURVE)


def g2_to_compressed(P):
    if P is None:
        return bytes([0xC0]) + bytes(95)
    (x0, x1), y = P
    out = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if _f2_lex_largest(y) else 0)
    return bytes(out)


def g2_from_compressed(b):
    """strict (oracle/decode.py), on-curve level"""
    from . import decode
    return decode.decode_point("g2", decode.COMPRESSED, b, decode.ON_CURVE)


def g2_to_affine_mont(P):
    """blst_p2_affine: x.c0, x.c1, y.c0, y.c1 as 6 x u64 little-endian Montgomery limbs; identity all zero"""
    if P is None:
        return bytes(192)
    (x0, x1), (y0, y1) = P
    return b"".join((v * M.FQ_MONT_R % Q).to_bytes(48, "little") for v in (x0, x1, y0, y1))


def g2_to_jacobian_mont(P):
    """blst_p2: (X, Y, Z) Jacobian, identity Z = 0"""
    if P is None:
        return bytes(288)
    return g2_to_affine_mont(P) + (M.FQ_MONT_R % Q).to_bytes(48, "little") + bytes(48)


# --------------------------------------------------------------------------------------
# Fq12 = Fq2[w]/(w^6 - xi): elements are 6-tuples of Fq2 coefficients of w^0..w^5
# (tower view: Fq6 = Fq2[v]/(v^3 - xi) with v = w^2, Fq12 = Fq6[w]/(w^2 - v))
# --------------------------------------------------------------------------------------
F12_ONE = (F2_ONE,) + (F2_ZERO,) * 5


def f12_mul(a, b):
    acc = [F2_ZERO] * 11
    for i in range(6):
        if a[i] == F2_ZERO:
            continue
        for j in range(6):
            acc[i + j] = f2_add(acc[i + j], f2_mul(a[i], b[j]))
    for k in range(10, 5, -1):
        acc[k - 6] = f2_add(acc[k - 6], f2_mul(acc[k], XI))
    return tuple(acc[:6])


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    """a^(q^6): w -> -w"""
    return tuple(c if i % 2 == 0 else f2_neg(c) for i, c in enumerate(a))


# Frobenius: (sum b_k w^k)^q = sum conj(b_k) * xi^(k(q-1)/6) * w^k
FROB1 = tuple(f2_pow(XI, k * (Q - 1) // 6) for k in range(6))
FROB2 = tuple(f2_pow(XI, k * (Q * Q - 1) // 6) for k in range(6))


def f12_frob(a):
    return tuple(f2_mul(f2_conj(c), FROB1[k]) for k, c in enumerate(a))


def f12_frob2(a):
    return tuple(f2_mul(c, FROB2[k]) for k, c in enumerate(a))


def f12_pow(a, e):
    out = F12_ONE
    while e:
        if e & 1:
            out = f12_mul(out, a)
        a = f12_sqr(a)
        e >>= 1
    return out


def _f6_from12(a):
    return (a[0], a[2], a[4]), (a[1], a[3], a[5])


def _f6_mul(a, b):
    t = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    return (f2_add(t[0], f2_mul(t[3], XI)), f2_add(t[1], f2_mul(t[4], XI)), t[2])


def _f6_inv(a):
    a0, a1, a2 = a
    c0 = f2_sub(f2_sqr(a0), f2_mul(XI, f2_mul(a1, a2)))
    c1 = f2_sub(f2_mul(XI, f2_sqr(a2)), f2_mul(a0, a1))
    c2 = f2_sub(f2_sqr(a1), f2_mul(a0, a2))
    t = f2_add(f2_mul(a0, c0), f2_mul(XI, f2_add(f2_mul(a2, c1), f2_mul(a1, c2))))
    ti = f2_inv(t)
    return (f2_mul(c0, ti), f2_mul(c1, ti), f2_mul(c2, ti))


def f12_inv(a):
    c0, c1 = _f6_from12(a)  # a = c0 + c1 w, w^2 = v
    c1sq = _f6_mul(c1, c1)
    v_c1sq = (f2_mul(c1sq[2], XI), c1sq[0], c1sq[1])  # times v
    c0sq = _f6_mul(c0, c0)
    t = _f6_inv(tuple(f2_sub(x, y) for x, y in zip(c0sq, v_c1sq)))
    r0 = _f6_mul(c0, t)
    r1 = tuple(f2_neg(x) for x in _f6_mul(c1, t))
    return (r0[0], r1[0], r0[1], r1[1], r0[2], r1[2])


# --------------------------------------------------------------------------------------
# optimal ate pairing
# --------------------------------------------------------------------------------------
def _line(lam, T, P):
    """The line of slope lam (on the twist) through T, evaluated at P in G1 and scaled by w^3 (an element of a
    proper subfield, annihilated by the final exponentiation):  yP*w^3 - lam*xP*w^2 + (lam*xT - yT)."""
    xP, yP = P
    return (f2_sub(f2_mul(lam, T[0]), T[1]), F2_ZERO, f2_neg(f2_scale(lam, xP)), (yP, 0), F2_ZERO, F2_ZERO)


def miller_loop(pairs):
    """prod_i f_{z,Q_i}(P_i) for (P_i in G1, Q_i in G2); pairs with an identity member contribute 1"""
    pairs = [(P, S) for P, S in pairs if P is not None and S is not None]
    f = F12_ONE
    Ts = [S for _, S in pairs]
    for bit in bin(BLS_Z_ABS)[3:]:
        f = f12_sqr(f)
        for i, (P, S) in enumerate(pairs):
            T = Ts[i]
            lam = f2_mul(f2_scale(f2_sqr(T[0]), 3), f2_inv(f2_scale(T[1], 2)))
            f = f12_mul(f, _line(lam, T, P))
            x3 = f2_sub(f2_sqr(lam), f2_scale(T[0], 2))
            Ts[i] = T = (x3, f2_sub(f2_mul(lam, f2_sub(T[0], x3)), T[1]))
            if bit == "1":
                lam = f2_mul(f2_sub(S[1], T[1]), f2_inv(f2_sub(S[0], T[0])))
                f = f12_mul(f, _line(lam, T, P))
                x3 = f2_sub(f2_sub(f2_sqr(lam), T[0]), S[0])
                Ts[i] = (x3, f2_sub(f2_mul(lam, f2_sub(T[0], x3)), T[1]))
    return f12_conj(f)  # z < 0


HARD_EXP_TIMES_3 = 3 * ((Q ** 4 - Q ** 2 + 1) // R)
assert (Q ** 4 - Q ** 2 + 1) % R == 0
_z = -BLS_Z_ABS
assert (_z - 1) ** 2 * (_z + Q) * (_z * _z + Q * Q - 1) + 3 == HARD_EXP_TIMES_3  # Hayashida-Hayasaka-Teruya


def f12_cyclotomic_sqr(a):
    """a^2 for a in the cyclotomic subgroup (Granger-Scott: three Fq4 squarings, 6 Fq2 products instead of 12)"""
    nr = lambda x: f2_mul(x, XI)  # noqa: E731
    dbl = lambda x: f2_add(x, x)  # noqa: E731
    r0, r4, r3 = a[0], a[2], a[4]  # c0 = (a0, a2, a4), c1 = (a1, a3, a5) in the tower view
    r2, r1, r5 = a[1], a[3], a[5]

    def fq4_sqr(x, y):
        t = f2_mul(x, y)
        return f2_sub(f2_sub(f2_mul(f2_add(x, y), f2_add(nr(y), x)), t), nr(t)), dbl(t)

    t0, t1 = fq4_sqr(r0, r1)
    t2, t3 = fq4_sqr(r2, r3)
    t4, t5 = fq4_sqr(r4, r5)
    z0 = f2_add(dbl(f2_sub(t0, r0)), t0)
    z1 = f2_add(dbl(f2_add(t1, r1)), t1)
    t = nr(t5)
    z2 = f2_add(dbl(f2_add(t, r2)), t)
    z3 = f2_add(dbl(f2_sub(t4, r3)), t4)
    z4 = f2_add(dbl(f2_sub(t2, r4)), t2)
    z5 = f2_add(dbl(f2_add(t3, r5)), t3)
    return (z0, z2, z4, z1, z3, z5)


def _exp_z(a):
    """a^z for a in the cyclotomic subgroup (inverse = conjugate)"""
    return f12_conj(f12_pow(a, BLS_Z_ABS))


def final_exponentiation(f):
    """f^(3 (q^12 - 1)/r)"""
    f1 = f12_mul(f12_conj(f), f12_inv(f))        # ^(q^6 - 1)
    f2 = f12_mul(f12_frob2(f1), f1)              # ^(q^2 + 1)
    a = f12_mul(_exp_z(f2), f12_conj(f2))        # ^(z - 1)
    a = f12_mul(_exp_z(a), f12_conj(a))          # ^(z - 1)
    b = f12_mul(_exp_z(a), f12_frob(a))          # ^(z + q)
    c = f12_mul(f12_mul(_exp_z(_exp_z(b)), f12_frob2(b)), f12_conj(b))  # ^(z^2 + q^2 - 1)
    return f12_mul(c, f12_mul(f12_sqr(f2), f2))


def final_exponentiation_naive(f):
    return f12_pow(f, 3 * ((Q ** 12 - 1) // R))


def pairing(P, S):
    """pairing(&G1Affine, &G2Affine) -> Gt (external; call sites src/coeff_form.rs:133-141)"""
    return final_exponentiation(miller_loop([(P, S)]))


def pairing_product_is_one(pairs):
    return final_exponentiation(miller_loop(pairs)) == F12_ONE


# --------------------------------------------------------------------------------------
# the reference's verifiers
# --------------------------------------------------------------------------------------
class KZGParamsG2:  # the hs half of KZGParams (src/lib.rs:14-19)
    def __init__(self, gs, hs):
        self.gs, self.hs = gs, hs


def setup(s, num_coeffs, fast=True):
    """setup (src/lib.rs:38-55), both halves"""
    gs = M.setup_g1_fast(s, num_coeffs) if fast else M.setup_g1(s, num_coeffs)
    return KZGParamsG2(gs, setup_g2(s, num_coeffs))


class KZGVerifier:  # src/coeff_form.rs:114-183
    def __init__(self, parameters):
        self.parameters = parameters

    def verify_poly(self, commitment, polynomial):  # :119-124
        gs = self.parameters.gs[:polynomial.num_coeffs()]
        return M.g1_multi_exp(gs, polynomial.slice_coeffs()) == commitment

    def verify_eval(self, point, commitment, witness):  # :126-142  lhs == rhs
        x, y = point
        p = self.parameters
        h = g2_add(p.hs[1], g2_neg(g2_mul(p.hs[0], x)))
        a = M.g1_add(commitment, M.g1_neg(M.g1_mul(p.gs[0], y)))
        return pairing(witness, h) == pairing(a, p.hs[0])

    def verify_eval_batched(self, xs, commitment, witness_w, witness_r):  # :144-182
        z = M.op_tree(len(xs), lambda i: M.Polynomial.new_from_coeffs([M.fr_neg(xs[i]), 1], 1), lambda a, b: a.best_mul(b))
        p = self.parameters
        if z.num_coeffs() == 1:
            hz = g2_mul(p.hs[0], z.coeffs[0])
        else:
            hz = g2_multi_exp(p.hs[:z.num_coeffs()], z.slice_coeffs())
        if witness_r.num_coeffs() == 1:
            gr = M.g1_mul(p.gs[0], witness_r.coeffs[0])
        else:
            gr = M.g1_multi_exp(p.gs[:witness_r.num_coeffs()], witness_r.slice_coeffs())
        a = M.g1_add(commitment, M.g1_neg(gr))
        return pairing(witness_w, hz) == pairing(a, p.hs[0])


class KZGVerifierEvalForm:  # src/eval_form.rs:149-218
    def __init__(self, parameters, lagrange_basis_g, lagrange_basis_h):
        self.parameters = parameters
        self.d, self.exp, self.omega = M.compute_omega(len(parameters.gs))
        self.lagrange_basis_g, self.lagrange_basis_h = lagrange_basis_g, lagrange_basis_h

    def verify_eval(self, point, commitment, witness):  # :173-190
        i, y = point
        omega = pow(M.FR_ROOT_OF_UNITY, 1 << (M.FR_S - self.exp), R)
        return KZGVerifier(self.parameters).verify_eval((pow(omega, i, R), y), commitment, witness)

    def verify_eval_all(self, ys, commitment, witness):  # :192-217 (z.coeffs[0] = -1, z.coeffs[d-1] = 1 as written)
        hz = g2_add(g2_neg(self.lagrange_basis_h[0]), self.lagrange_basis_h[self.d - 1]) if self.d > 1 else None
        if self.d == 1:  # both writes hit index 0; the later one (1) wins
            hz = self.lagrange_basis_h[0]
        gr = M.g1_multi_exp(self.lagrange_basis_g[:len(ys)], list(ys))
        a = M.g1_add(commitment, M.g1_neg(gr))
        return pairing(witness, hz) == pairing(a, self.parameters.hs[0])


def lagrange_basis_g2_known_tau(tau, d):
    """[L_i(tau)] H with the closed form used for the G1 basis (kzg_model.lagrange_basis_g1_known_tau)"""
    _, exp, omega = M.compute_omega(d)
    num = (pow(tau, d, R) - 1) * M.fr_inv(d) % R
    out = []
    for i in range(d):
        wi = pow(omega, i, R)
        if (tau - wi) % R == 0:
            out.append(G2 if True else None)
            continue
        out.append(g2_mul(G2, num * wi % R * M.fr_inv(tau - wi) % R))
    return out


def selfcheck(full=False):
    assert g2_is_on_curve(G2) and g2_mul(G2, R - 1) == g2_neg(G2) and g2_add(g2_mul(G2, R - 1), G2) is None
    assert g2_from_compressed(g2_to_compressed(G2)) == G2 and g2_from_uncompressed(g2_to_uncompressed(G2)) == G2
    e = pairing(M.G1, G2)
    assert e != F12_ONE and f12_pow(e, R) == F12_ONE
    a, b = 0x1234567, 0xabcdef01
    assert pairing(M.g1_mul(M.G1, a), g2_mul(G2, b)) == f12_pow(e, a * b % R)
    assert f12_mul(e, f12_inv(e)) == F12_ONE
    if full:
        f = miller_loop([(M.G1, G2)])
        assert final_exponentiation(f) == final_exponentiation_naive(f)
        assert f12_cyclotomic_sqr(e) == f12_sqr(e)
    return True
