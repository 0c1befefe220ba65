"""
ORACLE (test infrastructure, NOT product code) -- the strict reference decoder of the eight point formats of
include/kzg_mi355x.h, written from the published zcash / blst serialisation rules (the ones G1Affine / G2Affine
::from_compressed / from_uncompressed apply upstream) and from the header's format table, not from the HIP kernels.

    decode_point(group, fmt, data, level) -> point | None (the identity); raises BadPoint

group "g1" / "g2"; fmt AFFINE_MONT / JACOBIAN_MONT / UNCOMPRESSED / COMPRESSED (the numbering both KZG_G1_* and KZG_G2_* use);
level 0 trusted, 1 on the curve, 2 + in the r-torsion subgroup (common.h).  Points are kzg_model / pairing_model values.

  compressed     bit 7 set.  Bit 6 (infinity): bit 5 clear and every other bit zero -> identity.  Otherwise x = the remaining
                 381 bits (G2: c1 || c0), every component < q, y^2 = x^3 + b has a root, y is the lexicographically larger
                 root exactly when bit 5 is set.
  uncompressed   bit 7 clear.  Bit 6: everything else, bit 5 included, zero -> identity.  Otherwise bit 5 clear, every
                 coordinate < q, (x, y) satisfies the curve equation -- all-zero bytes are (0, 0), which does not.
  affine Mont    every limb vector < q; all-zero is the identity; everything else goes through the curve equation.
  Jacobian Mont  X, Y, Z < q (also when Z = 0); Z = 0 is the identity; otherwise Y^2 = X^3 + b Z^6.
  level 2        [r]P = O by plain double-and-add (g1_mul / g2_mul reduce their scalar mod r).
  level 0        the Montgomery formats are taken as they are (limbs mod q, no curve equation): the engine's own results.  The
                 wire formats have no trusted reading -- a decoder cannot skip the flags or the square root -- so level 0 is
                 level 1 there.

Each accepted WIRE encoding is the only encoding of its point: encode_point(decode_point(b)) == b (tests/test_decode_corpus.py).
"""
import functools

from . import kzg_model as M
from . import pairing_model as PM

Q, R = M.Q, M.R
AFFINE_MONT, JACOBIAN_MONT, UNCOMPRESSED, COMPRESSED = 0, 1, 2, 3
FORMATS = (AFFINE_MONT, JACOBIAN_MONT, UNCOMPRESSED, COMPRESSED)
WIRE_FORMATS = (UNCOMPRESSED, COMPRESSED)
TRUSTED, ON_CURVE, SUBGROUP = 0, 1, 2
MONT_R_INV = pow(M.FQ_MONT_R, Q - 2, Q)


class BadPoint(ValueError):
    pass


def point_bytes(group, fmt):
    return {AFFINE_MONT: 96, JACOBIAN_MONT: 144, UNCOMPRESSED: 96, COMPRESSED: 48}[fmt] * (1 if group == "g1" else 2)


# ---- the two coordinate fields behind one face: elements are tuples of `deg` integers (c0[, c1]) ---------------------------
class _Fq:
    deg = 1
    b = (4,)

    @staticmethod
    def mul(a, b):
        return (a[0] * b[0] % Q,)

    @staticmethod
    def add(a, b):
        return ((a[0] + b[0]) % Q,)

    @staticmethod
    def neg(a):
        return ((-a[0]) % Q,)

    @staticmethod
    def inv(a):
        return (pow(a[0], Q - 2, Q),)

    @staticmethod
    def sqrt(a):
        y = pow(a[0], (Q + 1) // 4, Q)
        return (y,) if y * y % Q == a[0] else None

    @staticmethod
    def lex_largest(y):  # y > -y as integers in [0, q)
        return y[0] > (Q - 1) // 2


class _Fq2:
    deg = 2
    b = (4, 4)
    mul = staticmethod(PM.f2_mul)
    add = staticmethod(PM.f2_add)
    neg = staticmethod(PM.f2_neg)
    inv = staticmethod(PM.f2_inv)
    sqrt = staticmethod(PM.f2_sqrt)

    @staticmethod
    def lex_largest(y):  # (c1, c0) against the negation's; c0 decides when c1 = 0
        if y[1] != 0:
            return y[1] > (Q - 1) // 2
        return y[0] > (Q - 1) // 2


def _field(group):
    if group == "g1":
        return _Fq
    if group == "g2":
        return _Fq2
    raise ValueError("group is 'g1' or 'g2'")


def _point(F, x, y):
    return (x[0], y[0]) if F.deg == 1 else (x, y)


def _curve_rhs(F, x):
    return F.add(F.mul(F.mul(x, x), x), F.b)


@functools.lru_cache(maxsize=None)
def in_subgroup(group, P):
    """[r]P == O with plain additions"""
    add = M.g1_add if group == "g1" else PM.g2_add
    acc, base, k = None, P, R
    while k:
        if k & 1:
            acc = add(acc, base)
        base = add(base, base)
        k >>= 1
    return acc is None


def _wire_element(F, chunk_ints):
    """big-endian components as they are on the wire (G2: c1 first) -> element; every component < q"""
    if any(v >= Q for v in chunk_ints):
        raise BadPoint("coordinate >= q")
    return tuple(reversed(chunk_ints))


def _decode_wire(F, fmt, data):
    flags = data[0] >> 5
    compressed, infinity, sign = bool(flags & 4), bool(flags & 2), bool(flags & 1)
    if compressed != (fmt == COMPRESSED):
        raise BadPoint("compression flag does not match the format")
    body = bytes([data[0] & 0x1F]) + data[1:]
    if infinity:
        if sign or any(body):
            raise BadPoint("infinity flag with a sign flag or a payload")
        return None
    if fmt == UNCOMPRESSED and sign:
        raise BadPoint("sign flag on an uncompressed point")
    ints = [int.from_bytes(body[k:k + 48], "big") for k in range(0, len(body), 48)]
    x = _wire_element(F, ints[:F.deg])
    if fmt == UNCOMPRESSED:
        y = _wire_element(F, ints[F.deg:])
        if F.mul(y, y) != _curve_rhs(F, x):
            raise BadPoint("not on the curve")
        return x, y
    y = F.sqrt(_curve_rhs(F, x))
    if y is None:
        raise BadPoint("x^3 + b is not a square")
    if F.lex_largest(y) != sign:
        y = F.neg(y)
    return x, y


def _decode_mont(F, fmt, data, level):
    limbs = [int.from_bytes(data[k:k + 48], "little") for k in range(0, len(data), 48)]
    if level >= ON_CURVE and any(v >= Q for v in limbs):
        raise BadPoint("Montgomery limbs >= q")
    vals = [v * MONT_R_INV % Q for v in limbs]
    zero = (0,) * F.deg
    x, y = tuple(vals[:F.deg]), tuple(vals[F.deg:2 * F.deg])
    if fmt == AFFINE_MONT:
        if x == zero and y == zero:
            return None
        if level >= ON_CURVE and F.mul(y, y) != _curve_rhs(F, x):
            raise BadPoint("not on the curve")
        return x, y
    z = tuple(vals[2 * F.deg:])
    if z == zero:
        return None
    z2 = F.mul(z, z)
    z3 = F.mul(z2, z)
    if level >= ON_CURVE and F.mul(y, y) != F.add(F.mul(F.mul(x, x), x), F.mul(F.b, F.mul(z3, z3))):
        raise BadPoint("not on the curve")
    return F.mul(x, F.inv(z2)), F.mul(y, F.inv(z3))


def decode_point(group, fmt, data, level=SUBGROUP):
    F = _field(group)
    data = bytes(data)
    if fmt not in FORMATS or len(data) != point_bytes(group, fmt):
        raise ValueError("format / length")
    xy = _decode_wire(F, fmt, data) if fmt in WIRE_FORMATS else _decode_mont(F, fmt, data, level)
    if xy is None:
        return None
    P = _point(F, *xy)
    if level >= SUBGROUP and not in_subgroup(group, P):
        raise BadPoint("not in the r-torsion subgroup")
    return P


_ENCODERS = {
    "g1": {AFFINE_MONT: M.g1_to_affine_mont, JACOBIAN_MONT: M.g1_to_jacobian_mont, UNCOMPRESSED: M.g1_to_uncompressed,
           COMPRESSED: M.g1_to_compressed},
    "g2": {AFFINE_MONT: PM.g2_to_affine_mont, JACOBIAN_MONT: PM.g2_to_jacobian_mont, UNCOMPRESSED: PM.g2_to_uncompressed,
           COMPRESSED: PM.g2_to_compressed},
}


def encode_point(group, fmt, P):
    """the canonical encoding (Jacobian: Z = 1), by the encoders of kzg_model / pairing_model"""
    return _ENCODERS[group][fmt](P)
