"""The corpus of point encodings shared by tests/test_decode_corpus.py (the strict reference decoder, no GPU) and
tests/test_gpu_decode.py (k_decode_points and k_g2_decode through the C ABI).

corpus() -> [Entry(group, fmt, data, cls, point, name)]

`cls` is written by hand next to each construction, from the rules in oracle/decode.py's docstring and from number theory stated in
the comment beside it -- never from running a decoder:

    ok               accepted at the on-curve level and at the subgroup level; `point` is what it decodes to (None: the identity)
    ok-oncurve-only  on the curve, outside the r-torsion subgroup: accepted at level 1 (option trusted_points), refused at level 2
    bad-flags        a flag bit that must be clear is set, or the infinity flag comes with a payload
    bad-range        a coordinate or a limb vector is >= q
    bad-curve        coordinates in range that do not satisfy the curve equation
    bad-sqrt         compressed: x in range, x^3 + b is not a square

`point` of an accepted entry is built from the group law (multiples of the generators) or from a square root taken here, with the
larger root chosen by comparing tuples of integers -- the encoders of kzg_model / pairing_model only turn it into honest bytes."""
import collections
import functools
import random

from oracle import kzg_model as M
from oracle import pairing_model as PM
from oracle.decode import AFFINE_MONT, JACOBIAN_MONT, UNCOMPRESSED, COMPRESSED, encode_point, point_bytes

Q, R = M.Q, M.R
HALF = (Q - 1) // 2
Entry = collections.namedtuple("Entry", "group fmt data cls point name")
FMT_NAMES = {AFFINE_MONT: "affine_mont", JACOBIAN_MONT: "jacobian_mont", UNCOMPRESSED: "uncompressed", COMPRESSED: "compressed"}
GROUPS = ("g1", "g2")
FORMATS = (AFFINE_MONT, JACOBIAN_MONT, UNCOMPRESSED, COMPRESSED)
OK_CLASSES = ("ok", "ok-oncurve-only")
BAD_CLASSES = ("bad-flags", "bad-range", "bad-curve", "bad-sqrt")


def accepted(cls, level):
    """the hand label's verdict at a validation level (1 on the curve, 2 subgroup)"""
    assert cls in OK_CLASSES + BAD_CLASSES
    return cls == "ok" or (cls == "ok-oncurve-only" and level < 2)


# ---- integers, field elements, bytes ---------------------------------------------------------------------------------------------
def is_qr(v):
    return pow(v % Q, HALF, Q) == 1


def f2_is_square(a):
    """a != 0 in Fq2 is a square exactly when its norm a0^2 + a1^2 is a square in Fq"""
    return is_qr(a[0] * a[0] + a[1] * a[1])


def be(v):
    return v.to_bytes(48, "big")


def mont(v):
    """a limb vector: Montgomery form, little-endian; `v` is reduced first, so mont(v) is always canonical"""
    return (v % Q * M.FQ_MONT_R % Q).to_bytes(48, "little")


def le(v):
    return v.to_bytes(48, "little")


def comps(group, P):
    """the coordinates as integers in the order of the zcash formats: x, y (G1) or x.c1, x.c0, y.c1, y.c0 (G2)"""
    if group == "g1":
        return [P[0], P[1]]
    (x0, x1), (y0, y1) = P
    return [x1, x0, y1, y0]


def limbs(group, P):
    """the coordinates in the order of the Montgomery formats: x, y (G1) or x.c0, x.c1, y.c0, y.c1 (G2)"""
    return [P[0], P[1]] if group == "g1" else [P[0][0], P[0][1], P[1][0], P[1][1]]


def neg(group, P):
    return M.g1_neg(P) if group == "g1" else PM.g2_neg(P)


def with_flags(data, top3):
    return bytes([(data[0] & 0x1F) | (top3 << 5)]) + data[1:]


def set_byte(data, offset, value):
    return data[:offset] + bytes([value]) + data[offset + 1:]


def y_is_larger(group, P):
    """is y the lexicographically larger of (y, -y)?  G1: as integers; G2: (c1, c0) as tuples of integers"""
    if group == "g1":
        return P[1] > Q - P[1]
    y, ny = P[1], PM.f2_neg(P[1])
    return (y[1], y[0]) > (ny[1], ny[0])


# ---- base points -------------------------------------------------------------------------------------------------------------------
def times_r_is_identity(group, P):
    """[r]P == O with plain additions (g1_mul / g2_mul reduce their scalar mod r), as tests/test_gpu_validation.py does"""
    add = M.g1_add if group == "g1" else PM.g2_add
    acc, base, k = None, P, R
    while k:
        if k & 1:
            acc = add(acc, base)
        base = add(base, base)
        k >>= 1
    return acc is None


def _first_outside_subgroup(group, candidates):
    for P in candidates:
        if P is not None and not times_r_is_identity(group, P):
            return P
    raise AssertionError("no point outside the subgroup")


def _g1_at(x):
    rhs = (x * x * x + 4) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    return (x, y) if y * y % Q == rhs else None


def _g2_at(x):
    y = PM.f2_sqrt(PM.f2_add(PM.f2_mul(PM.f2_sqr(x), x), (4, 4)))
    return (x, y) if y is not None else None


@functools.lru_cache(maxsize=None)
def base_points():
    """{group: {"sub": [(name, P)], "curve": [(name, P)]}}: points of the subgroup, and curve points outside it"""
    ks = (1, 2, 3, 5, 0x1234567890ABCDEF1234567890ABCDEF, R - 0xFEDCBA9876543210)
    g1 = [("%dG" % i, M.g1_mul(M.G1, k)) for i, k in enumerate(ks)]
    g2 = [("%dH" % i, PM.g2_mul(PM.G2, k)) for i, k in enumerate(ks)]
    for group, pts in (("g1", g1), ("g2", g2)):       # both y signs occur among the multiples
        assert {y_is_larger(group, P) for _, P in pts} == {True, False}
    # the points tests/test_gpu_validation.py builds: the first x >= 5 (G1) / (3 + k, 1) (G2) with a point outside the subgroup
    T1 = _first_outside_subgroup("g1", (_g1_at(x) for x in range(5, 50)))
    T2 = _first_outside_subgroup("g2", (_g2_at((x, 1)) for x in range(3, 50)))
    # x = 4: 4^3 + 4 = 68 is a square, and 4 + q < 2^381 -- the alias x + q fits under the flag bits
    S1 = _g1_at(4)
    assert S1 is not None and 4 + Q < 1 << 381
    # (0, 2): 2^2 = 0 + 4.  A point of order 3, so outside the subgroup of order r
    Z1 = (0, 2)
    # twist points with x^3 + 4(1+u) in Fq: for x = a + b u the u-part 3 a^2 b - b^3 + 4 vanishes when a^2 = (b^3 - 4) / (3 b)
    special = []
    for b, tag in ((2, "imag"), (19, "real")):
        a2 = (b ** 3 - 4) * pow(3 * b, Q - 2, Q) % Q
        a = pow(a2, (Q + 1) // 4, Q)
        assert a * a % Q == a2
        x = (a, b)
        rhs = PM.f2_add(PM.f2_mul(PM.f2_sqr(x), x), (4, 4))
        assert rhs[1] == 0
        if tag == "imag":      # a non-residue of Fq: y = c u with c^2 = -rhs (f2_sqrt's alpha == -1 branch)
            assert not is_qr(rhs[0])
            c = pow(-rhs[0] % Q, (Q + 1) // 4, Q)
            y = (0, c)
        else:                  # a residue of Fq: y in Fq, y.c1 = 0 (the c0 fallback of the lexicographic comparison)
            assert is_qr(rhs[0])
            y = (pow(rhs[0], (Q + 1) // 4, Q), 0)
        assert PM.f2_sqr(y) == rhs
        special.append(("twist_" + tag, (x, y)))
    out = {"g1": {"sub": g1, "curve": [("T", T1), ("x4", S1), ("x0", Z1)]},
           "g2": {"sub": g2, "curve": [("T", T2)] + special}}
    for group in GROUPS:       # "sub": multiples of a generator of order r.  "curve": outside, checked with plain additions, once
        assert not any(times_r_is_identity(group, P) for _, P in out[group]["curve"])
        out[group]["curve"] += [(n + "_neg", neg(group, P)) for n, P in out[group]["curve"]]
    return out


# ---- the entries -------------------------------------------------------------------------------------------------------------------
def _wire_entries(group, add):
    base = base_points()[group]
    deg = 1 if group == "g1" else 2
    finite = [(n, P, "ok") for n, P in base["sub"]] + [(n, P, "ok-oncurve-only") for n, P in base["curve"]]
    for fmt in (UNCOMPRESSED, COMPRESSED):
        size = point_bytes(group, fmt)
        good_top = 4 if fmt == COMPRESSED else 0
        # honest encodings of every base point (both y signs occur)
        for n, P, cls in finite:
            add(fmt, encode_point(group, fmt, P), cls, P, "honest_" + n)
        # one honest encoding under all 8 values of the top three bits (compressed, infinity, sign)
        for n, P, cls in (finite[0], finite[1], finite[len(base["sub"])]):
            honest = encode_point(group, fmt, P)
            larger = y_is_larger(group, P)
            assert honest[0] >> 5 == (good_top | (1 if fmt == COMPRESSED and larger else 0))
            for top in range(8):
                data = with_flags(honest, top)
                if data == honest:
                    continue
                if fmt == COMPRESSED and top == (honest[0] >> 5) ^ 1:   # only the sign differs: the honest encoding of -P
                    add(fmt, data, cls, neg(group, P), "flags%d_%s" % (top, n))
                else:          # wrong compression bit, infinity bit over a payload, sign bit on an uncompressed point
                    add(fmt, data, "bad-flags", None, "flags%d_%s" % (top, n))
        # the identity: canonical; with the sign flag; with one nonzero byte behind the flags
        ident = encode_point(group, fmt, None)
        assert ident == bytes([0x40 | (good_top << 5)]) + bytes(size - 1)
        add(fmt, ident, "ok", None, "identity")
        add(fmt, with_flags(ident, good_top | 3), "bad-flags", None, "identity_sign")
        add(fmt, set_byte(ident, 0, ident[0] | 0x01), "bad-flags", None, "identity_byte0_low_bit")
        offsets = {1, size // 2, size - 1}
        if group == "g2":
            offsets |= {48 + 5}                      # the second half of x
            if fmt == UNCOMPRESSED:
                offsets |= {96 + 5, 144 + 5}         # the y half
        for off in sorted(offsets):
            add(fmt, set_byte(ident, off, 0x01), "bad-flags", None, "identity_payload_%d" % off)
        # all-zero bytes
        if fmt == UNCOMPRESSED:
            add(fmt, bytes(size), "bad-curve", None, "all_zero")      # (0, 0): 0 != 0 + b
        else:
            add(fmt, bytes(size), "bad-flags", None, "all_zero")      # the compression bit is clear
    # compressed x at the bounds of [0, q), component by component; the other component of a G2 x is 0
    for which in range(deg):                          # 0: the component in the first 48 bytes (G2: c1), 1: G2's c0
        tag = "x" if group == "g1" else ("c1" if which == 0 else "c0")
        for name, v, cls in (("q-1", Q - 1, None), ("q", Q, "bad-range"), ("q+1", Q + 1, "bad-range"), ("2^381-1", (1 << 381) - 1, "bad-range")):
            parts = [0] * deg
            parts[which] = v
            data = with_flags(b"".join(be(p) for p in parts), 4)
            if cls is None:
                # G1: (-1)^3 + 4 = 3, a non-residue mod q.  G2 c0 = -1: x^3 + b = 3 + 4u (norm 25 = 5^2: a square of Fq2);
                # G2 c1 = -1: x = -u, x^3 = u, x^3 + b = 4 + 5u (norm 41, a non-residue)
                if group == "g1":
                    assert not is_qr(3)
                    cls, P = "bad-sqrt", None
                elif which == 1:
                    assert f2_is_square((3, 4))
                    P = _smaller_root_point("g2", (Q - 1, 0))
                    assert not times_r_is_identity("g2", P)
                    cls = "ok-oncurve-only"
                else:
                    assert not f2_is_square((4, 5))
                    cls, P = "bad-sqrt", None
                add(COMPRESSED, data, cls, P, "bound_%s_%s" % (tag, name))
            else:
                add(COMPRESSED, data, cls, None, "bound_%s_%s" % (tag, name))
    # aliases v + q of real curve points whose first component is small enough to stay under the flag bits
    small = dict(base["curve"])["x4" if group == "g1" else "T"]
    c = comps(group, small)
    assert c[0] + Q < 1 << 381
    for k in range(deg):                              # compressed: every component of x
        parts = list(c[:deg])
        parts[k] += Q
        honest = encode_point(group, COMPRESSED, small)
        data = bytes([(honest[0] & 0xE0) | be(parts[0])[0]]) + b"".join(be(p) for p in parts)[1:]
        add(COMPRESSED, data, "bad-range", None, "alias_x%d_plus_q" % k)
    for k in range(2 * deg):                          # uncompressed: every component of x and y
        parts = list(c)
        parts[k] += Q
        add(UNCOMPRESSED, b"".join(be(p) for p in parts), "bad-range", None, "alias_%d_plus_q" % k)
    # off the curve / no square root
    P = base["sub"][2][1]
    c = comps(group, P)
    for k in range(1, 2 * deg):                       # the same alias on a point of the subgroup (its first component is too large)
        parts = list(c)
        parts[k] += Q
        add(UNCOMPRESSED, b"".join(be(p) for p in parts), "bad-range", None, "alias_sub_%d_plus_q" % k)
    c[-1] = (c[-1] + 1) % Q
    add(UNCOMPRESSED, b"".join(be(p) for p in c), "bad-curve", None, "y_plus_1")
    if group == "g1":
        for x in (1, 7):                              # 1 + 4 = 5 and 343 + 4 = 347: non-residues
            assert not is_qr(x ** 3 + 4)
            add(COMPRESSED, with_flags(be(x), 4), "bad-sqrt", None, "nonresidue_x%d" % x)
            add(COMPRESSED, with_flags(be(x), 5), "bad-sqrt", None, "nonresidue_x%d_sign" % x)
    else:
        for x in ((1, 0), (0, 2)):                    # 5 + 4u (norm 41) and 4 + (4 - 8)u = 4 - 4u (norm 32 = 2^5, 2 a non-residue)
            rhs = PM.f2_add(PM.f2_mul(PM.f2_sqr(x), x), (4, 4))
            assert not f2_is_square(rhs)
            add(COMPRESSED, with_flags(be(x[1]) + be(x[0]), 4), "bad-sqrt", None, "nonresidue_x%d_%d" % x)
        # an honest encoding with the halves of its Fq2 coordinates swapped (c0 || c1 instead of c1 || c0)
        for n, P in base["sub"][:2]:
            (x0, x1), (y0, y1) = P
            sx = (x1, x0)
            assert not f2_is_square(PM.f2_add(PM.f2_mul(PM.f2_sqr(sx), sx), (4, 4)))      # so the compressed form has no root
            honest = encode_point(group, COMPRESSED, P)
            add(COMPRESSED, bytes([(honest[0] & 0xE0) | be(x0)[0]]) + be(x0)[1:] + be(x1), "bad-sqrt", None, "swapped_halves_" + n)
            assert PM.f2_sqr((y1, y0)) != PM.f2_add(PM.f2_mul(PM.f2_sqr(sx), sx), (4, 4))
            add(UNCOMPRESSED, be(x0) + be(x1) + be(y0) + be(y1), "bad-curve", None, "swapped_halves_" + n)


def _smaller_root_point(group, x):
    """the curve point over x whose y is the lexicographically smaller root (a compressed encoding without the sign flag)"""
    P = _g1_at(x) if group == "g1" else _g2_at(x)
    assert P is not None
    return neg(group, P) if y_is_larger(group, P) else P


def _mont_entries(group, add):
    base = base_points()[group]
    deg = 1 if group == "g1" else 2
    rng = random.Random(0xDEC0DE + deg)
    finite = [(n, P, "ok") for n, P in base["sub"]] + [(n, P, "ok-oncurve-only") for n, P in base["curve"]]
    one = [1] + [0] * (deg - 1)
    F_mul = (lambda a, b: [a[0] * b[0] % Q]) if deg == 1 else (lambda a, b: list(PM.f2_mul(tuple(a), tuple(b))))

    def jac(P, z):
        """(x z^2, y z^3, z) as limb integers"""
        l = limbs(group, P)
        z2 = F_mul(z, z)
        z3 = F_mul(z2, z)
        return F_mul(l[:deg], z2) + F_mul(l[deg:], z3) + list(z)

    def blob(vals):
        return b"".join(mont(v) for v in vals)

    for n, P, cls in finite:
        add(AFFINE_MONT, blob(limbs(group, P)), cls, P, "honest_" + n)
        add(JACOBIAN_MONT, blob(limbs(group, P) + one), cls, P, "honest_" + n)
    add(AFFINE_MONT, bytes(point_bytes(group, AFFINE_MONT)), "ok", None, "identity")
    add(JACOBIAN_MONT, bytes(point_bytes(group, JACOBIAN_MONT)), "ok", None, "identity")
    P = base["sub"][3][1]
    l = limbs(group, P)
    # the limb alias v + q of every limb vector (v + q < 2^384)
    for k in range(2 * deg):
        data = blob(l)
        v = int.from_bytes(data[48 * k:48 * k + 48], "little") + Q
        add(AFFINE_MONT, data[:48 * k] + le(v) + data[48 * k + 48:], "bad-range", None, "limb%d_plus_q" % k)
    for k in range(3 * deg):
        data = blob(l + one)
        v = int.from_bytes(data[48 * k:48 * k + 48], "little") + Q
        add(JACOBIAN_MONT, data[:48 * k] + le(v) + data[48 * k + 48:], "bad-range", None, "limb%d_plus_q" % k)
    add(AFFINE_MONT, b"".join(le(Q) for _ in range(2 * deg)), "bad-range", None, "every_limb_vector_q")     # q itself: zero mod q, not < q
    # off the curve
    add(AFFINE_MONT, blob(l[:-1] + [l[-1] + 1]), "bad-curve", None, "y_plus_1")
    add(JACOBIAN_MONT, blob(l[:-1] + [l[-1] + 1] + one), "bad-curve", None, "y_plus_1")
    # x = 0 or y = 0 is a coordinate like any other, not a sign of the identity
    zero = [0] * deg
    if group == "g2":   # (0, 2): 4 != 0 + 4(1+u); no twist point has x = 0 at all (4(1+u) has norm 32, a non-residue)
        add(AFFINE_MONT, blob(zero + [2, 0]), "bad-curve", None, "x0_y2")
        add(JACOBIAN_MONT, blob(zero + [2, 0] + one), "bad-curve", None, "x0_y2")
    # (x, 0): y = 0 would be a point of order 2, and both group orders are odd -- no such point exists
    add(AFFINE_MONT, blob(l[:deg] + zero), "bad-curve", None, "x_y0")
    add(JACOBIAN_MONT, blob(l[:deg] + zero + one), "bad-curve", None, "x_y0")
    add(JACOBIAN_MONT, blob(zero + zero + one), "bad-curve", None, "x0_y0_z1")      # 0 != 0 + b Z^6 as long as Z != 0
    add(JACOBIAN_MONT, blob(zero + zero + [5] * deg), "bad-curve", None, "x0_y0_z5")
    # Z = 0 is the identity whatever X and Y are, as long as they are < q
    xy = [rng.randrange(Q) for _ in range(2 * deg)]
    add(JACOBIAN_MONT, blob(xy + zero), "ok", None, "z0_random_xy")
    for k in range(2 * deg):
        data = blob(xy + zero)
        v = int.from_bytes(data[48 * k:48 * k + 48], "little") + Q
        add(JACOBIAN_MONT, data[:48 * k] + le(v) + data[48 * k + 48:], "bad-range", None, "z0_limb%d_plus_q" % k)
    add(JACOBIAN_MONT, blob(xy) + b"".join(le(Q) for _ in range(deg)), "bad-range", None, "z_equals_q")     # Z = q: zero mod q, not < q
    # Z != 1, on and off the curve
    zs = [[7] + [0] * (deg - 1), [rng.randrange(1, Q) for _ in range(deg)]]
    if group == "g2":
        zs.append([0, rng.randrange(1, Q)])           # Z = z1 u
    for zi, z in enumerate(zs):
        for n, P, cls in (finite[1], finite[len(base["sub"])]):
            j = jac(P, z)
            add(JACOBIAN_MONT, blob(j), cls, P, "z%d_%s" % (zi, n))
            j[2 * deg - 1] = (j[2 * deg - 1] + 1) % Q
            add(JACOBIAN_MONT, blob(j), "bad-curve", None, "z%d_%s_y_plus_1" % (zi, n))


@functools.lru_cache(maxsize=None)
def corpus():
    out = []
    for group in GROUPS:
        def add(fmt, data, cls, point, name, group=group):
            assert len(data) == point_bytes(group, fmt) and cls in OK_CLASSES + BAD_CLASSES
            assert cls in OK_CLASSES or point is None
            same = [e for e in out if (e.group, e.fmt, e.data) == (group, fmt, bytes(data))]
            if same:           # two constructions of the same bytes (the sign-flipped encoding of P is the honest one of -P) agree
                assert (same[0].cls, same[0].point) == (cls, point), (same[0].name, name)
                return
            out.append(Entry(group, fmt, bytes(data), cls, point, "%s-%s-%s" % (group, FMT_NAMES[fmt], name)))
        _wire_entries(group, add)
        _mont_entries(group, add)
    assert len({e.name for e in out}) == len(out)
    assert len({(e.group, e.fmt, e.data) for e in out}) == len(out), "two entries with the same bytes"
    return tuple(out)


def entries(group=None, fmt=None, classes=None):
    return [e for e in corpus() if (group is None or e.group == group) and (fmt is None or e.fmt == fmt) and
            (classes is None or e.cls in classes)]
