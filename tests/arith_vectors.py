"""Operand generators and big-integer checks of the field layers (kzg_amd/csrc/field.h, field30.h, fr29.h), shared by the CPU tests
of the portable branch (tests/test_host_math.py, through tests/host_math.cpp) and the GPU tests of the generated inline-asm branch
(tests/test_gpu_arith.py, through kzg_test_arith).  Every generator takes the caller's random.Random, so a caller's sequence of
draws -- and with it its cases -- is fixed by its own seed."""
import struct

from oracle import kzg_model as M

# ---- signed 13 x 30-bit Fq (field30.h) -------------------------------------------------------------------------------------------
N30, B30 = 13, 30
R30 = 1 << (N30 * B30)          # the Montgomery radix of the 30-bit layer
H30 = 1 << (B30 - 1)            # balanced digits lie in [-H30, H30)
U30 = (1 << B30) - 1            # largest unsigned digit
KINDS30 = ["max", "min", "neg_of_min", "alt", "rnd", "rnd", "rnd"]
UKINDS30 = ["umax", "umax", "urnd", "urnd", "uzero"]


def val30(l):
    return sum(v << (B30 * i) for i, v in enumerate(l))


def raw30(l):
    return struct.pack("<13i", *l)


def unraw30(b):
    return list(struct.unpack("<13i", b))


def limbs30(rng, kind):
    """Balanced limbs of one kind: every digit 2^29 - 1 / -2^29 / +2^29 (the limb-wise negation of a normalised value) /
    alternating extremes / random; a random top limb, |value| < 2^387 ~ 80 q."""
    if kind == "max":
        l = [H30 - 1] * 12
    elif kind == "min":
        l = [-H30] * 12
    elif kind == "neg_of_min":          # limb-wise negation of a normalised value: +2^29 digits
        l = [H30] * 12
    elif kind == "alt":
        l = [(-H30 if i & 1 else H30 - 1) for i in range(12)]
    else:
        l = [rng.randrange(-H30, H30) for _ in range(12)]
    return l + [rng.randrange(-(1 << 27), 1 << 27)]


def ulimbs30(rng, kind):
    """Unsigned-digit limbs (the outputs of mul30u / sqr30_sub2u): every digit 2^30 - 1, zero, or random."""
    if kind == "umax":
        l = [U30] * 12
    elif kind == "uzero":
        l = [0] * 12
    else:
        l = [rng.randrange(0, 1 << B30) for _ in range(12)]
    return l + [rng.randrange(-(1 << 23), 1 << 23)]


def is_normalised30(r):
    return all(-H30 <= v < H30 for v in r[:12])


def is_unsigned30(r):
    return all(0 <= v < (1 << B30) for v in r[:12])


def check_mont30(r, num, bound_q):
    """r: the 13 output limbs of a Montgomery product whose numerator is `num`: normalised, r * 2^390 = num (mod q) exactly, and
    |r| <= bound_q * q."""
    assert is_normalised30(r), r
    x = val30(r)
    assert (x * R30 - num) % M.Q == 0                                 # exact Montgomery quotient
    assert abs(x) / M.Q <= bound_q, (abs(x) / M.Q, bound_q)       # (the bound itself, not the bound truncated to 1/1000 q)


def mont30_bound(num_abs):
    """The documented magnitude bound of a 30-bit Montgomery product with |numerator| = num_abs, in units of q."""
    return 0.5001 + num_abs / M.Q / M.Q * (M.Q / R30)


def check_mul30_sub(r, a, b, c):
    """mul30_sub: normalised, exact a*b/R - c mod q, |r| <= |ab|/R + q/2 + |c| + 2."""
    assert is_normalised30(r), r
    assert ((val30(r) + val30(c)) * R30 - val30(a) * val30(b)) % M.Q == 0
    assert abs(val30(r)) <= abs(val30(a) * val30(b)) // R30 + M.Q // 2 + abs(val30(c)) + 2


def check_sqr30_sub2(r, a, c, e, unsigned=False):
    """sqr30_sub2 / sqr30_sub2u: exact a^2/R - c - 2e mod q; balanced (bounded) or unsigned digits."""
    if unsigned:
        assert is_unsigned30(r), r
    else:
        assert is_normalised30(r), r
        assert abs(val30(r)) <= val30(a) ** 2 // R30 + M.Q // 2 + abs(val30(c)) + 2 * abs(val30(e)) + 2
    assert ((val30(r) + val30(c) + 2 * val30(e)) * R30 - val30(a) ** 2) % M.Q == 0


def check_mul30_any(r, a, b, unsigned):
    """mul30 / mul30u with an unsigned operand: exact, |r| <= |ab|/R + q/2 + 2, balanced or unsigned digits."""
    assert ((val30(r)) * R30 - val30(a) * val30(b)) % M.Q == 0
    assert abs(val30(r)) <= abs(val30(a) * val30(b)) // R30 + M.Q // 2 + 2
    assert (is_unsigned30(r) if unsigned else is_normalised30(r)), r


def normalize30_input(rng):
    """Limbs below 3 * 2^29 in magnitude (what normalize30 accepts)."""
    return [rng.randrange(-3 * H30 + 1, 3 * H30) for _ in range(12)] + [rng.randrange(-(1 << 20), 1 << 20)]


def balanced30(x):
    """The normalised 13-limb form of the integer x."""
    l, t = [], x
    for _i in range(12):
        d = ((t + H30) % (1 << B30)) - H30
        l.append(d)
        t = (t - d) >> B30
    l.append(t)
    return l


def from30_input(rng):
    """A lazy value up to 255 q in magnitude, either sign, normalised (what from30 accepts); returns (limbs, x)."""
    x = rng.randrange(-255 * M.Q, 255 * M.Q)
    return balanced30(x), x


def from30_want(x):
    return x * pow(R30, -1, M.Q) * M.FQ_MONT_R % M.Q


# ---- 9 x 29-bit Fr (fr29.h) ------------------------------------------------------------------------------------------------------
MASK29 = (1 << 29) - 1
R256, B261 = 1 << 256, 1 << 261


def limbs29(v):
    return [(v >> (29 * i)) & MASK29 for i in range(9)]


def val29(ls):
    return sum(int(x) << (29 * i) for i, x in enumerate(ls))


def mont_r(w):
    """w -> its blst_fr Montgomery form w * 2^256 mod r (what the twiddle tables hold)."""
    return w * R256 % M.R


def shoup_operand(rng, it):
    """The x of a Shoup product, by it % 4: a normalised value below 2^256 (a tile load); any value below 2^261 (2^261 - 1 early);
    an unnormalised sum with every limb up to 1.5 * 2^30 (every limb at that bound early); a value below r.  Returns the 9 raw
    limbs and the integer."""
    kind = it % 4
    if kind == 0:
        x = rng.randrange(R256)
        return limbs29(x), x
    if kind == 1:
        x = rng.randrange(B261) if it > 8 else B261 - 1
        return limbs29(x), x
    if kind == 2:
        raw = [rng.randrange(3 << 29) for _ in range(8)] + [rng.randrange(1 << 27)]
        if it < 12:
            raw = [(3 << 29) - 1] * 8 + [(1 << 27) - 1]
        x = val29(raw)
        assert x < B261
        return raw, x
    x = rng.randrange(M.R)
    return limbs29(x), x


def shoup_twiddle(rng, it):
    return rng.randrange(M.R) if it > 3 else [0, 1, M.R - 1, 7][it]


def check_shoup(out, x, w):
    """A Shoup product: limbs normalised, exact mod r, below 2r."""
    assert all(0 <= v <= MASK29 for v in out), out
    got = val29(out)
    assert got % M.R == x * w % M.R and got < 2 * M.R


def shoup_pair(w):
    """(w, wp) of the twiddle table: wp = floor(w 2^261 / r)."""
    return w, (w << 261) // M.R


def radix4_chain_ref(x0, xs, ws, pairs, which):
    """`pairs` radix-4 stage pairs along one element chain (output `which` continues): the exact value mod r."""
    X0 = x0
    for p in range(pairs):
        x1, x2, x3 = xs[3 * p: 3 * p + 3]
        a, bb, c = ws[3 * p: 3 * p + 3]
        t1, t3 = x1 * a, x3 * a
        s0, y1, s2, y3 = X0 + t1, X0 - t1, x2 + t3, x2 - t3
        t2, t3b = s2 * bb, y3 * c
        X0 = [s0 + t2, y1 + t3b, s0 - t2, y1 - t3b][which] % M.R
    return X0 % M.R


def radix4_chain_case(rng, pairs):
    """x0, 3 * pairs inputs and 3 * pairs twiddles (all random 256-bit inputs, twiddles below r)."""
    x0 = rng.randrange(R256)
    xs = [rng.randrange(R256) for _ in range(3 * pairs)]
    ws = [rng.randrange(M.R) for _ in range(3 * pairs)]
    return x0, xs, ws


QUOTIENT_MAX_M = 10
QUOTIENT_NB_MAX = 25 * M.R     # the largest neighbour value the quotient kernels hold


QUOTIENT_BIG_X = [M.R - 1, 1, 0, M.R - 2, 2, M.R - 1]


def quotient_case(rng, it):
    """One thread of the quotient kernels: eight raw 256-bit coefficients, x, the step constant p, m <= 10 neighbour values below
    25 r, the next coefficient.  The first six cases put every operand at its largest (coefficients 2^256 - 1, p = r - 1, ten
    neighbours just below 25 r) with x at the edges.  Returns (a, x, p, m, nbv, a_next)."""
    big = it < len(QUOTIENT_BIG_X)
    a = [R256 - 1 if big else rng.randrange(R256) for _ in range(8)]
    x = QUOTIENT_BIG_X[it] if big else rng.randrange(M.R)
    p = M.R - 1 if big else rng.randrange(M.R)
    m = QUOTIENT_MAX_M if big else rng.randrange(0, QUOTIENT_MAX_M + 1)
    nbv = [QUOTIENT_NB_MAX - 1 - i if big else rng.randrange(QUOTIENT_NB_MAX) for i in range(m)]
    a_next = rng.randrange(M.R) if not big else M.R - 1
    return a, x, p, m, nbv, a_next


def nb_limbs(v):
    """A neighbour value as read from LDS: limbs below 2^29, the excess in the top limb."""
    return [(v >> (29 * j)) & MASK29 if j < 8 else v >> 232 for j in range(9)]


def quotient_want(a, x, p, nbv, a_next):
    scan = (sum(c * pow(x, k, M.R) for k, c in enumerate(a)) + p * sum(nbv)) % M.R
    return scan, (a_next + scan * x) % M.R


QUOTIENT_TOP_MAX = 64 * (M.R >> 232)     # what fr29_reduce_below_2r accepts


# ---- saturated Fq / Fr (field.h) -------------------------------------------------------------------------------------------------
def saturated_edges(p, nlimbs):
    """Edge operands of the saturated add / sub / mul, all < p: 0, 1, p-1, p-2, R mod p, pairs summing to p, p-1 and 2p-2, a = b,
    a borrow that starts at every limb position, all-ones limb patterns below p.  Returns a list of (a, b)."""
    R = 1 << (32 * nlimbs)
    top = p >> (32 * (nlimbs - 1))
    singles = [0, 1, p - 1, p - 2, R % p, (R * R) % p, p >> 1, (p + 1) >> 1]
    for k in range(nlimbs):                    # all-ones patterns: the low k limbs all ones, the rest of the value below p
        v = (1 << (32 * k)) - 1
        if v < p:
            singles.append(v)
        if k < nlimbs - 1:
            singles.append(v | (top - 1) << (32 * (nlimbs - 1)))
    pairs = [(x, y) for x in singles for y in singles]
    for s in (p, p - 1, 2 * p - 2):            # a + b = p (add: 0), p - 1 (the largest unreduced), 2p - 2 (the largest sum)
        for x in singles + [p // 3, p // 7 * 5]:
            y = s - x
            if 0 <= x < p and 0 <= y < p:
                pairs.append((x, y))
    pairs += [(x, x) for x in singles]         # a = b: sub gives 0
    for k in range(nlimbs):                    # borrow starting at limb k and running to the top: a - b with a's limb k below b's
        b = 1 << (32 * k)
        pairs.append((0, b))
        pairs.append(((1 << (32 * k)) - 1, b))
        pairs.append((p - 1 - b, p - 1))
    return [(x % p, y % p) for x, y in pairs]
