"""A big-int model of kzg_poly_divide as poly_divide.hip computes it: the series inverse of the reversed divisor by a
schoolbook base and Newton doubling with wrapped cyclic products, the quotient as a reversed truncated product, the remainder from
a - q b folded modulo X^N - 1.  Cyclic products stand for the NTTs: a transform of T points multiplies modulo X^T - 1.  Imported by
test_poly_divide_model.py (against oracle.kzg_model) and by test_gpu_poly_divide.py (to build exact divisions)."""
from oracle.kzg_model import R, fr_inv

DEFAULT_BASE = 64  # PD_BASE in poly_divide.hip


def pow2_ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def cyclic_mul(a, b, T):
    """a b mod (X^T - 1): what forward transforms of T points, a pointwise product and the inverse transform give"""
    out = [0] * T
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[(i + j) % T] = (out[(i + j) % T] + x * y) % R
    return out


def fold(v, N):
    """v mod (X^N - 1)"""
    out = [0] * N
    for i, x in enumerate(v):
        out[i % N] = (out[i % N] + x) % R
    return out


def newton_size(k, hi, fl):
    """transform size of the Newton level k -> hi (k < hi <= 2k) for a divisor with fl coefficients below X^hi: the product
    f g g has fl + 2k - 2 coefficients; wrapped modulo X^T - 1 the ones from T on land below fl + 2k - 2 - T, which must not reach k"""
    return pow2_ceil(max(hi, fl + k - 2))


def series_inverse(f, m, base=DEFAULT_BASE, levels=None):
    """g = 1 / f mod X^m (f[0] != 0); `levels` collects the (k, hi, T) of the Newton levels"""
    k = min(base, m)
    g0 = fr_inv(f[0])
    g = [g0]
    for i in range(1, k):  # g_i = -g_0 sum_{j >= 1} f_j g_(i-j)
        s = sum(f[j] * g[i - j] for j in range(1, min(i, len(f) - 1) + 1)) % R
        g.append((-g0 * s) % R)
    while k < m:
        hi = min(2 * k, m)
        fl = min(hi, len(f))
        T = newton_size(k, hi, fl)
        F, G = f[:fl], g  # k coefficients of g
        e = cyclic_mul(F, G, T)                      # pointwise F G ...
        e = [(2 - x) % R if i == 0 else (-x) % R for i, x in enumerate(e)]
        # (the device does 2 - F G on the transformed values, where the constant 2 is 2 at every point; here on coefficients)
        h = cyclic_mul(e, G, T)                      # ... G (2 - F G)
        g = g + h[k:hi]                              # the low k coefficients do not change
        if levels is not None:
            levels.append((k, hi, T))
        k = hi
    return g


def divide(a, b, base=DEFAULT_BASE, levels=None):
    """(q, r) zero-padded to na - nb + 1 and nb - 1 coefficients; b[-1] != 0 mod r"""
    a, b = [x % R for x in a], [x % R for x in b]
    na, nb = len(a), len(b)
    assert na >= 1 and nb >= 1 and b[-1] != 0
    if na < nb:
        return [], a + [0] * (nb - 1 - na)
    m = na - nb + 1
    if nb == 1:
        c = fr_inv(b[0])
        return [x * c % R for x in a], []
    f = b[::-1]
    g = series_inverse(f, m, base, levels)
    Tq = pow2_ceil(2 * m - 1)
    ra = a[::-1][:m]                                 # rev(a) mod X^m
    q = cyclic_mul(ra, g, Tq)[:m][::-1]
    N = pow2_ceil(nb - 1)
    qb = cyclic_mul(fold(q, N), fold(b, N), N)
    af = fold(a, N)
    r = [(x - y) % R for x, y in zip(af, qb)][: nb - 1]
    return q, r
