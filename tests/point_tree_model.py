"""Big-int model of kzg_amd/csrc/point_tree.hip (kzg_point_tree_*), step by step: the tree padded with dummy points 0 to a power of
two, schoolbook products up to the leaf size and products wrapped modulo X^(2d) - 1 with the top coefficient fixed above it, the
power-series inverse of the reversed root, the correlation going down (schoolbook / cyclic at the node's size), blocks of K
coefficients combined in x^K, the combination going up, and den_i = M'(x_i) through the model's own evaluation.

Products of coefficient lists go through one big-integer multiplication (Kronecker substitution): the plain convolution, exact."""
import os
import re

from oracle import kzg_model as M

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "kzg_amd", "csrc", "point_tree.hip")
SLOT = 66  # bytes per coefficient of a packed polynomial: 2 x 255 bits for a product and 18 bits for sums of up to 2^18 of them


def constant(name, src=None):
    """an integer `constexpr ... NAME = <int or 1 << int>` of point_tree.hip"""
    src = open(SRC).read() if src is None else src
    m = re.search(r"constexpr\s+[\w:]+\s+(?:\w+\s*=\s*[^,;]+,\s*)*%s\s*=\s*(?:\(size_t\))?\s*(\d+)(?:\s*<<\s*(\d+))?\s*[;,]" % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


LEAF = constant("PT_LEAF")
SMALL = 1 << constant("PT_SMALL_LOG")
CHUNK_ELEMS = constant("PT_CHUNK_ELEMS")


def pmul(a, b):
    """the plain product of two coefficient lists, reduced mod r"""
    if not a or not b:
        return []
    assert min(len(a), len(b)) < 1 << 18
    x = int.from_bytes(b"".join(int(v % R).to_bytes(SLOT, "little") for v in a), "little")
    y = int.from_bytes(b"".join(int(v % R).to_bytes(SLOT, "little") for v in b), "little")
    n = len(a) + len(b) - 1
    raw = (x * y).to_bytes(SLOT * (n + 1), "little")
    return [int.from_bytes(raw[i * SLOT:(i + 1) * SLOT], "little") % R for i in range(n)]


def cyc(a, b, T):
    """a b modulo X^T - 1"""
    out = [0] * T
    for i, v in enumerate(pmul(a, b)):
        out[i % T] = (out[i % T] + v) % R
    return out


def corr(m, f, T):
    """out[t] = sum_j m[j] f[(t + j) mod T], t < T: the cyclic correlation a transform of T points computes"""
    out = [0] * T
    for i, v in enumerate(pmul(m[::-1], f)):  # index i holds sum m[j] f[s] over s - j = i - (len(m) - 1)
        t = (i - (len(m) - 1)) % T
        out[t] = (out[t] + v) % R
    return out


def next_pow2(k):
    K = 1
    while K < k:
        K *= 2
    return K


class Tree:
    def __init__(self, xs, leaf=LEAF):
        assert len(xs) >= 1 and all(0 <= x < R for x in xs) and leaf >= 1 and leaf & (leaf - 1) == 0
        self.k, self.leaf = len(xs), leaf
        self.K = K = next_pow2(self.k)
        self.pts = list(xs) + [0] * (K - self.k)
        self.levels = [[[(-x) % R] for x in self.pts]]  # the low d coefficients of every monic node of degree d
        d = 1
        while d < K:
            cur, nxt = self.levels[-1], []
            for v in range(0, len(cur), 2):
                a, b = cur[v] + [1], cur[v + 1] + [1]
                if 2 * d <= leaf:                  # schoolbook: the coefficients below X^(2d)
                    w = pmul(a, b)[: 2 * d]
                else:                              # wrapped: the top 1 lands on coefficient 0
                    w = cyc(a, b, 2 * d)
                    w[0] = (w[0] - 1) % R
                nxt.append(w)
            self.levels.append(nxt)
            d *= 2
        root = self.levels[-1][0] + [1]            # X^(K - k) M
        self.G = series_inverse(root[::-1], K)
        self.M = root[K - self.k:]
        self.xK = [pow(x, K, R) for x in self.pts]
        dM = [self.M[i] * i % R for i in range(1, self.k + 1)]
        self.den = self.eval(dM)
        self.distinct = all(self.den)
        self.den_inv = [pow(v, -1, R) if v else 0 for v in self.den]

    # ---- evaluation ----
    def eval_block(self, p):
        """the values of at most K coefficients at all K (real and dummy) points"""
        K = self.K
        assert len(p) <= K
        P = ([c % R for c in p] + [0] * (K - len(p)))[::-1]
        f = [cyc(P, self.G, 2 * K)[:K]]
        lv, D = len(self.levels) - 1, K
        while D > 1:
            d, nodes, nf = D // 2, self.levels[lv - 1], []
            for v, fv in enumerate(f):
                for sib in (nodes[2 * v + 1] + [1], nodes[2 * v] + [1]):  # the left child takes the RIGHT sibling
                    if D <= self.leaf:
                        nf.append([sum(sib[j] * fv[t + j] for j in range(d + 1)) % R for t in range(d)])
                    else:
                        nf.append(corr(sib, fv, D)[:d])
            f, D, lv = nf, d, lv - 1
        return [f[i][0] for i in range(K)]

    def eval(self, p):
        K = self.K
        blocks = [self.eval_block(p[i:i + K]) for i in range(0, len(p), K)]
        out = []
        for i in range(self.k):
            acc = 0
            for vals in reversed(blocks):
                acc = (acc * self.xK[i] + vals[i]) % R
            out.append(acc)
        return out

    # ---- combination ----
    def combine(self, cs, weights=None):
        k, K = self.k, self.K
        assert len(cs) == k
        N = [[c % R * (weights[i] if weights else 1) % R] for i, c in enumerate(cs)] + [[0]] * (K - k)
        d, lv = 1, 0
        while d < K:
            nodes, nn = self.levels[lv], []
            for v in range(0, len(N), 2):
                ml, mr = nodes[v] + [1], nodes[v + 1] + [1]
                if 2 * d <= self.leaf:
                    a, b = pmul(N[v], mr), pmul(N[v + 1], ml)
                else:
                    a, b = cyc(N[v], mr, 2 * d), cyc(N[v + 1], ml, 2 * d)
                a, b = a + [0] * (2 * d - len(a)), b + [0] * (2 * d - len(b))
                nn.append([(x + y) % R for x, y in zip(a[: 2 * d], b[: 2 * d])])
            N, d, lv = nn, 2 * d, lv + 1
        return N[0][K - k:]

    def interpolate(self, ys):
        assert self.distinct
        return self.combine(ys, self.den_inv)

    # ---- what the plan holds ----
    def plan_bytes(self):
        return plan_bytes(self.k, self.leaf)


def plan_bytes(k, leaf=LEAF):
    """HBM the plan holds: every level's low coefficients (K each), the kept transforms (2K per level from the leaf size up to K / 2),
    the transform of G (2K), the two twiddle tables (K each), the points and their K-th powers (K each), 1 / den (k) and M (k + 1)"""
    K = next_pow2(k)
    log_K = K.bit_length() - 1
    nhat = sum(1 for j in range(log_K) if (1 << j) >= leaf)
    return 32 * ((log_K + 1) * K + nhat * 2 * K + 2 * K + 2 * K + 2 * K + k + (k + 1))


def series_inverse(f, m):
    """g = 1 / f mod X^m: the recurrence g_i = -g_0 sum_{j >= 1} f_j g_(i - j) up to 64 coefficients, then Newton doubling
    g <- g (2 - f g) mod X^hi (the inverse is unique: the same coefficients either way)"""
    g = [pow(f[0], -1, R)]
    for i in range(1, min(m, 64)):
        s = sum(f[j] * g[i - j] for j in range(1, min(i, len(f) - 1) + 1)) % R
        g.append((-g[0] * s) % R)
    while len(g) < m:
        hi = min(2 * len(g), m)
        e = [(-v) % R for v in pmul(f[:hi], g)[:hi]]
        e[0] = (e[0] + 2) % R
        g = pmul(g, e)[:hi]
    return g


def chunk_units(K):
    """blocks (or vectors) a chunk of the GPU calls holds"""
    return max(1, CHUNK_ELEMS // K)
