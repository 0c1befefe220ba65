"""Big-int model of exactly the steps of kzg_msm_g2_bucket (kzg_amd/csrc/g2_msm.hip): the signed 8-bit window digits, the slice / slot
/ window / bucket accumulation chunk after chunk into one arena, the fold of the slots, the suffix scan and tree sum of a window, the
Horner chain over the windows; and of kzg_verify_eval_tree (kzg_amd/csrc/witness_tree.hip) with the opening it checks: the plan's product
M, p = q M + r with r the interpolant, hz by that bucket sum, the pairing equation.  Points are the affine pairs of
oracle/pairing_model.py and oracle/kzg_model.py (None = the identity)."""
from oracle import kzg_model as M
from oracle import pairing_model as P

C = 8                 # window bits
W = 32                # windows: 32 x 8 = 256 > the top bit of a reduced scalar
D = 1 << (C - 1)      # buckets per window: |digit| in 1..128
SLICE, SLOTS = 2048, 16   # the defaults of options g2_msm_slice / g2_msm_slots


def digit(k, win):
    """vc_digit: Booth recoding, every digit from its own c + 1 bits: bits[c win, c win + c) + bit[c win - 1] - 2^c bit[c win + c - 1]"""
    assert 0 <= k < 1 << 256
    x = ((k << 1) >> (C * win)) & ((2 << C) - 1)
    d = (x >> 1) + (x & 1)
    return d - (1 << C) if x >> C else d


def digits(k):
    return [digit(k, w) for w in range(W)]


def recompose(ds):
    return sum(d << (C * w) for w, d in enumerate(ds))


def accumulate(points, scalars, S=SLICE, slots=SLOTS):
    """arena[slot][win][b] after every chunk of slots x S points has added into it; returns (arena, slots used)"""
    assert len(points) == len(scalars) and S & (S - 1) == 0 and 1 <= S <= 2048 and 1 <= slots <= 16
    arena = [[[None] * D for _ in range(W)] for _ in range(slots)]
    used, CH = 1, slots * S
    for i0 in range(0, len(points), CH):          # a chunk: one launch
        B = min(CH, len(points) - i0)
        used = max(used, (B + S - 1) // S)
        for p in range(B):                         # slice p // S is slot p // S of this chunk
            k = scalars[i0 + p] % M.R              # reduced BEFORE the digits are taken
            for w in range(W):
                d = digit(k, w)
                assert abs(d) <= D
                if d:
                    bk = arena[p // S][w]
                    bk[abs(d) - 1] = P.g2_add(bk[abs(d) - 1], points[i0 + p] if d > 0 else P.g2_neg(points[i0 + p]))
    return arena, used


def reduce_window(arena, used, w):
    """k_g2b_reduce: fold the slots, suffix sums in 7 doubling rounds, then a tree sum of the 128 suffixes"""
    sh = [None] * D
    for b in range(D):
        for g in range(used):
            sh[b] = P.g2_add(sh[b], arena[g][w][b])
    s = 1
    while s < D:
        sh = [P.g2_add(sh[t], sh[t + s]) if t + s < D else sh[t] for t in range(D)]
        s <<= 1
    s = D // 2
    while s >= 1:
        for t in range(s):
            sh[t] = P.g2_add(sh[t], sh[t + s])
        s >>= 1
    return sh[0]


def finish(wins):
    acc = wins[W - 1]
    for w in range(W - 2, -1, -1):
        for _ in range(C):
            acc = P.g2_add(acc, acc)
        acc = P.g2_add(acc, wins[w])
    return acc


def msm_g2_bucket(points, scalars, S=SLICE, slots=SLOTS):
    arena, used = accumulate(points, scalars, S, slots)
    return finish([reduce_window(arena, used, w) for w in range(W)])


# ---------------------------------------------------------------------------------------------------------------------
# kzg_verify_eval_tree (kzg_amd/csrc/witness_tree.hip) and the opening it checks.  Coefficient lists, lowest first.
# ---------------------------------------------------------------------------------------------------------------------
def product(xs):
    """M = prod (X - x_i): what the plan keeps (k + 1 coefficients, monic)"""
    m = [1]
    for x in xs:
        m = [((m[j - 1] if j else 0) - x * (m[j] if j < len(m) else 0)) % M.R for j in range(len(m) + 1)]
    return m


def divide(p, m):
    """p = q m + r for monic m of k + 1 coefficients: (q, r zero-padded to k coefficients); n <= k leaves q empty and r = p padded"""
    k = len(m) - 1
    assert m[k] == 1
    rem, q = [c % M.R for c in p], [0] * max(len(p) - k, 0)
    for i in range(len(p) - 1, k - 1, -1):
        c = rem[i]
        q[i - k] = c
        for j in range(k + 1):
            rem[i - k + j] = (rem[i - k + j] - c * m[j]) % M.R
    return q, (rem[:k] + [0] * k)[:k]


def interpolate(xs, ys):
    """the k coefficients of the polynomial of degree < k through (x_i, y_i): sum_i y_i / M'(x_i) M / (X - x_i)"""
    k, m = len(xs), product(xs)
    out = [0] * k
    for x, y in zip(xs, ys):
        quot, _ = divide(m, [(-x) % M.R, 1])
        w = y * M.fr_inv(sum(c * pow(x, j, M.R) for j, c in enumerate(quot)) % M.R) % M.R
        out = [(o + w * c) % M.R for o, c in zip(out, quot)]
    return out


def poly_eval(cs, x):
    acc = 0
    for c in reversed(cs):
        acc = (acc * x + c) % M.R
    return acc


def verify_eval_tree(gs, hs, xs, r, commitment, witness, S=SLICE, slots=SLOTS):
    """one check of kzg_verify_eval_tree: hz = the bucket sum of hs[0 .. k] against M, gr = MSM(gs[0 .. k), r), and
    e(w, hz) e(-(C - gr), hs[0]) == 1"""
    k = len(xs)
    assert len(r) == k and len(hs) >= k + 1 and len(gs) >= k
    hz = msm_g2_bucket(hs[:k + 1], product(xs), S, slots)
    gr = M.g1_multi_exp(gs[:k], r)
    a = M.g1_add(commitment, M.g1_neg(gr))
    return P.pairing_product_is_one([(witness, hz), (M.g1_neg(a), hs[0])])
