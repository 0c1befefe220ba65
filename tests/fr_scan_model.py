"""Python-integer model of kzg_fr_scan, kzg_fr_grand_product and kzg_fr_batch_inverse (kzg_amd/csrc/fr_scan.hip) on values below r."""
from oracle import kzg_model as M

R = M.R


def scan(vec, op="product", exclusive=False):
    """(out, total) of one vector"""
    acc, out = (1 if op == "product" else 0), []
    for v in vec:
        if exclusive:
            out.append(acc)
        acc = acc * v % R if op == "product" else (acc + v) % R
        if not exclusive:
            out.append(acc)
    return out, acc


def batch_inverse(vec):
    """(inverses with zero for zero, zeros)"""
    return [pow(v, -1, R) if v % R else 0 for v in vec], sum(1 for v in vec if v % R == 0)


def grand_product(num, den, n, t):
    """one vector: num, den are t columns of n values.  (z, total, zero_den); all zero where a denominator is zero"""
    N, D = [1] * n, [1] * n
    for j in range(t):
        for i in range(n):
            N[i] = N[i] * num[j * n + i] % R
            D[i] = D[i] * den[j * n + i] % R
    if any(d == 0 for d in D):
        return [0] * n, 0, 1
    inv, _ = batch_inverse(D)
    z, total = scan([a * b % R for a, b in zip(N, inv)], "product", True)
    return z, total, 0
