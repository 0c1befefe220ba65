"""Python-integer model of kzg_mle_eq / kzg_mle_bind / kzg_mle_eval / kzg_fr_program_degree / kzg_sumcheck_round (kzg_amd/csrc/mle.hip).
A multilinear polynomial in m variables is a table f of 2^m values, f[i] at the corner whose coordinate x_j is bit j of i; rounds bind
the TOP variable; point[j] belongs to variable j.  Any integer counts as its residue modulo r.  ShapeError wherever the library
returns KZG_ERR_SHAPE."""
from tests import fr_program_model as FM

R = FM.R
ShapeError = FM.ShapeError
MAX_EVAL, MAX_ACC, MAX_LOG, MAX_COLS = 16, 32, 28, 4096


def _scalars(xs):
    if any(not 0 <= x < R for x in xs):
        raise ShapeError("a single scalar is not below r")


def eq(point):
    """out[i] = prod_j (bit_j(i) ? point[j] : 1 - point[j]), by the definition (not by doubling)"""
    _scalars(point)
    if len(point) > MAX_LOG:
        raise ShapeError("m")
    out = []
    for i in range(1 << len(point)):
        v = 1
        for j, u in enumerate(point):
            v = v * (u if (i >> j) & 1 else 1 - u) % R
        out.append(v)
    return out


def bind(col, rho):
    n = len(col)
    if n < 2 or n & (n - 1) or n > 1 << MAX_LOG:
        raise ShapeError("n")
    _scalars([rho])
    h = n // 2
    return [(col[i] + rho * (col[i + h] - col[i])) % R for i in range(h)]


def evaluate(f, point):
    """(f(point), quotients): binding from the top variable down; the 2^k values of q_k = hi - lo at quotients[2^k - 1 ..]"""
    m = len(point)
    if len(f) != 1 << m or m > MAX_LOG:
        raise ShapeError("table length")
    _scalars(point)
    cur, q = [x % R for x in f], [0] * (len(f) - 1)
    for k in range(m - 1, -1, -1):
        h = 1 << k
        for i in range(h):
            q[h - 1 + i] = (cur[i + h] - cur[i]) % R
        cur = [(cur[i] + point[k] * q[h - 1 + i]) % R for i in range(h)]
    return cur[0], q


def degrees(words, n_cols, n_consts, n_out):
    FM.validate(words, n_cols, n_consts, n_out)
    temps, out = {}, [0] * n_out
    for k in range(0, len(words), FM.WORDS):
        head, dst, a, b = words[k:k + 4]
        d = [1 if kind == FM.COL else temps[idx] if kind == FM.TEMP else 0 for kind, idx in (((head >> 16) & 0xFF, a), (head >> 24, b))]
        r = min(d[0] + d[1] if head & 0xFF == FM.MUL else max(d), (1 << 32) - 1)
        if (head >> 8) & 0xFF == FM.TEMP:
            temps[dst] = r
        else:
            out[dst] = r
    return out


def has_shift(words):
    return any((((words[k] >> 16) & 0xFF) == FM.COL and words[k + 4]) or ((words[k] >> 24) == FM.COL and words[k + 5]) for k in range(0, len(words), FM.WORDS))


def round_sums(words, n_cols, n_consts, n_out, cols, consts, n_eval):
    """sums[o][X] = sum_{i < h} P_o(v_0(i, X), ...), v_c(i, X) = lo + X (hi - lo): the program run (fr_program_model.run) over the h rows
    of the columns taken at X"""
    FM.validate(words, n_cols, n_consts, n_out)
    if has_shift(words) or not 1 <= n_eval <= MAX_EVAL or n_out * n_eval > MAX_ACC or len(cols) != n_cols:
        raise ShapeError("shift, n_eval or accumulators")
    n = len(cols[0]) if cols else 0
    if n < 2 or n & (n - 1) or any(len(c) != n for c in cols):
        raise ShapeError("n")
    h = n // 2
    sums = [[0] * n_eval for _ in range(n_out)]
    for X in range(n_eval):
        at_x = [[(c[i] + X * (c[i + h] - c[i])) % R for i in range(h)] for c in cols]
        outs = FM.run(words, n_cols, n_consts, n_out, at_x, consts, h)
        for o in range(n_out):
            sums[o][X] = sum(outs[o]) % R
    return sums


def interpolate(values, x):
    """the polynomial of degree < len(values) through (j, values[j]) at x"""
    acc = 0
    for j, v in enumerate(values):
        num, den = 1, 1
        for t in range(len(values)):
            if t != j:
                num, den = num * (x - t) % R, den * (j - t) % R
        acc = (acc + v * num * pow(den, -1, R)) % R
    return acc


def prove(words, n_cols, n_consts, n_out, cols, consts, challenge):
    """the rounds of kzg_amd.sumcheck.prove in integers: (round_sums, point, final_values)"""
    n = len(cols[0])
    m = n.bit_length() - 1
    n_eval = max(2, max(degrees(words, n_cols, n_consts, n_out)) + 1)
    cur, rounds, point = [list(c) for c in cols], [], [0] * m
    for k in range(m):
        s = round_sums(words, n_cols, n_consts, n_out, cur, consts, n_eval)
        rho = challenge(k, s) % R
        rounds.append(s)
        point[m - 1 - k] = rho
        cur = [bind(c, rho) for c in cur]
    return rounds, point, [c[0] % R for c in cur]


def verify(claims, rounds, point, finals, evaluate_fn):
    m = len(rounds)
    if len(point) != m:
        return False
    running = [c % R for c in claims]
    for k, sums in enumerate(rounds):
        for o, s in enumerate(sums):
            if (s[0] + s[1]) % R != running[o]:
                return False
            running[o] = interpolate(s, point[m - 1 - k])
    return [v % R for v in evaluate_fn(finals)] == running


# ---- programs the tests share -------------------------------------------------------------------------------------------------------
def product_program():
    """out0 = col0 col1: degree 2"""
    return FM.insn(FM.MUL, FM.OUT, 0, FM.COL, 0, FM.COL, 1), 2, 0, 1


def eq_gate_program():
    """out0 = eq (q_L a + q_R b + q_O c + q_M a b + q_C): columns a b c q_L q_R q_O q_M q_C eq, degree 4"""
    I, A, M_, C, T, O = FM.insn, FM.ADD, FM.MUL, FM.COL, FM.TEMP, FM.OUT
    words = (I(M_, T, 0, C, 3, C, 0) + I(M_, T, 1, C, 4, C, 1) + I(A, T, 0, T, 0, T, 1) + I(M_, T, 1, C, 5, C, 2) + I(A, T, 0, T, 0, T, 1) +
             I(M_, T, 1, C, 0, C, 1) + I(M_, T, 1, T, 1, C, 6) + I(A, T, 0, T, 0, T, 1) + I(A, T, 0, T, 0, C, 7) + I(M_, O, 0, T, 0, C, 8))
    return words, 9, 0, 1


def eq_gate_value(v):
    a, b, c, ql, qr, qo, qm, qc, e = v
    return e * (ql * a + qr * b + qo * c + qm * a * b + qc) % R
