"""Python-integer interpreter of the words of kzg_fr_program_setup / kzg_fr_program_run (kzg_amd/csrc/fr_program.hip).  It applies the
validation rules of the header and raises ShapeError wherever the library returns KZG_ERR_SHAPE.  Any integer counts as its residue
modulo r."""
from oracle import kzg_model as M

R = M.R
ADD, SUB, MUL = 0, 1, 2
COL, CONST, TEMP, OUT = 0, 1, 2, 3
WORDS, MAX_TEMPS = 6, 16
MAX_N, MAX_INSNS, MAX_COLS, MAX_CONSTS, MAX_OUT = 1 << 28, 65536, 4096, 4096, 64


class ShapeError(Exception):
    """KZG_ERR_SHAPE"""


def insn(op, dst_kind, dst, a_kind, a, b_kind, b, a_shift=0, b_shift=0):
    return [op | dst_kind << 8 | a_kind << 16 | b_kind << 24, dst, a, b, a_shift & 0xFFFFFFFF, b_shift & 0xFFFFFFFF]


def _signed(w):
    return w - (1 << 32) if w >> 31 else w


def validate(words, n_cols, n_consts, n_out):
    """the checks of kzg_fr_program_setup; (n_insns, n_temps, n_mul)"""
    if len(words) % WORDS or not 0 < len(words) // WORDS <= MAX_INSNS:
        raise ShapeError("n_insns")
    if n_cols > MAX_COLS or n_consts > MAX_CONSTS or not 0 < n_out <= MAX_OUT:
        raise ShapeError("sizes")
    temps, outs, n_temps, n_mul = set(), set(), 0, 0
    for k in range(0, len(words), WORDS):
        head, dst, a, b, sa, sb = words[k:k + WORDS]
        op, dk = head & 0xFF, (head >> 8) & 0xFF
        if op not in (ADD, SUB, MUL):
            raise ShapeError("op")
        for kind, idx, sh in (((head >> 16) & 0xFF, a, sa), (head >> 24, b, sb)):
            if kind == COL:
                if idx >= n_cols:
                    raise ShapeError("column index")
            elif kind == CONST:
                if idx >= n_consts:
                    raise ShapeError("const index")
            elif kind == TEMP:
                if idx >= MAX_TEMPS or idx not in temps:
                    raise ShapeError("temp index, or read before written")
            else:
                raise ShapeError("source kind")
            if kind != COL and sh:
                raise ShapeError("shift on a non-column")
        if dk == TEMP:
            if dst >= MAX_TEMPS:
                raise ShapeError("temp index")
            temps.add(dst)
            n_temps = max(n_temps, dst + 1)
        elif dk == OUT:
            if dst >= n_out or dst in outs:
                raise ShapeError("output index, or written twice")
            outs.add(dst)
        else:
            raise ShapeError("destination kind")
        n_mul += op == MUL
    if len(outs) != n_out:
        raise ShapeError("an output is never written")
    return len(words) // WORDS, n_temps, n_mul


def run(words, n_cols, n_consts, n_out, cols, consts, n):
    """the outputs of kzg_fr_program_run as lists of n residues; cols: lists of ints (any size of int counts as its residue)"""
    validate(words, n_cols, n_consts, n_out)
    if not 0 < n <= MAX_N or len(cols) != n_cols or len(consts) != n_consts:
        raise ShapeError("n")
    for c in cols:
        ln = len(c)
        if ln == 0 or (ln != n and (ln & (ln - 1) or n % ln)):
            raise ShapeError("column length")
    if any(not 0 <= k < R for k in consts):
        raise ShapeError("a const is not below r")
    outs = [[0] * n for _ in range(n_out)]
    for i in range(n):
        temps = {}
        for k in range(0, len(words), WORDS):
            head, dst, a, b, sa, sb = words[k:k + WORDS]
            v = []
            for kind, idx, sh in (((head >> 16) & 0xFF, a, sa), (head >> 24, b, sb)):
                if kind == COL:
                    v.append(cols[idx][(i + _signed(sh)) % len(cols[idx])] % R)
                elif kind == CONST:
                    v.append(consts[idx])
                else:
                    v.append(temps[idx])
            op = head & 0xFF
            d = (v[0] + v[1] if op == ADD else v[0] - v[1] if op == SUB else v[0] * v[1]) % R
            if (head >> 8) & 0xFF == TEMP:
                temps[dst] = d
            else:
                outs[dst][i] = d
    return outs


def rejected_programs():
    """(name, words, n_cols, n_consts, n_out) of programs kzg_fr_program_setup refuses: the header's list"""
    I, A, M_, C, K, T, O = insn, ADD, MUL, COL, CONST, TEMP, OUT
    ok = I(A, O, 0, C, 0, C, 0)
    return [
        ("no instruction", [], 1, 0, 1),
        ("too many instructions", I(A, T, 0, C, 0, C, 0) * 65536 + ok, 1, 0, 1),
        ("too many columns", ok, 4097, 0, 1),
        ("too many consts", ok, 1, 4097, 1),
        ("too many outputs", ok, 1, 0, 65),
        ("no output", I(A, T, 0, C, 0, C, 0), 1, 0, 0),
        ("unknown op", I(3, O, 0, C, 0, C, 0), 1, 0, 1),
        ("unknown source kind", I(A, O, 0, 4, 0, C, 0), 1, 0, 1),
        ("unknown destination kind", I(A, 7, 0, C, 0, C, 0), 1, 0, 1),
        ("an output as a source", I(A, O, 0, C, 0, C, 0) + I(A, O, 1, O, 0, C, 0), 1, 0, 2),
        ("a column as a destination", I(A, C, 0, C, 0, C, 0) + ok, 1, 0, 1),
        ("a const as a destination", I(A, K, 0, C, 0, C, 0) + ok, 1, 1, 1),
        ("column index out of range", I(A, O, 0, C, 1, C, 0), 1, 0, 1),
        ("const index out of range", I(A, O, 0, C, 0, K, 2), 1, 2, 1),
        ("output index out of range", I(A, O, 1, C, 0, C, 0), 1, 0, 1),
        ("temp index 16 as a destination", I(A, T, 16, C, 0, C, 0) + ok, 1, 0, 1),
        ("temp index 16 as a source", I(A, T, 15, C, 0, C, 0) + I(A, O, 0, T, 16, C, 0), 1, 0, 1),
        ("a temp read before it is written", I(A, O, 0, T, 0, C, 0) + I(A, T, 0, C, 0, C, 0), 1, 0, 1),
        ("a temp squared before it is written", I(M_, T, 0, T, 0, T, 0) + ok, 1, 0, 1),
        ("a shift on a const", I(A, O, 0, C, 0, K, 0, 0, 1), 1, 1, 1),
        ("a shift on a temp", I(A, T, 0, C, 0, C, 0) + I(A, O, 0, T, 0, C, 0, -1, 0), 1, 0, 1),
        ("an output written twice", ok + ok, 1, 0, 1),
        ("an output never written", ok, 1, 0, 2),
    ]
