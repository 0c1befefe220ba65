"""Expressions over columns of Fr, compiled to the words of kzg_fr_program_setup (include/kzg_mi355x.h).  Host-only Python.

    from kzg_amd import frp
    a, b, c = frp.col(0), frp.col(1), frp.col(2)
    gate = frp.col(3) * a + frp.col(4) * b + frp.col(5) * c + frp.col(6) * a * b + frp.col(7)
    prog = frp.compile([gate * frp.col(8)])          # column 8: the periodic 1 / Z_H
    plan = engine.fr_program(prog)

col(c, shift) is element (i + shift) mod len of column c at row i, const(k) the k-th scalar of the run; + - * and positive integer
powers (square and multiply) combine them.  compile(outputs) emits every common sub-expression once (a + b and b + a are one
expression), evaluates the operand that needs more temporaries first, allocates the 16 temporaries by liveness and raises FrpError,
naming the expression, where more than 16 values are alive at once."""
from ._lib import FRP_ADD, FRP_COL, FRP_CONST, FRP_MAX_TEMPS, FRP_MUL, FRP_OUT, FRP_SUB, FRP_TEMP, FRP_WORDS

_SYMBOL = {FRP_ADD: "+", FRP_SUB: "-", FRP_MUL: "*"}


class FrpError(ValueError):
    """an expression that cannot be compiled"""


class Expr:
    __slots__ = ("op", "a", "b")     # a leaf: op = "col" (a = column, b = shift) or "const" (a = index); else op = FRP_*, a and b Exprs

    def __init__(self, op, a, b=None):
        self.op, self.a, self.b = op, a, b

    def is_leaf(self):
        return self.op in ("col", "const")

    def _bin(self, op, other, swap=False):
        if not isinstance(other, Expr):
            raise TypeError("operands are expressions: a scalar of the run is const(k)")
        return Expr(op, other, self) if swap else Expr(op, self, other)

    def __add__(self, o):
        return self._bin(FRP_ADD, o)

    def __sub__(self, o):
        return self._bin(FRP_SUB, o)

    def __mul__(self, o):
        return self._bin(FRP_MUL, o)

    def __pow__(self, e):
        if not isinstance(e, int) or isinstance(e, bool) or e < 1:
            raise FrpError("a power is a positive integer")
        acc, base = None, self
        while True:
            if e & 1:
                acc = base if acc is None else acc * base
            e >>= 1
            if not e:
                return acc
            base = base * base

    def __repr__(self):
        return _text(self, 160)


def col(c, shift=0):
    if c < 0 or not -(1 << 31) <= shift < (1 << 31):
        raise FrpError("a column index is >= 0 and a shift an int32")
    return Expr("col", int(c), int(shift))


def const(k):
    if k < 0:
        raise FrpError("a const index is >= 0")
    return Expr("const", int(k))


def _text(e, limit):
    """the expression as text, cut off at about `limit` characters (iterative: expressions may be deep)"""
    out, stack, size = [], [e], 0
    while stack and size < limit:
        x = stack.pop()
        if isinstance(x, str):
            s = x
        elif x.op == "col":
            s = "col%d" % x.a if not x.b else "col%d[%+d]" % (x.a, x.b)
        elif x.op == "const":
            s = "const%d" % x.a
        else:
            stack += [")", x.b, " %s " % _SYMBOL[x.op], x.a, "("]
            continue
        out.append(s)
        size += len(s)
    return "".join(out) + (" ..." if stack else "")


class Compiled:
    """the words of a program and the sizes kzg_fr_program_setup takes"""

    def __init__(self, words, n_cols, n_consts, n_out, n_temps, n_mul):
        self.words, self.n_cols, self.n_consts, self.n_out, self.n_temps, self.n_mul = words, n_cols, n_consts, n_out, n_temps, n_mul
        self.n_insns = len(words) // FRP_WORDS


def insn(op, dst_kind, dst, a_kind, a, b_kind, b, a_shift=0, b_shift=0):
    """the six words of one instruction"""
    return [op | dst_kind << 8 | a_kind << 16 | b_kind << 24, dst, a, b, a_shift & 0xFFFFFFFF, b_shift & 0xFFFFFFFF]


def compile(outputs):  # noqa: A001 (the name the expressions' users expect)
    outputs = list(outputs)
    if not outputs or len(outputs) > 64:
        raise FrpError("1 to 64 outputs")
    # the DAG: structurally equal expressions are one node.  nodes[k] = ("col", c, s) | ("const", k) | (op, node a, node b)
    nodes, index, text_of, memo = [], {}, {}, {}

    def intern(root):
        stack = [root]
        while stack:
            e = stack[-1]
            if id(e) in memo:
                stack.pop()
                continue
            if e.is_leaf():
                key = (e.op, e.a, e.b)
            else:
                pending = [x for x in (e.a, e.b) if id(x) not in memo]
                if pending:
                    stack += pending
                    continue
                ka, kb = memo[id(e.a)], memo[id(e.b)]
                if e.op != FRP_SUB and ka > kb:
                    ka, kb = kb, ka
                key = (e.op, ka, kb)
            if key not in index:
                index[key] = len(nodes)
                nodes.append(key)
                text_of[index[key]] = e
            memo[id(e)] = index[key]
            stack.pop()
        return memo[id(root)]

    roots = [intern(e) for e in outputs]
    for o, r in enumerate(roots):
        if nodes[r][0] in ("col", "const"):
            raise FrpError("output %d is %r: an output is the result of an operation" % (o, text_of[r]))
    leaf = [n[0] in ("col", "const") for n in nodes]
    # operand references still to come, per node; temporaries an expression needs on its own (leaves take none: an operand of an
    # instruction may be a column or a const), for the order of evaluation
    refs, need = [0] * len(nodes), [0] * len(nodes)
    for k, n in enumerate(nodes):          # (children have lower numbers than their parents)
        if leaf[k]:
            continue
        refs[n[1]] += 1
        refs[n[2]] += 1
        la, lb = need[n[1]], need[n[2]]
        need[k] = max(1, la + 1 if la == lb and n[1] != n[2] and la else max(la, lb))
    out_of = {}
    for o, r in enumerate(roots):
        out_of.setdefault(r, []).append(o)
    words, temp_of, free, state = [], {}, list(range(FRP_MAX_TEMPS)), {"peak": 0, "mul": 0}

    def operand(k):
        n = nodes[k]
        if n[0] == "col":
            return FRP_COL, n[1], n[2]
        if n[0] == "const":
            return FRP_CONST, n[1], 0
        return FRP_TEMP, temp_of[k], 0

    def emit(k):
        op, a, b = nodes[k]
        (ak, ai, ash), (bk, bi, bsh) = operand(a), operand(b)
        outs = out_of.get(k, [])
        for o in outs[:-1] if not refs[k] else outs:     # (before the temporary: it may take the place of a source)
            words.extend(insn(op, FRP_OUT, o, ak, ai, bk, bi, ash, bsh))
            state["mul"] += op == FRP_MUL
        for x in (a, b):
            refs[x] -= 1
            if not leaf[x] and refs[x] == 0 and x in temp_of:
                free.append(temp_of.pop(x))
        if refs[k]:
            if not free:
                raise FrpError("more than %d values are alive at once at %r" % (FRP_MAX_TEMPS, text_of[k]))
            free.sort()
            temp_of[k] = free.pop(0)
            state["peak"] = max(state["peak"], temp_of[k] + 1)
            words.extend(insn(op, FRP_TEMP, temp_of[k], ak, ai, bk, bi, ash, bsh))
        else:
            words.extend(insn(op, FRP_OUT, outs[-1], ak, ai, bk, bi, ash, bsh))
        state["mul"] += op == FRP_MUL

    done = set()
    for r in roots:
        stack = [r]
        while stack:
            k = stack[-1]
            if k in done or leaf[k]:
                stack.pop()
                continue
            kids = [x for x in (nodes[k][1], nodes[k][2]) if not leaf[x] and x not in done]
            if kids:
                kids.sort(key=lambda x: need[x])      # the heavier operand on top of the stack: evaluated first
                stack += kids
                continue
            emit(k)
            done.add(k)
            stack.pop()
    n_cols = max([n[1] + 1 for n in nodes if n[0] == "col"], default=0)
    n_consts = max([n[1] + 1 for n in nodes if n[0] == "const"], default=0)
    return Compiled(words, n_cols, n_consts, len(outputs), state["peak"], state["mul"])
