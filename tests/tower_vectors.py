"""One vector set for the pairing tower (kzg_amd/csrc/tower.h), shared by the CPU test of the host build (tests/test_host_tower.py,
through ht_tower_op of tests/host_tower.cpp) and the GPU test of the device build (tests/test_gpu_tower.py, through kzg_test_tower).
For every op of include/kzg_mi355x_test.h: the records, and the expected bytes from oracle/pairing_model.py.  Where the model has no
function of the op's name the expected value is a one-line formula over the model's own functions:

  f12_mul_line(f, lam, cst, P)  = f12_mul(f, (cst, 0, -lam xP, (yP, 0), 0, 0))       the sparse element of tower.h:465-466 / P._line
  f12_exp_z(a)                  = f12_conj(f12_pow(a, |z|))
  g2_precompute_lines(Q)        = the 68 (lam, lam xT - yT) pairs of the model's Miller steps (model_lines below)

Every comparison is byte-exact: the Gt value is fixed by the final-exponentiation chain, which the model restates step by step.
vectors(name) -> [(record, expected, label)], built once per process; the aliasing forms are further records of the same op."""
import functools
import random
import struct

from oracle import kzg_model as M, pairing_model as P

Q, R = M.Q, M.R

# op ids and record sizes of include/kzg_mi355x_test.h (the CPU test checks them against the C table through ht_tower_shape)
OPS = ["f2_mul", "f2_sqr", "f2_inv", "f2_mul_fq", "f2_mul_xi", "f12_mul", "f12_sqr", "f12_cyclotomic_sqr", "f12_inv", "f12_frob",
       "f12_conj", "f12_is_one", "f12_exp_z", "f12_mul_line", "g2_add", "g2_double", "g2_mul", "g2_on_curve", "g2_precompute_lines",
       "miller_loop", "final_exponentiation", "pairing_product_is_one"]
OP = {name: i for i, name in enumerate(OPS)}
SHAPES = {"f2_mul": (196, 96), "f2_sqr": (100, 96), "f2_inv": (100, 96), "f2_mul_fq": (148, 96), "f2_mul_xi": (100, 96),
          "f12_mul": (1156, 576), "f12_sqr": (580, 576), "f12_cyclotomic_sqr": (580, 576), "f12_inv": (580, 576), "f12_frob": (584, 576),
          "f12_conj": (580, 576), "f12_is_one": (576, 4), "f12_exp_z": (580, 576), "f12_mul_line": (864, 576), "g2_add": (388, 192),
          "g2_double": (196, 192), "g2_mul": (224, 192), "g2_on_curve": (192, 4), "g2_precompute_lines": (192, 13056),
          "miller_loop": (1160, 576), "final_exponentiation": (576, 576), "pairing_product_is_one": (1160, 4)}
ALIAS = ["r distinct", "r is a", "r is b", "a is b, r distinct", "r, a, b one object"]


# ---- encodings ------------------------------------------------------------------------------------------------------------------
def fqb(x):
    return x.to_bytes(48, "little")


def f2b(a):
    return fqb(a[0]) + fqb(a[1])


def f12b(a):
    return b"".join(f2b(c) for c in a)


def g1b(p):
    return bytes(96) if p is None else fqb(p[0]) + fqb(p[1])


def g2b(p):
    return bytes(192) if p is None else f2b(p[0]) + f2b(p[1])


def u32(v):
    return struct.pack("<I", v)


def first_difference(got, want):
    """(index of the first differing 48-byte Fq coefficient -- or 4-byte word of a verdict --, got, want) or None"""
    step = 48 if len(want) >= 48 else 4
    for k in range(0, len(want), step):
        if got[k:k + step] != want[k:k + step]:
            return k // step, got[k:k + step][::-1].hex(), want[k:k + step][::-1].hex()
    return None


def check(name, results):
    """results[i] = the bytes an implementation gave for record i of vectors(name): fails naming the record, its aliasing form and
    the first differing coefficient"""
    vec = vectors(name)
    assert len(results) == len(vec)
    for i, (got, (_, want, label)) in enumerate(zip(results, vec)):
        if got != want:
            k, g, w = first_difference(got, want)
            raise AssertionError("%s: record %d (%s): coefficient %d is 0x%s, expected 0x%s" % (name, i, label, k, g, w))


# ---- operands -------------------------------------------------------------------------------------------------------------------
FQ_EDGE = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2]
F2_EDGE = [(a, b) for a in FQ_EDGE for b in FQ_EDGE]     # includes c0 = 0, c1 = 0, both
F12_ZERO = (P.F2_ZERO,) * 6
F12_MINUS_ONE = ((Q - 1, 0),) + (P.F2_ZERO,) * 5


def rf2(rng):
    return (rng.randrange(Q), rng.randrange(Q))


def rf12(rng):
    return tuple(rf2(rng) for _ in range(6))


def f12_with(base, pos, value):
    """base with its Fq coefficient number pos (0..11: coefficient pos // 2 of w, component pos % 2) replaced"""
    c = [list(x) for x in base]
    c[pos // 2][pos % 2] = value % Q
    return tuple(tuple(x) for x in c)


@functools.lru_cache(maxsize=None)
def f12_elements():
    """0, 1, -1; a single non-zero Fq coefficient in each of the 12 positions; two elements of the Fq6 subfield (c1 = 0: the odd
    powers of w vanish); 16 random elements.  The first 19 are the edge set."""
    rng = random.Random(0x7012)
    el = [F12_ZERO, P.F12_ONE, F12_MINUS_ONE]
    el += [f12_with(F12_ZERO, pos, rng.randrange(1, Q)) for pos in range(12)]
    el += [tuple(rf2(rng) if k % 2 == 0 else P.F2_ZERO for k in range(6)) for _ in range(2)]
    el += [rf12(rng) for _ in range(16)]
    return el


N_F12_EDGE = 19


def model_lines(S):
    """g2_precompute_lines: (lam, lam xT - yT) of every doubling and addition step of the model's Miller loop for S, in loop order"""
    out = []
    if S is None:
        return [P.F2_ZERO] * (2 * 68)
    T = S
    for bit in bin(P.BLS_Z_ABS)[3:]:
        lam = P.f2_mul(P.f2_scale(P.f2_sqr(T[0]), 3), P.f2_inv(P.f2_scale(T[1], 2)))
        out += [lam, P._line(lam, T, (0, 0))[0]]
        x3 = P.f2_sub(P.f2_sqr(lam), P.f2_scale(T[0], 2))
        T = (x3, P.f2_sub(P.f2_mul(lam, P.f2_sub(T[0], x3)), T[1]))
        if bit == "1":
            lam = P.f2_mul(P.f2_sub(S[1], T[1]), P.f2_inv(P.f2_sub(S[0], T[0])))
            out += [lam, P._line(lam, T, (0, 0))[0]]
            x3 = P.f2_sub(P.f2_sub(P.f2_sqr(lam), T[0]), S[0])
            T = (x3, P.f2_sub(P.f2_mul(lam, P.f2_sub(T[0], x3)), T[1]))
    assert len(out) == 2 * 68
    return out


# ---- Miller loop, final exponentiation, product check: one shared set -------------------------------------------------------------
def pairs_record(pairs, mask):
    np_ = len(pairs)
    pad = [(None, None)] * (4 - np_)
    return u32(np_) + u32(mask) + b"".join(g1b(p) for p, _ in pairs + pad) + b"".join(g2b(q) for _, q in pairs + pad)


@functools.lru_cache(maxsize=None)
def pairing_set():
    """-> (records, miller, final): records = [(pairs, mask, label)], miller / final = {tuple(pairs): model value}.

    Base sets of np = 1..4 pairs ([a_i]G, [b_i]H), balanced for np >= 2 (sum a_i b_i = 0 mod r: the product is 1) under every route
    mask; an identity P or Q in every position with that pair's mask bit set (all others clear) and clear (all others set), for
    np = 1, 2, 4; the same pair twice; the generators; and the balanced sets off by one."""
    rng = random.Random(0x7013)
    bs = [rng.randrange(1, R) for _ in range(3)] + [R - 1]
    Hs = [P.g2_mul(P.G2, b) for b in bs]
    g1 = functools.lru_cache(maxsize=None)(lambda a: M.g1_mul(M.G1, a % R))
    base, off = {}, {}
    for np_ in range(1, 5):
        a = [rng.randrange(1, R) for _ in range(np_)]
        if np_ > 1:
            a[-1] = -sum(x * b for x, b in zip(a[:-1], bs)) * pow(bs[np_ - 1], -1, R) % R
            assert sum(x * b for x, b in zip(a, bs)) % R == 0
            off[np_] = [(g1(x), h) for x, h in zip(a[:-1], Hs)] + [(g1(a[-1] + 1), Hs[np_ - 1])]
        base[np_] = [(g1(x), h) for x, h in zip(a, Hs)]
    records = []
    for np_ in range(1, 5):
        for mask in range(1 << np_):
            records.append((base[np_], mask, "np %d, %s" % (np_, "balanced" if np_ > 1 else "one pair")))
    for np_ in (1, 2, 4):
        full = (1 << np_) - 1
        for pos in range(np_):
            for which in (0, 1):
                pr = list(base[np_])
                pr[pos] = (None, pr[pos][1]) if which == 0 else (pr[pos][0], None)
                for mask in (1 << pos, full ^ (1 << pos)):
                    records.append((pr, mask, "np %d, identity %s in pair %d" % (np_, "PQ"[which], pos)))
    twice = [base[1][0], base[1][0]]
    records += [(twice, mask, "the same pair twice") for mask in range(4)]
    records += [([(M.G1, P.G2)], mask, "the generators") for mask in range(2)]
    records += [([(M.G1, P.G2), (M.g1_neg(M.G1), P.G2)], mask, "the generators and the negation") for mask in (0, 3)]
    for np_ in (2, 3, 4):
        records += [(off[np_], mask, "np %d, off by one" % np_) for mask in (0, (1 << np_) - 1)]
    records = [(tuple(pr), mask, "%s, route mask %s" % (label, bin(mask))) for pr, mask, label in records]
    miller, final = {}, {}
    for pr, _, _ in records:
        if pr not in miller:
            miller[pr] = P.miller_loop(list(pr))
            final[pr] = P.final_exponentiation(miller[pr])
    # the integer reference of the verdicts: the product is 1 exactly when the exponents cancel (or every pair has an identity member)
    for np_ in (2, 3, 4):
        assert final[tuple(base[np_])] == P.F12_ONE and final[tuple(off[np_])] != P.F12_ONE
    assert final[tuple(base[1])] != P.F12_ONE and final[tuple(twice)] != P.F12_ONE
    return records, miller, final


@functools.lru_cache(maxsize=None)
def cyclotomic_elements():
    """1 and the final exponentiations of 8 distinct Miller values (genuine elements of the cyclotomic subgroup)"""
    _, _, final = pairing_set()
    out = [P.F12_ONE]
    for v in final.values():
        if v not in out:
            out.append(v)
        if len(out) == 9:
            break
    assert len(out) == 9
    return out


def _bad(name, offset, *words):
    rec = bytearray(SHAPES[name][0])
    rec[offset:offset + 4 * len(words)] = struct.pack("<%dI" % len(words), *words)
    return name, bytes(rec)


# records of the right size whose alias / power / np / mask word is out of range: refused (KZG_ERR_SHAPE) before anything runs
BAD_RECORDS = [_bad("f2_mul", 192, 5), _bad("f2_sqr", 96, 2), _bad("f2_inv", 96, 0xffffffff), _bad("f2_mul_fq", 144, 2),
               _bad("f2_mul_xi", 96, 2), _bad("f12_mul", 1152, 5), _bad("f12_sqr", 576, 2), _bad("f12_cyclotomic_sqr", 576, 2),
               _bad("f12_inv", 576, 2), _bad("f12_conj", 576, 2), _bad("f12_exp_z", 576, 2), _bad("f12_frob", 576, 0, 0),
               _bad("f12_frob", 576, 3, 0), _bad("f12_frob", 576, 1, 2), _bad("g2_add", 384, 5), _bad("g2_double", 192, 2),
               _bad("miller_loop", 0, 0, 0), _bad("miller_loop", 0, 5, 0), _bad("miller_loop", 0, 2, 4),
               _bad("pairing_product_is_one", 0, 0, 0), _bad("pairing_product_is_one", 0, 5, 1), _bad("pairing_product_is_one", 0, 1, 2)]


# ---- the vectors ----------------------------------------------------------------------------------------------------------------
def _unary(elements, fn, extra=lambda a: b""):
    return [(f12b(a) + extra(a) + u32(al), f12b(fn(a)), "element %d, %s" % (i, ALIAS[al])) for i, a in enumerate(elements) for al in (0, 1)]


@functools.lru_cache(maxsize=None)
def vectors(name):
    rng = random.Random(0x7000 + OP[name])
    out = []
    if name == "f2_mul":
        pairs = [(a, b) for a in F2_EDGE for b in F2_EDGE] + [(rf2(rng), rf2(rng)) for _ in range(64)]
        for a, b in pairs:
            out += [(f2b(a) + f2b(b) + u32(al), f2b(P.f2_mul(a, b)), ALIAS[al]) for al in (0, 1, 2)]
        for a in F2_EDGE + [rf2(rng) for _ in range(64)]:
            out += [(f2b(a) + f2b(rf2(rng)) + u32(al), f2b(P.f2_mul(a, a)), ALIAS[al]) for al in (3, 4)]
    elif name in ("f2_sqr", "f2_inv", "f2_mul_xi"):
        fn = {"f2_sqr": P.f2_sqr, "f2_inv": P.f2_inv, "f2_mul_xi": lambda a: P.f2_mul(a, P.XI)}[name]
        for a in F2_EDGE + [rf2(rng) for _ in range(64)]:
            if name == "f2_inv" and a == P.F2_ZERO:
                continue
            out += [(f2b(a) + u32(al), f2b(fn(a)), ALIAS[al]) for al in (0, 1)]
    elif name == "f2_mul_fq":
        for a, k in [(a, k) for a in F2_EDGE for k in FQ_EDGE] + [(rf2(rng), rng.randrange(Q)) for _ in range(64)]:
            out += [(f2b(a) + fqb(k) + u32(al), f2b(P.f2_scale(a, k)), ALIAS[al]) for al in (0, 1)]
    elif name == "f12_mul":
        el = f12_elements()
        for i, a in enumerate(el[:N_F12_EDGE]):
            for j, b in enumerate(el[:N_F12_EDGE]):
                out.append((f12b(a) + f12b(b) + u32(0), f12b(P.f12_mul(a, b)), "elements %d, %d, %s" % (i, j, ALIAS[0])))
        for i, a in enumerate(el):
            j = (5 * i + 1) % len(el)
            for al in range(5):
                want = P.f12_mul(a, el[j] if al < 3 else a)
                out.append((f12b(a) + f12b(el[j]) + u32(al), f12b(want), "elements %d, %d, %s" % (i, j, ALIAS[al])))
    elif name == "f12_sqr":
        out = _unary(f12_elements(), P.f12_sqr)
    elif name == "f12_inv":
        out = _unary([a for a in f12_elements() if a != F12_ZERO], P.f12_inv)
    elif name == "f12_conj":
        out = _unary(f12_elements(), P.f12_conj)
    elif name == "f12_frob":
        for power, fn in ((1, P.f12_frob), (2, P.f12_frob2)):
            out += _unary(f12_elements(), fn, lambda a: u32(power))
    elif name == "f12_cyclotomic_sqr":
        for a in cyclotomic_elements():
            assert P.f12_sqr(a) == P.f12_cyclotomic_sqr(a)
        out = _unary(cyclotomic_elements(), P.f12_sqr)
    elif name == "f12_exp_z":
        out = _unary(cyclotomic_elements(), lambda a: P.f12_conj(P.f12_pow(a, P.BLS_Z_ABS)))
    elif name == "f12_is_one":
        cases = [(P.F12_ONE, "1"), (F12_MINUS_ONE, "-1"), (F12_ZERO, "0"), (f12_with(P.F12_ONE, 0, 1 + (1 << 352)), "1 + 2^352 in c0.c0.c0")]
        for pos in range(12):
            for d in (1, -1):
                cases.append((f12_with(P.F12_ONE, pos, (1 if pos == 0 else 0) + d), "1 with coefficient %d changed by %+d" % (pos, d)))
        out = [(f12b(a), u32(1 if a == P.F12_ONE else 0), label) for a, label in cases]
        assert sum(want == u32(1) for _, want, _ in out) == 1
    elif name == "f12_mul_line":
        pts = [M.G1, M.g1_mul(M.G1, rng.randrange(1, R))]
        for fi, f in enumerate((rf12(rng), P.F12_ONE)):
            for lam, cst in [(rf2(rng), rf2(rng)), (P.F2_ZERO, rf2(rng)), (rf2(rng), P.F2_ZERO), (P.F2_ZERO, P.F2_ZERO)]:
                for pi, pt in enumerate(pts):
                    line = (cst, P.F2_ZERO, P.f2_neg(P.f2_scale(lam, pt[0])), (pt[1], 0), P.F2_ZERO, P.F2_ZERO)
                    label = "f %s, lam %s, cst %s, P %s" % (("random", "1")[fi], "0" if lam == P.F2_ZERO else "random",
                                                             "0" if cst == P.F2_ZERO else "random", ("the generator", "random")[pi])
                    out.append((f12b(f) + f2b(lam) + f2b(cst) + g1b(pt), f12b(P.f12_mul(f, line)), label))
    elif name == "g2_add":
        a, c = P.g2_mul(P.G2, 11), P.g2_mul(P.G2, 31)
        names = ["distinct", "equal", "inverse", "Q the identity", "P the identity", "both the identity"]
        for (x, y), nm in zip([(a, c), (a, a), (a, P.g2_neg(a)), (a, None), (None, c), (None, None)], names):
            out += [(g2b(x) + g2b(y) + u32(al), g2b(P.g2_add(x, y)), "%s, %s" % (nm, ALIAS[al])) for al in (0, 1, 2)]
            out += [(g2b(x) + g2b(y) + u32(al), g2b(P.g2_add(x, x)), "%s, %s" % (nm, ALIAS[al])) for al in (3, 4)]
    elif name == "g2_double":
        for x in (P.G2, P.g2_mul(P.G2, 11), None):
            out += [(g2b(x) + u32(al), g2b(P.g2_add(x, x)), ALIAS[al]) for al in (0, 1)]
    elif name == "g2_mul":
        ks = [0, 1, 2, R - 1, R, (1 << 256) - 1, rng.randrange(1 << 256)]
        for x in (P.G2, P.g2_mul(P.G2, 11), None):
            out += [(g2b(x) + k.to_bytes(32, "little"), g2b(P.g2_mul(x, k % R) if x else None), "k = %#x" % k) for k in ks]
    elif name == "g2_on_curve":
        a = P.g2_mul(P.G2, 11)
        for x in (P.G2, a, None, (P.G2[0], P.f2_add(P.G2[1], (1, 0))), (a[1], a[0]), (P.G2[0], P.f2_add(P.G2[1], (0, 1))), ((0, 0), (1, 0))):
            out.append((g2b(x), u32(1 if P.g2_is_on_curve(x) else 0), "point %d" % len(out)))
    elif name == "g2_precompute_lines":
        for x, label in ((P.G2, "the generator"), (P.g2_mul(P.G2, rng.randrange(1, R)), "random"), (None, "the identity")):
            out.append((g2b(x), b"".join(f2b(c) for c in model_lines(x)), label))
    elif name == "miller_loop":
        records, miller, _ = pairing_set()
        out = [(pairs_record(list(pr), mask), f12b(miller[pr]), label) for pr, mask, label in records]
    elif name == "final_exponentiation":
        _, miller, final = pairing_set()
        out = [(f12b(P.F12_ONE), f12b(P.final_exponentiation(P.F12_ONE)), "the value 1")]
        out += [(f12b(miller[pr]), f12b(final[pr]), "Miller value %d" % i) for i, pr in enumerate(miller)]
    elif name == "pairing_product_is_one":
        records, _, final = pairing_set()
        out = [(pairs_record(list(pr), mask), u32(1 if final[pr] == P.F12_ONE else 0), label) for pr, mask, label in records]
    else:
        raise KeyError(name)
    for rec, want, _ in out:
        assert (len(rec), len(want)) == SHAPES[name], (name, len(rec), len(want))
    return out
