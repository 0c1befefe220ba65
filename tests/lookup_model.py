"""Python-integer model of kzg_lookup_count and kzg_logup_terms (kzg_amd/csrc/lookup.hip).  Any integer counts as its residue modulo r."""
from oracle import kzg_model as M

R = M.R
NONE = 0xFFFFFFFF


def owners(table):
    """{residue: the lowest row that holds it}"""
    own = {}
    for i, t in enumerate(table):
        own.setdefault(t % R, i)
    return own


def multiplicities(table, values):
    """one vector: (mult per table row -- the number of values the row owns, 0 at rows that own nothing --, the owner of every value
    or NONE, the number of values that are not in the table, the position of the first of them or None)"""
    own = owners(table)
    mult, idx, missing, first = [0] * len(table), [], 0, None
    for j, v in enumerate(values):
        i = own.get(v % R)
        if i is None:
            idx.append(NONE)
            missing += 1
            if first is None:
                first = j
        else:
            idx.append(i)
            mult[i] += 1
    return mult, idx, missing, first


def logup_terms(values, table, mult, beta):
    """one vector: values is a list of t columns of n values; table, mult: n values each, or both None.  (out, zero_den); all zero
    where a denominator is zero"""
    n = len(table) if table is not None else len(values[0])
    dens = [(beta + x) % R for col in values for x in col] + ([(beta + x) % R for x in table] if table is not None else [])
    if any(d == 0 for d in dens):
        return [0] * n, 1
    out = []
    for i in range(n):
        acc = sum(pow((beta + col[i]) % R, -1, R) for col in values)
        if table is not None:
            acc -= mult[i] * pow((beta + table[i]) % R, -1, R)
        out.append(acc % R)
    return out, 0
