"""A sumcheck prover over multilinear tables on the device, and its verifier in Python integers.

The claim: for every output o of a constraint program P (a kzg_amd.FrProgram without rotations), the sum of P_o over the hypercube
-- over all n = 2^m rows of the columns -- is claims[o].  Round k binds the TOP variable that is left (variable m - 1 - k): the
prover sends, per output, the values s(0) .. s(D) of the round polynomial (kzg_sumcheck_round), the challenge rho_k comes back, and
every column is folded with it in place (kzg_mle_bind).  After m rounds each column is one value, its multilinear extension at the
point (point[j] for variable j, so point[m - 1 - k] = rho_k), and the verifier ends by evaluating P there."""
from .api import R_MODULUS, DeviceBuffer, ReferencePanic, pack_scalars

R = R_MODULUS


def _view(buf, n):
    """the first n scalars of a DeviceBuffer as a DeviceBuffer that owns nothing"""
    v = DeviceBuffer.__new__(DeviceBuffer)
    v.engine, v.n, v.sfmt, v.ptr = buf.engine, n, buf.sfmt, buf.ptr
    return v


def prove(engine, program, cols, consts, challenge):
    """m rounds over the columns `cols` (n = 2^m scalars each: all lists of ints, or all DeviceBuffers of one format -- those are
    FOLDED IN PLACE and hold the final value in their first scalar afterwards).  program: a FrProgram; consts: ints in [0, R);
    challenge(round_index, sums) -> int in [0, R), sums being one list of degree + 1 ints per output.  Returns (round_sums, point,
    final_values): round_sums[k][o][X], the point (point[j] for variable j) and every column's value at it."""
    if not cols:
        raise ReferencePanic("sumcheck: no columns")
    own = []
    try:
        if isinstance(cols[0], DeviceBuffer):
            bufs = list(cols)
        else:
            for c in cols:
                blob = pack_scalars(c)
                own.append(engine.alloc_scalars(len(blob) // 32).upload(blob))
            bufs = own
        n = bufs[0].n
        if n < 1 or n & (n - 1) or any(b.n != n for b in bufs):
            raise ReferencePanic("sumcheck: every column holds the same power of two of scalars")
        m = n.bit_length() - 1
        n_eval = max(2, max(program.degrees()) + 1)    # s(0) and s(1) are checked even where the degree is 0
        round_sums, point = [], [0] * m
        for k in range(m):
            views = [_view(b, n >> k) for b in bufs]
            sums = program.sumcheck_round(views, consts, n_eval)
            rho = int(challenge(k, sums)) % R
            round_sums.append(sums)
            point[m - 1 - k] = rho
            engine.mle_bind(views, rho)
        finals = []
        for b in bufs:
            raw = b.download(1)
            finals.append(engine._scalar_from(raw, b.sfmt) % R)
        return round_sums, point, finals
    finally:
        for b in own:
            b.free()


def interpolate(values, x):
    """the polynomial of degree < len(values) through (j, values[j]), j = 0 .. len(values) - 1, at x"""
    d, x, acc = len(values), x % R, 0
    for j, v in enumerate(values):
        num, den = 1, 1
        for t in range(d):
            if t != j:
                num = num * (x - t) % R
                den = den * (j - t) % R
        acc = (acc + v * num * pow(den, -1, R)) % R
    return acc


def verify(claims, round_sums, point_challenges, final_values, evaluate):
    """True if the proof is accepted.  claims[o]: the claimed hypercube sum of output o; round_sums as prove returns them;
    point_challenges: the point of prove (the challenge of round k is point_challenges[m - 1 - k]; the caller re-derives them from
    the transcript); evaluate(final_values) -> one int per output, P at the point -- the caller obtains the columns' values at the
    point from the openings of its commitments.  Per round and output: s(0) + s(1) equals the running claim, which becomes s(rho)
    by interpolation over 0 .. D; at the end the running claims equal evaluate(final_values)."""
    m = len(round_sums)
    if len(point_challenges) != m:
        return False
    running = [c % R for c in claims]
    for k, sums in enumerate(round_sums):
        if len(sums) != len(running):
            return False
        rho = point_challenges[m - 1 - k] % R
        for o, s in enumerate(sums):
            if len(s) < 2 or (s[0] + s[1]) % R != running[o]:
                return False
            running[o] = interpolate(s, rho)
    return [v % R for v in evaluate(final_values)] == running
