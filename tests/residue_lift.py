"""The one generator of tests/test_gpu_scalar_residues.py: representatives >= r of given residues.

include/kzg_mi355x.h: "scalars in KZG_FR_CANONICAL_LE_32 that are >= r are taken mod r".  lift() turns canonical values (< r) into
other 256-bit words of the same residue classes; the tests feed those to a call and expect the bytes the canonical input gives.
r is about 0.45 * 2^256, so v + r always fits in 32 bytes and v + 2r fits for v < 2^256 - 2r (about a tenth of all residues)."""
from oracle import kzg_model as M

R = M.R
TOP = 1 << 256
T = (TOP - 1) % R                      # the residue of the all-ones word: 2^256 - 1 = 2r + T
MODES = ("all", "sparse", "edges")
# base(): the residues planted at the head of every base vector, and what "edges" makes of them (position by position)
PLANTED = (0, 0, 1, 1, R - 1, T)
EDGE_WORDS = (R, 2 * R, R + 1, 2 * R + 1, 2 * R - 1, TOP - 1)
SMALL = TOP - 2 * R                    # residues below this have two lifted representatives (v + r and v + 2r)


def lift_one(v):
    """the largest representative of v below 2^256: v + 2r where that fits, else v + r"""
    return v + 2 * R if v + 2 * R < TOP else v + R


def lift(values, mode):
    """values: canonical ints (< r).  Returns ints of the same residues below 2^256:
      "all"     every element lifted (lift_one);
      "sparse"  every 7th element (index 0, 7, 14, ..) lifted, the rest untouched: binary operations see mixed operands;
      "edges"   "sparse", and positions 0 .. 5 take v + r (even position) or v + 2r (odd position, where it fits): on a base() vector
                these are the words r, 2r, r + 1, 2r + 1, 2r - 1 and 2^256 - 1."""
    vals = [int(v) for v in values]
    assert all(0 <= v < R for v in vals), "lift() takes canonical values"
    if mode == "all":
        return [lift_one(v) for v in vals]
    out = [lift_one(v) if i % 7 == 0 else v for i, v in enumerate(vals)]
    if mode == "sparse":
        return out
    if mode == "edges":
        for i in range(min(len(EDGE_WORDS), len(vals))):
            out[i] = vals[i] + R if i % 2 == 0 else lift_one(vals[i])
        return out
    raise ValueError(mode)


def lifted_positions(n, mode):
    """the indices lift(.., mode) moves to a representative >= r in a vector of n elements"""
    if mode == "all":
        return list(range(n))
    pos = set(range(0, n, 7))
    if mode == "edges":
        pos |= set(range(min(len(EDGE_WORDS), n)))
    return sorted(pos)


def base(rng, n):
    """n canonical values: uniform residues, with 0, 0, 1, 1, r - 1, (2^256 - 1) mod r at positions 0 .. 5, values below 2^256 - 2r
    at positions 6 and 7 (7 is lifted by "sparse": to v + 2r), and r - 1 at the end (a non-zero top coefficient)."""
    v = [rng.randrange(R) for _ in range(n)]
    for i, p in enumerate(PLANTED[:n]):
        v[i] = p
    for i in (6, 7):
        if i < n:
            v[i] = rng.randrange(1, SMALL)
    if n > 8:
        v[n - 1] = R - 1
    return v


def pack(values):
    """ints below 2^256 -> 32-byte little-endian words, as they are (no reduction)"""
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def lift_bytes(blob, mode):
    """lift() on packed canonical words; only the moved positions are touched (large vectors)"""
    out = bytearray(blob)
    n = len(blob) // 32
    for i in lifted_positions(n, mode):
        v = int.from_bytes(out[32 * i:32 * i + 32], "little")
        assert v < R
        if mode == "edges" and i < len(EDGE_WORDS):
            w = v + R if i % 2 == 0 else lift_one(v)
        else:
            w = lift_one(v)
        out[32 * i:32 * i + 32] = w.to_bytes(32, "little")
    return bytes(out)
