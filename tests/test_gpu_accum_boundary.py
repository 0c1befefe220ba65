"""k_accum_affine's bucket boundaries and its sign-tracked accumulator, through the C ABI (kzg_srs_upload_g1, kzg_msm_g1,
kzg_msm_g1_batch), every result against the oracle's MSM.

Round 1 keeps its accumulator as (X, Yt, ZZ, ZZZ, sigma), writes a partial raw at every bucket boundary and restarts from the table
point as it is; the fold kernels (k_fold_dense, k_fold_overflow) normalise a partial and apply its sign when they load it.  The
shapes below are the smallest at which that can go wrong: thousands of boundaries per launch (narrow windows at 2^10 / 2^12), a
sign flip at every entry of one bucket, a boundary at every entry, doublings and inverses at the head of a chain, identity table
entries, thread segments that start on a bucket start or end short, a bucket heavy enough for the overflow fold, the batched tail,
the positional tables and the wide-window readers."""
import random

import pytest

import kzg_amd
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests.gpu_common import rand_scalars

pytestmark = pytest.mark.gpu
R = M.R
TAU = 0xACC0_B0DA_4_5EED
N_MAX = 1 << 13


@pytest.fixture(scope="module")
def engine():
    """a context of this module's own: in the suite's order the file runs behind the tests that close the session's context"""
    e = kzg_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blob():
    return C.setup_g1(TAU, N_MAX)


class _Options:
    """engine options for the SRSs and MSMs inside the block, back to their defaults afterwards"""

    def __init__(self, engine, **opts):
        self.engine, self.opts = engine, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.engine.set_option(k, 0)


def _check(engine, raw, n, cases, **opts):
    with _Options(engine, **opts):
        srs = kzg_amd.Srs.upload(engine, raw[:96 * n], n)
        try:
            if opts.get("window_bits"):
                assert srs.window_info()[0] == opts["window_bits"]
            for name, sc in cases.items():
                assert len(sc) <= n
                assert engine.msm(srs, sc) == C.msm_g1(raw[:96 * len(sc)], sc), (name, n, opts)
        finally:
            srs.free()


@pytest.mark.parametrize("n,wb", [(1 << 10, 4), (1 << 10, 8), (1 << 12, 4), (1 << 12, 8), (1 << 13, 0)])
def test_many_boundaries_per_launch(engine, blob, n, wb):
    """64 / 32 windows of 8 / 128 buckets (and the default width at 2^13): every thread's eight entries cross boundaries"""
    rng = random.Random(1000 * wb + n)
    _check(engine, blob, n, {"random": rand_scalars(rng, n), "u64": rand_scalars(rng, n, "u64")}, window_bits=wb)


@pytest.mark.parametrize("wb", [8, 17])
def test_sign_flip_at_every_entry(engine, blob, wb):
    """scalars 1 and r - 1 alternating.  17 bits: r - 1 is recoded as -1, so all entries share bucket 1 with alternating signs"""
    n = 1 << 10
    cases = {"1,r-1": [1, R - 1] * (n // 2), "r-1,1": [R - 1, 1] * (n // 2), "1,1,r-1": ([1, 1, R - 1] * n)[:n],
             "r-1 only": [R - 1] * n, "odd count": ([1, R - 1] * n)[:777]}
    _check(engine, blob, n, cases, window_bits=wb)


def test_boundary_at_every_entry(engine, blob):
    """distinct small scalars under 17-bit windows: one entry per scalar, every entry in a bucket of its own -- flush and restart at
    every iteration of every lane, and every partial a bare table point (one partial per bucket: the fold must hand it on normalised)"""
    n = 1 << 12
    rng = random.Random(12)
    shuffled = list(range(1, n + 1))
    rng.shuffle(shuffled)
    cases = {"i+1": list(range(1, n + 1)), "shuffled": shuffled, "negated": [R - i for i in range(1, n + 1)],
             "alternating sign": [(i if i & 1 else R - i) for i in range(1, n + 1)], "pairs": [i // 2 + 1 for i in range(n)]}
    _check(engine, blob, n, cases, window_bits=17)


def test_repeated_points_and_identity_entries(engine):
    """an SRS holding the same point several times, its inverse and identity entries; all in one bucket with equal signs (a chain that
    starts P, P: doubling), with opposite signs (P, -P: infinity mid-chain, then more entries), and spread over buckets"""
    G = C.g1_generator()
    P = C.g1_mul(G, 777)
    nP = C.point_to_blob(M.g1_neg(C.blob_to_point(P)))
    Q = C.g1_mul(G, 31337)
    inf = bytes(96)
    rng = random.Random(13)
    for pts in ([P, P, nP, inf, G, P, inf, nP], [P, P, P, P, Q, Q, inf, inf], [inf, P, P, Q, nP, nP, P, G]):
        pts = pts * 32
        n = len(pts)
        raw = b"".join(pts)
        cases = {
            "one bucket, equal signs": [5] * n,
            "one bucket, opposite signs": [5, R - 5] * (n // 2),
            "P, -P, then more": ([5, R - 5, 5, 5] * n)[:n],
            "negated": [R - 5] * n,
            "two buckets": [5, 5, 9, 9] * (n // 4),
            "bucket per entry pair": [i // 2 + 1 for i in range(n)],
            "random": rand_scalars(rng, n),
            "zeros between": [0, 5, 5, 0, R - 5, 5, 0, 0] * (n // 8),
        }
        _check(engine, raw, n, cases, window_bits=17)
        _check(engine, raw, n, {k: cases[k] for k in ("one bucket, equal signs", "P, -P, then more", "random")}, window_bits=8)


@pytest.mark.parametrize("n", [32, 35, 67, 8 * 129 + 1])
def test_segment_edges(engine, blob, n):
    """17-bit windows, small scalars: one entry per scalar, eight entries per thread.  Buckets of exactly eight entries put every
    thread's first entry on a bucket start; n = 8 k + r leaves the last thread r entries; a bucket of 11 moves the starts off the grid"""
    aligned = [i // 8 + 1 for i in range(n)]
    off_grid = ([1] * 8 + [2] * 11 + [3] * 5 + [i // 8 + 4 for i in range(n)])[:n]
    single_last = [1] * (n - 1) + [2]
    _check(engine, blob, n, {"aligned": aligned, "off grid": off_grid, "last thread starts a bucket": single_last}, window_bits=17)


def test_heavy_bucket_reaches_the_overflow_fold(engine, blob):
    """all-equal scalars at 2^12: one bucket per window with 512 partials -- k_fold_overflow's slices read the raw list too"""
    n = 1 << 12
    rng = random.Random(14)
    s = rng.randrange(R)
    _check(engine, blob, n, {"all equal": [s] * n, "all r-1": [R - 1] * n, "two values": [s, R - s] * (n // 2)})
    _check(engine, blob, n, {"all equal": [s] * n, "all 1": [1] * n, "1,r-1": [1, R - 1] * (n // 2)}, window_bits=17)


@pytest.mark.parametrize("wb", [0, 17])
def test_batch_of_three(engine, blob, wb):
    """kzg_msm_g1_batch runs the pipelined tail (k_fold_dense<1> / k_rc_sums_t) where a lone call runs the other pair"""
    n = 1 << 12
    rng = random.Random(15 + wb)
    polys = [rand_scalars(rng, n), [rng.randrange(R)] * n, list(range(1, n + 1))]
    with _Options(engine, window_bits=wb):
        srs = kzg_amd.Srs.upload(engine, blob[:96 * n], n)
        try:
            got = engine.msm_batch(srs, [x for p in polys for x in p], n, 3)
            assert got == [C.msm_g1(blob[:96 * n], p) for p in polys]
        finally:
            srs.free()


def test_positional_tables(engine, blob):
    """option naf_window = 18: the same accumulation kernel on width-18 NAF digits, at one point and at 2^10"""
    n = 1 << 10
    rng = random.Random(16)
    cases = {"one point": [rng.randrange(R)], "random": rand_scalars(rng, n), "1,r-1": [1, R - 1] * (n // 2), "all equal": [rng.randrange(R)] * n,
             "i+1": list(range(1, n + 1))}
    _check(engine, blob, n, cases, naf_window=18)


@pytest.mark.parametrize("single_pass", [0, 1])
def test_widest_windows(engine, blob, single_pass):
    """window_bits = 20 (2^19 buckets) at 2^10: through its own two-level sort, and (sort_single_pass) through the two-pass sort of
    msm_wide.hip, whose round 1 and tail read the same partial list"""
    n = 1 << 10
    rng = random.Random(17 + single_pass)
    cases = {"random": rand_scalars(rng, n), "1,r-1": [1, R - 1] * (n // 2), "i+1": list(range(1, n + 1)), "all equal": [rng.randrange(R)] * n}
    _check(engine, blob, n, cases, window_bits=20, sort_single_pass=single_pass)
