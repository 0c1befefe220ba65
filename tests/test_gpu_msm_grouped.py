"""The grouped shape of kzg_msm_g1_batch (four streams whatever the hardware-queue pool: one sort launch and one tail launch per
group of MSMs, grid.y = the MSM's slot; two groups in flight in the two halves of a group arena) against the per-lane shape
(option group_msms = 0) byte for byte, and against the oracle's [p(tau)]G.

Nearly everything runs at n = 2^17, the smallest size the grouped shape covers (17-bit windows, 4-byte sort records), with option
hw_queues = 4 forcing the narrow plan whatever the process has; the last two tests take a ragged size and the other plans.  Batch counts with G = 8: 1 (a lone MSM: never grouped), 7 (less
than a group), 8 (one group exactly), 9 (a partial last group), 17 and 24 (a third group, which re-uses the first arena half).
The number of k_bin_hist launches says which shape ran: one per group, or one per MSM."""
import ctypes

import pytest

import kzg_amd
from oracle import c_oracle as C
from oracle import kzg_model as M

pytestmark = pytest.mark.gpu

TAU = 0x6709_ED5A_11CE
N = 1 << 17
N_RAGGED = 140001        # odd, and 15 x 140001 entries are more than small_entries = 2^21: not a small MSM under any plan
SRS_N = N_RAGGED + 512   # room for a non-zero SRS offset
BATCH = 24
OFFSET = 300
G1 = C.g1_generator()


@pytest.fixture(scope="module")
def engine():
    """a context of this module's own: in the suite's order the file runs behind the tests that close the session's context"""
    e = kzg_amd.Engine(0)
    yield e
    e.close()


def _view(engine, buf, b, n=N):
    v = kzg_amd.DeviceBuffer.__new__(kzg_amd.DeviceBuffer)
    v.engine, v.n, v.sfmt, v.ptr = engine, n, buf.sfmt, ctypes.c_void_p(buf.ptr.value + 32 * n * b)
    return v


def _batch(engine, srs, scalars, batch, group, offset=0, n=N, hw_queues=4):
    """(results, k_bin_hist launches) of one kzg_msm_g1_batch with option group_msms = group, planned for hw_queues hardware queues
    (4: the narrow plan, 3 lanes + 1 accumulation stream; 24: 13 + 4; 0: whatever the process has)"""
    engine.set_option("hw_queues", hw_queues)
    engine.set_option("group_msms", group)
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        got = engine.msm_batch(srs, scalars, n, batch, offset=offset)
        return got, engine.prof_get("k_bin_hist")[0]
    finally:
        engine.prof_enable(False)
        engine.set_option("group_msms", 16)     # the default
        engine.set_option("hw_queues", 0)


@pytest.fixture(scope="module")
def world(engine):
    """SRS, 24 uniform scalar vectors in one device buffer, their results on the per-lane shape (computed once; every batch count
    below is a prefix of it) and the oracle's value for the last MSM of every batch count"""
    params = kzg_amd.setup(engine, TAU, SRS_N, g2_len=0)
    assert params.gs.window_info() == (17, 15)
    buf = engine.alloc_scalars(N * BATCH)
    views = [_view(engine, buf, b).fill_random(4100 + b) for b in range(BATCH)]
    ref, launches = _batch(engine, params.gs, buf, BATCH, 0)
    assert launches == BATCH
    oracle = {b: C.g1_mul(G1, C.poly_eval_bytes(views[b].download(), N, TAU)) for b in (0, 6, 7, 8, 16, 23)}
    for b, w in oracle.items():
        assert ref[b] == w, b
    yield {"srs": params.gs, "buf": buf, "views": views, "ref": ref, "oracle": oracle}
    buf.free()
    params.gs.free()


@pytest.mark.parametrize("batch", [1, 7, 8, 9, 17, 24])
def test_grouped_batch_counts(engine, world, batch):
    got, launches = _batch(engine, world["srs"], world["buf"], batch, 8)
    assert launches == (1 if batch == 1 else (batch + 7) // 8)      # one sort launch per group (a lone MSM keeps its lane)
    assert got == world["ref"][:batch]
    assert got[batch - 1] == world["oracle"][batch - 1]


@pytest.mark.parametrize("group", [1, 16])
def test_group_sizes_1_and_16(engine, world, group):
    got, launches = _batch(engine, world["srs"], world["buf"], 17, group)
    assert launches == (17 + group - 1) // group
    assert got == world["ref"][:17]
    assert got[16] == world["oracle"][16]


def test_calling_shapes_offset_and_host_scalars(engine, world):
    """A non-zero SRS offset (device-resident scalars), and scalar vectors that come from the host as one flat blob, as in
    test_msm_batch_pipeline_paths: each slot stages its vector into its own workspace on the sort stream."""
    srs, buf = world["srs"], world["buf"]
    want = C.g1_mul(G1, C.poly_eval_bytes(world["views"][8].download(), N, TAU) * pow(TAU, OFFSET, M.R) % M.R)
    ref, launches = _batch(engine, srs, buf, 9, 0, offset=OFFSET)
    assert launches == 9 and ref[8] == want
    got, launches = _batch(engine, srs, buf, 9, 8, offset=OFFSET)
    assert launches == 2 and got == ref
    blob = buf.download(N * 9)
    got, launches = _batch(engine, srs, blob, 9, 8)
    assert launches == 2 and got == world["ref"][:9]


def test_skewed_polynomials_inside_a_group(engine, world):
    """The 3rd and the 12th polynomial of 17 are all-equal and u64-valued: oversized sort bins in the middle of a group and of the
    next one.  (A bin is oversized beyond 4 x 32768 = 2^17 records at this size, and an all-equal polynomial puts 2^17 records
    into the bin of each non-zero window: the value has the same digit in three windows, 3 x 2^17 records in one bin.)  Same bytes
    as the per-lane shape and the oracle; the slots' words are picked up, so the NEXT batch keeps the per-lane path and sorts its
    oversized bins in slices (k_heavy_place is enqueued); setting heavy_bins clears the note."""
    srs = world["srs"]
    buf = engine.alloc_scalars(N * 17)
    try:
        buf.upload(world["buf"].download(N * 17))
        skew = M.fr_to_le(0x1234 | 0x1234 << 17 | 0x1234 << 34) * N
        for b in (2, 11):
            _view(engine, buf, b).upload(skew)
        want = C.g1_mul(G1, C.poly_eval_bytes(skew, N, TAU))
        engine.set_option("heavy_bins", 0)
        ref, _ = _batch(engine, srs, buf, 17, 0)
        assert ref[2] == want and ref[11] == want
        assert ref[:2] == world["ref"][:2] and ref[12:] == world["ref"][12:17]
        engine.set_option("heavy_bins", 0)                      # forget what the per-lane run saw
        got, launches = _batch(engine, srs, buf, 17, 8)
        assert launches == 3 and got == ref
        engine.set_option("hw_queues", 4)
        engine.prof_reset()
        engine.prof_enable(True)
        again = engine.msm_batch(srs, buf, N, 17)
        assert again == ref
        assert engine.prof_get("k_bin_hist")[0] == 17           # per lane
        assert engine.prof_get("k_heavy_place")[0] == 17        # ... and in slices: the pick-up fired
    finally:
        engine.prof_enable(False)
        engine.set_option("hw_queues", 0)
        engine.set_option("heavy_bins", 0)
        buf.free()


def test_reuse_two_batches_then_a_lone_commit(engine, world):
    """Two grouped calls in a row on one context (the arena halves, the slots' table and the events are re-used), then a lone
    commit: no state leaks from one call into the next."""
    srs, buf = world["srs"], world["buf"]
    a, la = _batch(engine, srs, buf, 24, 8)
    b, lb = _batch(engine, srs, _view(engine, buf, 7), 1, 8)
    tail = kzg_amd.DeviceBuffer.__new__(kzg_amd.DeviceBuffer)
    tail.engine, tail.n, tail.sfmt, tail.ptr = engine, N * 17, buf.sfmt, ctypes.c_void_p(buf.ptr.value + 32 * N * 7)
    c, lc = _batch(engine, srs, tail, 17, 8)
    assert (la, lb, lc) == (3, 1, 3)
    assert a == world["ref"] and b == world["ref"][7:8] and c == world["ref"][7:24]
    assert engine.msm(srs, world["views"][23], n=N) == world["oracle"][23]


def test_ragged_size_under_every_plan(engine, world):
    """n = 140001 (no multiple of any chunk or tile size; too many entries for the small-MSM rule), 5 MSMs in groups of 2 and of
    16: the plan for four queues (3 lanes + 1 accumulation stream: the second FIFO stream is a lane's), the plan for 24 (13 + 4: both
    FIFO streams are accumulation streams) and the plan for the queues the process really has -- the same bytes as the lanes, one
    of them against the oracle.  The context reports the group size."""
    srs = world["srs"]
    buf = engine.alloc_scalars(N_RAGGED * 5)
    try:
        views = [_view(engine, buf, b, N_RAGGED).fill_random(7300 + b) for b in range(5)]
        ref, launches = _batch(engine, srs, buf, 5, 0, n=N_RAGGED)
        assert launches == 5
        assert ref[4] == C.g1_mul(G1, C.poly_eval_bytes(views[4].download(), N_RAGGED, TAU))
        for hw_queues in (4, 24, 0):
            for group, want_launches in ((2, 3), (16, 1)):
                got, launches = _batch(engine, srs, buf, 5, group, n=N_RAGGED, hw_queues=hw_queues)
                assert launches == want_launches and got == ref, (hw_queues, group)
        engine.set_option("hw_queues", 24)
        engine.msm_batch(srs, buf, N_RAGGED, 5)
        assert "lanes=5 accum_streams=4" in engine.info() and "group_msms=16" in engine.info()
    finally:
        engine.set_option("hw_queues", 0)
        buf.free()


def test_small_msms_run_grouped_with_queues_to_spare_too(engine, world):
    """2^17 points are 15 x 2^17 <= small_entries sorted entries: as lanes, with three or more accumulation streams planned, such MSMs
    take the small accumulation grid on four streams (common.h opt_accum_blocks_small).  Grouped they measured faster, so they run
    grouped under the plan for 24 queues as well, whether that rule is on or off.  Same bytes."""
    srs, buf = world["srs"], world["buf"]
    got, launches = _batch(engine, srs, buf, 9, 16, hw_queues=24)
    assert launches == 1 and got == world["ref"][:9]
    lanes, launches = _batch(engine, srs, buf, 9, 0, hw_queues=24)
    assert launches == 9 and lanes == world["ref"][:9]
    engine.set_option("accum_blocks_small", 0)
    try:
        got, launches = _batch(engine, srs, buf, 9, 16, hw_queues=24)
        assert launches == 1 and got == world["ref"][:9]
    finally:
        engine.set_option("accum_blocks_small", 160)
