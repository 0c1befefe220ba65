"""The multi-GPU commit path behind the C ABI (kzg_mctx / kzg_msrs, kzg_amd/csrc/mgpu.hip) on however many GPUs the box has
(one on the test box: a group of one, with the RCCL all-gather forced on so that the exchange code runs).  Parity: the group's
commitment equals the single-GPU commitment, the oracle's Pippenger and [p(tau)]G; the 8-way sharding of configs[4] is
exercised shard by shard in tests/test_gpu_fullsize.py."""
import ctypes
import random

import pytest

import kzg_amd
from kzg_amd import _lib as L
from kzg_amd.distributed import shard_range
from oracle import c_oracle as C
from oracle import kzg_model as M
from tests.gpu_common import rand_scalars

pytestmark = pytest.mark.gpu

TAU = 0x0BADC0FFEE123457


NO_RCCL_NEEDED = ("test_group_rejects_bad_arguments", "test_rccl_load_failure_is_an_error_not_a_crash",
                  "test_group_commit_matches_single_gpu_and_oracle[0]")


@pytest.fixture(autouse=True)
def _rccl_or_skip(request):
    """Everything here but NO_RCCL_NEEDED forms an RCCL communicator in this process: skipped (with the probe's diagnostics) on a
    box where the session's probe child could not form one in time -- conftest.py, need_rccl."""
    if request.node.name not in NO_RCCL_NEEDED:
        request.getfixturevalue("need_rccl")


@pytest.fixture(scope="module")
def group():
    lib = L.load()
    ndev = lib.kzg_device_count()
    assert ndev >= 1
    g = kzg_amd.DeviceGroup(list(range(min(ndev, 8))))
    yield g
    g.close()


@pytest.mark.parametrize("always_gather", [0, 1])
def test_group_commit_matches_single_gpu_and_oracle(engine, group, always_gather):
    group.set_option("always_gather", always_gather)   # 1: ncclAllGather runs even in a group of one
    rng = random.Random(11)
    n = 1000
    srs = group.setup(TAU, n)
    assert len(srs) == n
    blob = C.setup_g1(TAU, n)
    # every resident shard holds exactly its contiguous range of setup(tau, n).gs
    for i in range(group.local_count):
        shard, first = srs.shard(i)
        lo, hi = shard_range(n, group.rank(i), group.world)
        assert first == lo and len(shard) == hi - lo
        assert shard.download() == blob[96 * lo: 96 * hi]
    for m in (n, 777, 1, 0):        # polynomials shorter than the SRS only reach the first shards
        coeffs = rand_scalars(rng, m)
        got = group.commit(srs, coeffs)
        assert got == C.msm_g1(blob[: 96 * m], coeffs), m
        assert got == C.g1_mul(C.g1_generator(), C.poly_eval(coeffs, TAU) if m else 0), m
    with pytest.raises(kzg_amd.ReferencePanic):          # polynomial longer than the SRS: the slice index panic
        group.commit(srs, rand_scalars(rng, n + 1))
    srs.free()
    group.set_option("always_gather", 0)


def test_group_commit_batch_host_and_device_resident(engine, group):
    group.set_option("always_gather", 1)
    rng = random.Random(12)
    n, batch = 4096 + 37, 5
    srs = group.setup(TAU, n)
    polys = [rand_scalars(rng, n) for _ in range(batch - 2)] + [[0] * n, [M.R - 1] * n]
    want = [C.g1_mul(C.g1_generator(), C.poly_eval(p, TAU)) for p in polys]
    flat = kzg_amd.pack_scalars([c for p in polys for c in p])
    assert group.commit_batch(srs, flat, n, batch) == want
    # compressed output format through the group path
    got48 = group.commit_batch(srs, flat, n, batch, ofmt=L.G1_ZCASH_COMPRESSED)
    assert [M.g1_to_compressed(C.blob_to_point(w)) for w in want] == got48
    # device-resident slices: per local GPU a [batch][shard] array
    bufs = []
    for i in range(group.local_count):
        lo, hi = shard_range(n, group.rank(i), group.world)
        e = group.engine(i)
        b = e.alloc_scalars((hi - lo) * batch)
        b.upload(kzg_amd.pack_scalars([c for p in polys for c in p[lo:hi]]))
        bufs.append(b)
    assert group.commit_batch(srs, bufs, n, batch) == want
    for b in bufs:
        b.free()
    srs.free()
    group.set_option("always_gather", 0)


def test_group_upload_and_witness(engine, group):
    group.set_option("always_gather", 1)
    rng = random.Random(13)
    n = 600
    blob = C.setup_g1(TAU, n)
    srs = group.upload(blob, n)
    coeffs = rand_scalars(rng, n)
    assert group.commit(srs, coeffs) == C.msm_g1(blob, coeffs)
    x = rng.randrange(M.R)
    y = C.poly_eval(coeffs, x)
    w = group.create_witness(srs, coeffs, (x, y))
    ptau = C.poly_eval(coeffs, TAU)
    assert w == C.g1_mul(C.g1_generator(), (ptau - y) * M.fr_inv(TAU - x) % M.R)
    with pytest.raises(kzg_amd.PointNotOnPolynomial):
        group.create_witness(srs, coeffs, (x, (y + 1) % M.R))
    # degree-0 polynomial: empty quotient -> identity (src/coeff_form.rs:332-341 edge)
    assert group.create_witness(srs, [5], (3, 5)) == bytes(96)
    srs.free()
    group.set_option("always_gather", 0)


def test_group_per_process_mode_world1(engine):
    """kzg_mctx_unique_id + kzg_mctx_create_rank (the one-process-per-GPU entry): a world of one rank."""
    uid = kzg_amd.DeviceGroup.unique_id()
    assert len(uid) == 128 and any(uid)
    g = kzg_amd.DeviceGroup.for_rank(0, 0, 1, uid)
    assert g.world == 1 and g.local_count == 1 and g.rank(0) == 0
    g.set_option("always_gather", 1)     # ncclCommInitRank + ncclAllGather in a world of one
    rng = random.Random(14)
    n = 300
    srs = g.setup(TAU, n)
    coeffs = rand_scalars(rng, n)
    assert g.commit(srs, coeffs) == C.g1_mul(C.g1_generator(), C.poly_eval(coeffs, TAU))
    srs.free()
    g.close()


def test_group_rejects_bad_arguments():
    lib = L.load()
    h = ctypes.c_void_p()
    arr = (ctypes.c_int * 2)(0, 0)
    assert lib.kzg_mctx_create(arr, 2, ctypes.byref(h)) == L.KZG_ERR_SHAPE      # duplicate device
    assert lib.kzg_mctx_create(arr, 0, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    assert lib.kzg_mctx_create_rank(0, 3, 2, None, ctypes.byref(h)) == L.KZG_ERR_SHAPE
    arr = (ctypes.c_int * 1)(99)
    assert lib.kzg_mctx_create(arr, 1, ctypes.byref(h)) == L.KZG_ERR_NO_DEVICE
    # a later device fails after an earlier context exists: the half-built group is torn down cleanly
    arr = (ctypes.c_int * 2)(0, 99)
    assert lib.kzg_mctx_create(arr, 2, ctypes.byref(h)) == L.KZG_ERR_NO_DEVICE


def test_group_info_names_the_adopted_rccl(group):
    info = group.info()
    assert "rccl=" in info and "librccl" in info and "hip=" in info and "version=" in info
    assert f"world={group.world}" in info


def test_group_device_resident_witness_and_batched(engine, group):
    """kzg_witness_coeff_sharded with the polynomial resident on every local GPU, and create_witness_batched over the group
    (replicated interpolant + quotient, sharded MSM): equal to the single-GPU calls and to the known-tau identities."""
    group.set_option("always_gather", 1)
    rng = random.Random(15)
    n = 5000
    srs = group.setup(TAU, n)
    coeffs = rand_scalars(rng, n)
    ptau = C.poly_eval(coeffs, TAU)
    G = C.g1_generator()
    x = rng.randrange(M.R)
    y = C.poly_eval(coeffs, x)
    want_w = C.g1_mul(G, (ptau - y) * M.fr_inv(TAU - x) % M.R)
    bufs = []
    for i in range(group.local_count):
        b = group.engine(i).alloc_scalars(n)
        b.upload(kzg_amd.pack_scalars(coeffs))
        bufs.append(b)
    assert group.create_witness(srs, bufs, (x, y)) == want_w
    assert group.create_witness(srs, coeffs, (x, y)) == want_w
    with pytest.raises(kzg_amd.PointNotOnPolynomial):
        group.create_witness(srs, bufs, (x, (y + 1) % M.R))
    for k in (1, 2, 7, 64):
        xs = [rng.randrange(M.R) for _ in range(k)]
        ys = [C.poly_eval(coeffs, v) for v in xs]
        single = kzg_amd.KZGProver(kzg_amd.setup(engine, TAU, n, g2_len=0))
        w1 = single.create_witness_batched(kzg_amd.Polynomial(coeffs), xs, ys)
        for arg in (coeffs, bufs):
            w, r = group.create_witness_batched(srs, arg, list(zip(xs, ys)))
            assert w == w1.elem() and r == w1.polynomial().coeffs, k
        if k >= 2:
            Z = 1
            for v in xs:
                Z = Z * (TAU - v) % M.R
            assert w == C.g1_mul(G, (ptau - C.poly_eval(r, TAU)) * M.fr_inv(Z) % M.R), k
        single.parameters.gs.free()
    ys_bad = list(ys)
    ys_bad[3] = (ys_bad[3] + 1) % M.R
    with pytest.raises(kzg_amd.PointNotOnPolynomial):
        group.create_witness_batched(srs, bufs, list(zip(xs, ys_bad)))
    with pytest.raises(kzg_amd.ReferencePanic):           # duplicate opening points: invert().unwrap()
        group.create_witness_batched(srs, coeffs, [(xs[0], ys[0]), (xs[0], ys[0]), (xs[1], ys[1])])
    for b in bufs:
        b.free()
    srs.free()
    group.set_option("always_gather", 0)


def _hooks_group(hooks, per_process):
    """a device group inside the -DKZG_TEST_HOOKS build of the library"""
    lib = hooks.lib
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.kzg_mctx_create.argtypes = [ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]
    lib.kzg_mctx_create_rank.argtypes = [i32, i32, i32, vp, ctypes.POINTER(vp)]
    lib.kzg_mctx_unique_id.argtypes = [vp]
    lib.kzg_mctx_destroy.argtypes = [vp]
    lib.kzg_mctx_destroy.restype = None
    lib.kzg_mctx_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    lib.kzg_mctx_last_error.argtypes = [vp]
    lib.kzg_mctx_last_error.restype = ctypes.c_char_p
    lib.kzg_srs_setup_g1_sharded.argtypes = [vp, vp, i32, sz, ctypes.POINTER(vp)]
    lib.kzg_msrs_free.argtypes = [vp, vp]
    lib.kzg_msrs_free.restype = None
    lib.kzg_commit_coeff_sharded.argtypes = [vp, vp, vp, sz, i32, i32, vp, i32]
    h = vp()
    if per_process:
        uid = ctypes.create_string_buffer(128)
        assert lib.kzg_mctx_unique_id(uid) == 0
        assert lib.kzg_mctx_create_rank(0, 0, 1, uid, ctypes.byref(h)) == 0
    else:
        arr = (i32 * 1)(0)
        assert lib.kzg_mctx_create(arr, 1, ctypes.byref(h)) == 0
    return h


@pytest.mark.parametrize("per_process", [False, True])
def test_local_failure_is_agreed_on_not_hung(hooks_engine, per_process):
    """A rank whose local phase fails still enters the exchange (per-process mode) and every rank returns its error; the group
    stays usable.  World of one with the all-gather forced on: the failure travels through ncclAllGather in the status slot."""
    lib = hooks_engine.lib
    h = _hooks_group(hooks_engine, per_process)
    assert lib.kzg_mctx_set_option(h, b"always_gather", 1) == 0
    n = 500
    srs = ctypes.c_void_p()
    assert lib.kzg_srs_setup_g1_sharded(h, (TAU % M.R).to_bytes(32, "little"), L.FR_CANONICAL, n, ctypes.byref(srs)) == 0
    rng = random.Random(16)
    coeffs = rand_scalars(rng, n)
    blob = kzg_amd.pack_scalars(coeffs)
    out = ctypes.create_string_buffer(96)
    want = C.g1_mul(C.g1_generator(), C.poly_eval(coeffs, TAU))
    assert lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT) == 0 and out.raw == want
    assert lib.kzg_test_mctx_inject_failure(h, L.KZG_ERR_ALLOC) == 0
    rc = lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)
    assert rc == L.KZG_ERR_ALLOC
    assert b"injected local failure" in lib.kzg_mctx_last_error(h)
    # the next call is unaffected
    assert lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT) == 0 and out.raw == want
    lib.kzg_msrs_free(h, srs)
    lib.kzg_mctx_destroy(h)


@pytest.mark.parametrize("per_process", [False, True])
def test_resource_failure_before_the_exchange_is_agreed_on(hooks_engine, per_process):
    """a rank-local allocation failure BEFORE the collective (growing the exchange buffers for a batch larger
    than any before) must not leave the peers inside the data all-gather.  The ranks agree on it through the status-only
    all-gather over buffers that exist since the group was formed; the call fails with the allocation error on every rank, the
    smaller buffers stay in place and the group stays usable (the same batch succeeds on the next call)."""
    lib = hooks_engine.lib
    h = _hooks_group(hooks_engine, per_process)
    sz, i32, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    lib.kzg_commit_coeff_sharded_batch.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, i32]
    assert lib.kzg_mctx_set_option(h, b"always_gather", 1) == 0
    n, batch = 300, 70    # 70 > the 64 partials the buffers hold from the start
    srs = ctypes.c_void_p()
    assert lib.kzg_srs_setup_g1_sharded(h, (TAU % M.R).to_bytes(32, "little"), L.FR_CANONICAL, n, ctypes.byref(srs)) == 0
    rng = random.Random(21)
    polys = [rand_scalars(rng, n) for _ in range(batch)]
    blob = b"".join(kzg_amd.pack_scalars(p) for p in polys)
    out = ctypes.create_string_buffer(96 * batch)
    assert lib.kzg_test_mctx_inject_alloc_failure(h) == 0
    rc = lib.kzg_commit_coeff_sharded_batch(h, srs, blob, n, batch, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)
    assert rc == L.KZG_ERR_ALLOC and b"exchange buffers" in lib.kzg_mctx_last_error(h)
    G = C.g1_generator()
    want = b"".join(C.g1_mul(G, C.poly_eval(p, TAU)) for p in polys)
    assert lib.kzg_commit_coeff_sharded_batch(h, srs, blob, n, batch, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT) == 0
    assert out.raw == want
    lib.kzg_msrs_free(h, srs)
    lib.kzg_mctx_destroy(h)


def test_exchange_deadline_kills_the_group_instead_of_hanging(hooks_engine):
    """A peer that never arrives: the wait behind the all-gather polls with a deadline (option gather_timeout_ms).  Simulated in a
    group of one by parking the exchange behind a 400 ms spin kernel with a 50 ms deadline: the call returns KZG_ERR_INTERNAL,
    the communicator is aborted, and the group is dead -- every later call fails at once -- until the host destroys it."""
    import time
    lib = hooks_engine.lib
    h = _hooks_group(hooks_engine, True)
    assert lib.kzg_mctx_set_option(h, b"always_gather", 1) == 0
    n = 200
    srs = ctypes.c_void_p()
    assert lib.kzg_srs_setup_g1_sharded(h, (TAU % M.R).to_bytes(32, "little"), L.FR_CANONICAL, n, ctypes.byref(srs)) == 0
    rng = random.Random(22)
    coeffs = rand_scalars(rng, n)
    blob = kzg_amd.pack_scalars(coeffs)
    out = ctypes.create_string_buffer(96)
    want = C.g1_mul(C.g1_generator(), C.poly_eval(coeffs, TAU))
    # a stall shorter than the deadline is just a slow exchange
    assert lib.kzg_mctx_set_option(h, b"gather_timeout_ms", 2000) == 0
    assert lib.kzg_test_mctx_inject_stall(h, 100) == 0
    assert lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT) == 0 and out.raw == want
    assert lib.kzg_mctx_set_option(h, b"gather_timeout_ms", 50) == 0
    assert lib.kzg_test_mctx_inject_stall(h, 400) == 0
    t0 = time.time()
    rc = lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)
    assert rc == L.KZG_ERR_INTERNAL and b"did not complete within 50 ms" in lib.kzg_mctx_last_error(h)
    assert time.time() - t0 < 6.0
    rc = lib.kzg_commit_coeff_sharded(h, srs, blob, n, L.FR_CANONICAL, 0, out, L.G1_AFFINE_MONT)
    assert rc == L.KZG_ERR_INTERNAL and b"group is dead" in lib.kzg_mctx_last_error(h)
    lib.kzg_msrs_free(h, srs)
    lib.kzg_mctx_destroy(h)


def test_exchange_deadline_ignores_another_contexts_work_on_the_shared_lanes(engine, need_rccl):
    """every context of a device draws its lanes from one shared stream pool, so a plain Engine busy on pool lane 0 used to
    sit in front of the group's all-gather and a short gather_timeout_ms read a healthy exchange as a dead peer.  The exchange now has
    a stream of its own, completion is an event behind the collective, and the group's local phase is waited for without a deadline:
    with an engine of the same device (same library, same pool) saturating the lanes from another thread, twenty commits under a
    100 ms deadline all succeed and the group stays alive."""
    import threading
    group = kzg_amd.DeviceGroup([0])
    group.set_option("always_gather", 1)
    n = 300
    srs = group.setup(TAU, n)
    rng = random.Random(24)
    coeffs = rand_scalars(rng, n)
    want = C.g1_mul(C.g1_generator(), C.poly_eval(coeffs, TAU))
    assert group.commit(srs, coeffs) == want       # the communicator is formed
    # the neighbour: batches of 32 commitments of 2^16 terms over all of the pool's lanes (about 10 ms each), back to back
    m, batch = 1 << 16, 32
    params = kzg_amd.setup(engine, TAU, m, g2_len=0)
    sc = engine.alloc_scalars(m * batch).fill_random(77)
    bout = ctypes.create_string_buffer(96 * batch)
    stop, steps, bad = threading.Event(), [0], []

    def neighbour():
        while not stop.is_set():
            rc = engine.lib.kzg_msm_g1_batch(engine.ctx, params.gs.handle, 0, sc.ptr, m, batch, sc.sfmt, L.IN_DEVICE, bout, L.G1_AFFINE_MONT)
            if rc:
                bad.append(rc)
                return
            steps[0] += 1
    th = threading.Thread(target=neighbour)
    th.start()
    try:
        while steps[0] < 2 and not bad:
            pass
        group.set_option("gather_timeout_ms", 100)
        for _ in range(20):
            assert group.commit(srs, coeffs) == want
        assert "dead=0" in group.info()
    finally:
        stop.set()
        th.join()
    assert steps[0] >= 2 and not bad
    sc.free()
    params.gs.free()
    srs.free()
    group.close()


def test_witness_eval_sharded(engine):
    """KZGProverEvalForm::create_witness over the device group (src/eval_form.rs:124-140): Lagrange-basis SRS sharded, quotient
    replicated, MSM sharded; equal to the oracle's [(p(tau) - y) / (tau - w^m)]G, to the single-GPU kzg_witness_eval, host- and
    device-resident evaluations; the reference's panics map to KZG_ERR_SHAPE."""
    d, log_d = 1 << 11, 11
    rng = random.Random(23)
    coeffs = rand_scalars(rng, d)
    evals = C.fft(coeffs)
    _, _, omega = kzg_amd.compute_omega(d)
    lag_single = kzg_amd.setup_lagrange(engine, TAU, d)
    group = kzg_amd.DeviceGroup([0])
    group.set_option("always_gather", 1)
    lag = group.upload(lag_single.download(), d)
    G = C.g1_generator()
    ptau = C.poly_eval(coeffs, TAU)
    for m in (0, 1, 777, d - 1):
        xm = pow(omega, m, M.R)
        want = C.g1_mul(G, (ptau - evals[m]) * pow(TAU - xm, -1, M.R) % M.R)
        assert group.create_witness_eval(lag, evals, m) == want
    dev = group.engine(0).alloc_scalars(d)
    dev.upload(kzg_amd.pack_scalars(evals))
    xm = pow(omega, 5, M.R)
    assert group.create_witness_eval(lag, [dev], 5) == C.g1_mul(G, (ptau - evals[5]) * pow(TAU - xm, -1, M.R) % M.R)
    with pytest.raises(Exception):
        group.create_witness_eval(lag, evals, d)            # index out of range
    with pytest.raises(Exception):
        group.create_witness_eval(lag, evals[:d - 1], 0)    # not a power of two
    dev.free()
    lag.free()
    group.close()
    lag_single.free()


def test_rccl_load_failure_is_an_error_not_a_crash():
    """dlerror() read twice -> std::string(nullptr).  With RCCL unloadable (forced in a child process, hooks build)
    kzg_mctx_unique_id and a forced all-gather return the 'cannot load RCCL' error."""
    import os
    import subprocess
    import sys
    code = r"""
import ctypes, os, sys
sys.path.insert(0, %r)
import kzg_amd
kzg_amd.load()
lib = ctypes.CDLL(os.path.join(os.path.dirname(kzg_amd.__file__), "libkzg_mi355x_hooks.so"))
buf = ctypes.create_string_buffer(128)
rc = lib.kzg_mctx_unique_id(buf)
assert rc == -4, rc
h = ctypes.c_void_p()
arr = (ctypes.c_int * 1)(0)
assert lib.kzg_mctx_create(arr, 1, ctypes.byref(h)) == 0
lib.kzg_mctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
assert lib.kzg_mctx_set_option(h, b"always_gather", 1) == 0
srs = ctypes.c_void_p()
lib.kzg_srs_setup_g1_sharded.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
assert lib.kzg_srs_setup_g1_sharded(h, (5).to_bytes(32, "little"), 1, 8, ctypes.byref(srs)) == 0
out = ctypes.create_string_buffer(96)
lib.kzg_commit_coeff_sharded.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
rc = lib.kzg_commit_coeff_sharded(h, srs, (1).to_bytes(32, "little") * 8, 8, 1, 0, out, 0)
lib.kzg_mctx_last_error.restype = ctypes.c_char_p
lib.kzg_mctx_last_error.argtypes = [ctypes.c_void_p]
msg = lib.kzg_mctx_last_error(h)
assert rc == -4 and b"cannot load RCCL" in msg, (rc, msg)
print("ok")
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KZG_TEST_NO_RCCL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=140)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.limit(300)
def test_prover_context_and_device_group_share_one_stream_pool():
    """VERDICT r4 weak #13 (the silent hardware-queue cliff): a plain prover context and a device group alive in ONE process -- what
    INTEGRATION.md section 5b describes.  All contexts of a device take their streams from one pool per process (runtime.hip, StreamPool),
    13 lanes + 4 accumulation streams (+ the group's exchange stream), which leaves the RCCL communicator its queues: neither plan is narrowed (kzg_ctx_info /
    kzg_mctx_info say so, and no warning is printed) and both paths give the same commitments, alone, one after the other and
    committing at once from two threads.  (Same-box rates: the group beside a live context 471 against 473 commitments/s alone; it
    was 385 with one set of streams per context, 337 with 16 + 4 beside the communicator.)  tools/engine_and_group_ab.py: each
    scenario in a fresh child process."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the children get the queue pool kzg_init_hw_queues(0) asks for (24), whatever GPU_MAX_HW_QUEUES the runner exported (the library
    # keeps an exported value, and a small one narrows every plan below)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "engine_and_group_ab.py"), "20", "32"], capture_output=True, text=True, timeout=280,
                       env=env)
    res = {d["scenario"]: d for d in (json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{"))}
    assert set(res) == {"engine", "group", "engine_then_group", "both"}, r.stdout[-2000:] + r.stderr[-2000:]
    for sc, d in res.items():
        assert "rc" not in d, d
        for key in ("engine_info", "group_info"):
            if key in d:
                assert "narrowed_from=none" in d[key] and "lanes=13 accum_streams=4" in d[key], (sc, d[key])
        assert not d["stderr_kzg_lines"], d["stderr_kzg_lines"]          # no "pipeline is narrowed" warning
    assert res["engine_then_group"]["same_results"] and res["both"]["same_results"]
    assert all(v > 0 for d in res.values() for k, v in d.items() if k.endswith("per_s"))
    # The RATES are in profiles/r05_engine_and_group.txt (group beside a live context 471 against 473 commitments/s alone, both at
    # once 512-517), measured by the same tool run on its own: here its children run beside the pytest process, which has used the
    # GPU, and a process' mere presence slows every other process on the chip by a factor that differs from child to child (141 /
    # 439 / 177 commitments/s in one run of this test) -- what can be asserted inside the suite is the plan, not the clock.


def test_cpp_host_mirror_device_group(tmp_path):
    """include/kzg_mi355x.hpp, DeviceGroup / ShardedKZGProver: the C++ mirror test with its device-group block (RCCL all-gather forced
    on in a group of one): the sharded commitment and witness equal the single-GPU ones, PointNotOnPolynomial comes through."""
    import subprocess
    from tests.gpu_common import build_cpp_mirror
    out = subprocess.run([build_cpp_mirror(tmp_path), "group"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "with the device group" in out.stdout, (out.returncode, out.stdout, out.stderr)
