#!/usr/bin/env python3
"""Folded-opening measurements (not part of bench.py): writes profiles/open_fold_bench.json and prints it as one JSON line.
At d = 2^log_d, evaluations and witnesses in device buffers, median wall time of blocking calls after a warm-up, one process; per
t in --ts (polynomials opened at ONE shared point, one group):
  fold_open_ms        (a) kzg_open_fold_eval: t values and ONE witness
  singles_ms          (b) kzg_open_eval on the same t polynomials with the shared z: t values and t witnesses, the route without the fold
  fr_fold_ms          (d) kzg_fr_fold alone            copy_ms   a device-to-device hipMemcpy of the same t x d x 32 bytes: the streaming
                      roof of this box (the copy also WRITES t x d x 32 bytes, the fold d x 32)
  verify_fold_ms      (e) kzg_verify_fold of the t values and the folded witness      verify_singles_ms   kzg_verify_eval of the t openings
  a_over_b, a_over_c  fold_open_ms / singles_ms, fold_open_ms / lone_ms       fold_over_copy   fr_fold_ms / copy_ms
  kernels_ms          per-kernel time of one kzg_open_fold_eval call (kzg_prof_get)
and once:
  lone_ms             (c) one kzg_open_eval call, one polynomial
   python tools/bench_open_fold.py [--log-d 20] [--ts 4,16,64] [--reps 7]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import R_MODULUS, _raise  # noqa: E402

KERNELS = ("k_fr_fold", "k_open_powtab", "k_open_denoms", "k_batch_inverse", "k_open_eval_partials", "k_open_eval_finish", "k_open_quotient")
AFF = L.G1_AFFINE_MONT
DEV = L.IN_DEVICE | L.OUT_DEVICE
CAN = L.FR_CANONICAL
HIP_MEMCPY_D2D = 3


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, default=20)
    ap.add_argument("--ts", default="4,16,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_fold_bench.json"))
    a = ap.parse_args()
    k, ts = a.log_d, [int(x) for x in a.ts.split(",")]
    d, T = 1 << k, max(ts)
    rng = random.Random(k)
    tau = rng.randrange(R_MODULUS)
    le = lambda v: (v % R_MODULUS).to_bytes(32, "little")  # noqa: E731
    e = kzg_amd.Engine(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int
    lag = kzg_amd.setup_lagrange(e, tau, d)
    small = kzg_amd.setup(e, tau, 2, g2_len=2)  # gs[0], hs[0], hs[1]: all the verifiers read
    evals = e.alloc_scalars(T * d).fill_random(k)
    spare = e.alloc_scalars(T * d)
    folded = e.alloc_scalars(d)
    out = e.alloc_scalars(T * 3)  # T x 96 bytes
    ys = ctypes.create_string_buffer(32 * T)
    z1, gamma, r = le(rng.randrange(R_MODULUS)), le(rng.randrange(1, R_MODULUS)), le(rng.randrange(1, R_MODULUS))

    def ok(rc):
        if rc:
            _raise(e, rc)

    def fold_open(t):
        ok(e.lib.kzg_open_fold_eval(e.ctx, lag.handle, evals.ptr, d, t, 1, z1, gamma, CAN, DEV, ys, out.ptr, AFF))

    def singles(t):
        ok(e.lib.kzg_open_eval(e.ctx, lag.handle, evals.ptr, d, t, z1 * t, CAN, DEV, ys, out.ptr, AFF))

    def copy(t):
        if hip.hipMemcpy(spare.ptr, evals.ptr, t * d * 32, HIP_MEMCPY_D2D) or hip.hipDeviceSynchronize():
            raise RuntimeError("hipMemcpy")

    def points(n):
        return out.download(n * 3)

    res = {"log_d": k, "ts": ts, "per_t": {}}
    res["lone_ms"] = round(timed(lambda: singles(1), a.reps) * 1e3, 3)
    # the commitments of the T polynomials, for the verifiers
    ok(e.lib.kzg_msm_g1_batch(e.ctx, lag.handle, 0, evals.ptr, d, T, CAN, DEV, out.ptr, AFF))
    commitments = points(T)
    for t in ts:
        reps = a.reps if t <= 16 else max(3, a.reps // 2)
        row = {}
        row["fold_open_ms"] = timed(lambda: fold_open(t), reps)
        ys_fold, w_fold = ys.raw[:32 * t], points(1)
        row["singles_ms"] = timed(lambda: singles(t), reps)
        ys_single, w_single = ys.raw[:32 * t], points(t)
        assert ys_fold == ys_single, "the two routes disagree on the values"
        row["fr_fold_ms"] = timed(lambda: ok(e.lib.kzg_fr_fold(e.ctx, evals.ptr, d, t, 1, gamma, CAN, DEV, folded.ptr)), reps)
        row["copy_ms"] = timed(lambda: copy(t), reps)
        okv, oks = ctypes.c_int(-1), ctypes.create_string_buffer(t)
        row["verify_fold_ms"] = timed(lambda: ok(e.lib.kzg_verify_fold(e.ctx, small.gs.handle, small.hs.handle, z1, ys_fold, CAN, commitments[:96 * t], t,
                                                                        None, w_fold, AFF, t, 1, gamma, r, ctypes.byref(okv))), reps)
        row["verify_singles_ms"] = timed(lambda: ok(e.lib.kzg_verify_eval(e.ctx, small.gs.handle, small.hs.handle, z1 * t, ys_single, CAN,
                                                                           commitments[:96 * t], w_single, AFF, t, oks)), reps)
        assert okv.value == 1 and oks.raw == b"\x01" * t, "an honest opening was rejected"
        row = {key: round(v * 1e3, 3) for key, v in row.items()}
        row["a_over_b"] = round(row["fold_open_ms"] / row["singles_ms"], 3)
        row["a_over_c"] = round(row["fold_open_ms"] / res["lone_ms"], 3)
        row["fold_over_copy"] = round(row["fr_fold_ms"] / row["copy_ms"], 2)
        row["fold_read_GBps"] = round(t * d * 32 / row["fr_fold_ms"] / 1e6, 1)
        e.prof_enable(True)
        e.prof_reset()
        fold_open(t)
        row["kernels_ms"] = {kn: round(e.prof_get(kn)[1], 3) for kn in KERNELS}
        e.prof_enable(False)
        res["per_t"][str(t)] = row
    for buf in (evals, spare, folded, out):
        buf.free()
    lag.free()
    small.gs.free()
    small.hs.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
