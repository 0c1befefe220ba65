#!/usr/bin/env python3
"""kzg_open_eval measurements (not part of bench.py): writes profiles/open_eval_bench.json and prints it as one JSON line.
At d = 2^log_d, evaluations and witnesses in device buffers, median wall time of blocking calls after a warm-up, one process:
  lone_ms             one kzg_open_eval call, one polynomial, z off the domain
  lone_fr_ms          its Fr part: kzg_quotient_eval_at (everything but the MSM)
  witness_eval_ms     kzg_witness_eval at an index               witness_eval_fr_ms   its Fr part: kzg_quotient_eval
  fr_ratio            lone_fr_ms / witness_eval_fr_ms (this path inverts d elements per call, that one has them in a table)
  coeff_route_ms      iNTT + kzg_poly_eval + kzg_witness_coeff on a monomial SRS of the same tau (the route without this call)
  batch_shared_ms     a batch of `batch` polynomials with ONE shared z      batch_distinct_ms   with `batch` distinct z
  msm_batch_ms        kzg_msm_g1_batch of the same batch against the same SRS
  *_per_s             polynomials per second of the three batch figures
  kernels_ms          per-kernel time of one lone call and one distinct-z batch (kzg_prof_get)
   python tools/bench_open_eval.py [--log-d 20] [--batch 64] [--reps 7]"""
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

KERNELS = ("k_open_powtab", "k_open_denoms", "k_batch_inverse", "k_open_eval_partials", "k_open_eval_finish", "k_open_quotient")
AFF = L.G1_AFFINE_MONT
DEV = L.IN_DEVICE | L.OUT_DEVICE
CAN = L.FR_CANONICAL


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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_eval_bench.json"))
    a = ap.parse_args()
    k, B = a.log_d, a.batch
    d = 1 << k
    rng = random.Random(k)
    tau = rng.randrange(R_MODULUS)
    le = lambda v: (v % R_MODULUS).to_bytes(32, "little")  # noqa: E731
    e = kzg_amd.Engine(0)
    lag = kzg_amd.setup_lagrange(e, tau, d)
    mono = kzg_amd.setup(e, tau, d, g2_len=0).gs
    evals = e.alloc_scalars(B * d).fill_random(k)
    work = e.alloc_scalars(d)
    q = e.alloc_scalars(d)
    out = e.alloc_scalars(B * 3)  # B x 96 bytes
    ys = ctypes.create_string_buffer(32 * B)
    z1 = le(rng.randrange(R_MODULUS))
    shared, distinct = z1 * B, b"".join(le(rng.randrange(R_MODULUS)) for _ in range(B))

    def ok(rc):
        if rc:
            _raise(e, rc)

    def open_eval(n, zs):
        ok(e.lib.kzg_open_eval(e.ctx, lag.handle, evals.ptr, d, n, zs, CAN, DEV, ys, out.ptr, AFF))

    def coeff_route():
        ok(e.lib.kzg_ntt_fr(e.ctx, work.ptr, k, 1, L.IN_DEVICE))
        ok(e.lib.kzg_poly_eval(e.ctx, work.ptr, d, z1, CAN, L.IN_DEVICE, ys))
        ok(e.lib.kzg_witness_coeff(e.ctx, mono.handle, work.ptr, d, z1, ys, CAN, DEV, out.ptr, AFF))
        ok(e.lib.kzg_ntt_fr(e.ctx, work.ptr, k, 0, L.IN_DEVICE))  # the evaluations again, for the next repetition

    work.upload(evals.download(d))
    res = {"log_d": k, "batch": B}
    res["lone_ms"] = timed(lambda: open_eval(1, z1), a.reps)
    res["lone_fr_ms"] = timed(lambda: ok(e.lib.kzg_quotient_eval_at(e.ctx, evals.ptr, d, z1, CAN, DEV, ys, q.ptr)), a.reps)
    res["witness_eval_ms"] = timed(lambda: ok(e.lib.kzg_witness_eval(e.ctx, lag.handle, evals.ptr, d, 12345 % d, CAN, DEV, out.ptr, AFF)), a.reps)
    res["witness_eval_fr_ms"] = timed(lambda: ok(e.lib.kzg_quotient_eval(e.ctx, evals.ptr, d, 12345 % d, CAN, DEV, q.ptr)), a.reps)
    # (the route's trailing forward transform restores the buffer and is not part of it: measured and taken off)
    fwd = timed(lambda: ok(e.lib.kzg_ntt_fr(e.ctx, q.ptr, k, 0, L.IN_DEVICE)), a.reps)
    res["coeff_route_ms"] = timed(coeff_route, a.reps) - fwd
    breps = max(3, a.reps // 2)
    res["batch_shared_ms"] = timed(lambda: open_eval(B, shared), breps)
    res["batch_distinct_ms"] = timed(lambda: open_eval(B, distinct), breps)
    res["msm_batch_ms"] = timed(lambda: ok(e.lib.kzg_msm_g1_batch(e.ctx, lag.handle, 0, evals.ptr, d, B, CAN, DEV, out.ptr, AFF)), breps)
    for key in [x for x in res if x.endswith("_ms")]:
        res[key] = round(res[key] * 1e3, 3)
    res["fr_ratio"] = round(res["lone_fr_ms"] / res["witness_eval_fr_ms"], 2)
    for key in ("batch_shared", "batch_distinct", "msm_batch"):
        res[key + "_per_s"] = round(B / res[key + "_ms"] * 1e3, 1)
    res["kernels_ms"] = {}
    for name, fn in (("lone", lambda: open_eval(1, z1)), ("batch_distinct", lambda: open_eval(B, distinct))):
        e.prof_enable(True)
        e.prof_reset()
        fn()
        res["kernels_ms"][name] = {kn: round(e.prof_get(kn)[1], 3) for kn in KERNELS}
        e.prof_enable(False)
    for buf in (evals, work, q, out):
        buf.free()
    lag.free()
    mono.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
