#!/usr/bin/env python3
"""Many-point evaluation measurements (not part of bench.py): writes profiles/multi_eval_bench.json and prints it as one JSON line.
At n = 2^log_n coefficients resident on the device (kzg_fill_random_fr), values to host memory, median wall time of blocking calls
after a warm-up, one process; per batch in --batches and k in --ks:
  multi_eval_ms   kzg_poly_multi_eval as shipped (below its crossover it takes the kzg_poly_eval scans itself)
  kernels_ms      the same call kept on its own two kernels (option multi_eval_points_chunk = 4096): what the crossover is read from
  loop_ms         the loop of k x batch kzg_poly_eval calls on the same buffers: the route without the call.  Above --loop-cap calls
                  the loop runs over the first loop_cap calls and is scaled (loop_scaled: true); its cost is linear in the calls
  floor_ms        n k batch field products at the library multiply rate (FR_MUL_PEAK_G_S, tools/benchlib/common.py)
  loop_over_call  loop_ms / multi_eval_ms           floor_frac   floor_ms / multi_eval_ms
  stage_ms        per-kernel time of one call (kzg_prof_get): k_me_partials, k_me_combine
The values of the two routes are compared before anything is timed.  The library under test is KZG_AMD_LIBRARY when set (A/B
variants from tools/ab_build.py, e.g. -DKZG_ME_MONT: stage A on the Montgomery product).
   python tools/bench_multi_eval.py [--log-n 20] [--ks 1,16,64,256,4096,16384] [--batches 1,16] [--reps 5]"""
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
from tools.benchlib.common import FR_MUL_PEAK_G_S  # noqa: E402

CAN = L.FR_CANONICAL
KERNELS = ("k_me_partials", "k_me_combine", "k_horner_partials", "k_horner_scan")


def timed(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--ks", default="1,16,64,256,4096,16384")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-cap", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_eval_bench.json"))
    a = ap.parse_args()
    ks, batches = [int(x) for x in a.ks.split(",")], [int(x) for x in a.batches.split(",")]
    n, K, B = 1 << a.log_n, max(ks), max(batches)
    rng = random.Random(a.log_n)
    e = kzg_amd.Engine(0)
    coeffs = e.alloc_scalars(B * n).fill_random(a.log_n)
    xs = b"".join(rng.randrange(R_MODULUS).to_bytes(32, "little") for _ in range(K))
    ys, ys_loop = ctypes.create_string_buffer(32 * B * K), ctypes.create_string_buffer(32 * B * K)

    def ok(rc):
        if rc:
            _raise(e, rc)

    def call(k, batch):
        ok(e.lib.kzg_poly_multi_eval(e.ctx, coeffs.ptr, n, batch, xs, k, CAN, L.IN_DEVICE, ys))

    def loop(k, batch, calls):
        done = 0
        for b in range(batch):
            src = ctypes.c_void_p(coeffs.ptr.value + 32 * n * b)
            for i in range(k):
                if done == calls:
                    return
                ok(e.lib.kzg_poly_eval(e.ctx, src, n, xs[32 * i:32 * i + 32], CAN, L.IN_DEVICE, ctypes.byref(ys_loop, 32 * (b * k + i))))
                done += 1

    res = {"log_n": a.log_n, "library": os.path.relpath(os.environ["KZG_AMD_LIBRARY"], ROOT) if os.environ.get("KZG_AMD_LIBRARY") else "default", "fr_mul_peak_G_s": FR_MUL_PEAK_G_S, "per_batch": {}}
    for batch in batches:
        rows = {}
        for k in ks:
            calls = min(k * batch, a.loop_cap)
            loop(k, batch, calls)
            call(k, batch)
            assert ys.raw[:32 * calls] == ys_loop.raw[:32 * calls], "the two routes disagree on the values"
            work_s = n * k * batch / (FR_MUL_PEAK_G_S * 1e9)
            reps = a.reps if work_s < 0.2 else max(2, a.reps // 2)
            row = {"multi_eval_ms": timed(lambda: call(k, batch), reps)}
            e.set_option("multi_eval_points_chunk", 4096)
            row["kernels_ms"] = timed(lambda: call(k, batch), reps)
            e.prof_enable(True)
            e.prof_reset()
            call(k, batch)
            stage = {kn: round(e.prof_get(kn)[1], 4) for kn in KERNELS if e.prof_get(kn)[0]}
            e.prof_enable(False)
            e.set_option("multi_eval_points_chunk", 0)
            row["loop_ms"] = timed(lambda: loop(k, batch, calls), reps if calls <= 1024 else 1, warm=False) * (k * batch / calls)
            row = {key: round(v * 1e3, 4) for key, v in row.items()}
            row["loop_scaled"] = calls < k * batch
            row["floor_ms"] = round(work_s * 1e3, 4)
            row["loop_over_call"] = round(row["loop_ms"] / row["multi_eval_ms"], 2)
            row["floor_frac"] = round(row["floor_ms"] / row["multi_eval_ms"], 3)
            row["stage_ms"] = stage
            rows[str(k)] = row
            print("batch", batch, "k", k, json.dumps(row), file=sys.stderr, flush=True)
        res["per_batch"][str(batch)] = rows
    coeffs.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
