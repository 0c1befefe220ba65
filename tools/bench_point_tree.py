#!/usr/bin/env python3
"""Point-tree measurements (not part of bench.py): writes profiles/point_tree_bench.json and prints it as one JSON line.
Polynomials of n = 2^log_n coefficients resident on the device (kzg_fill_random_fr), random points, results to device buffers, median
wall time of blocking calls after a warm-up, one process.  The plan is built outside the timed region.  Per k in --ks:
  setup_ms, plan_bytes   kzg_point_tree_setup (one timed call) and what the plan holds
and per batch in --batches:
  eval_ms          kzg_point_tree_eval
  multi_eval_ms    kzg_poly_multi_eval on the same buffers in the same run; above --scale-from points it is scaled from its time at
                   --scale-from points (linear in k: n k products) and multi_eval_scaled is true
  eval_ratio       eval_ms / multi_eval_ms
  interpolate_ms   kzg_point_tree_interpolate of `batch` value vectors
  old_interpolate_ms, interpolate_ratio   kzg_interpolate on the same values (k <= 16384, its limit)
  stage_ms         per-kernel time of one kzg_point_tree_eval call (kzg_prof_get), a run of its own
Before anything is timed the values at two points are checked against kzg_poly_eval.
   python tools/bench_point_tree.py [--log-n 20] [--ks 256,1024,4096,16384,65536,262144,1048576] [--batches 1,16] [--reps 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import _raise  # noqa: E402

CAN = L.FR_CANONICAL
DEV = L.IN_DEVICE | L.OUT_DEVICE
OLD_INTERPOLATE_MAX = 16384


def timed(fn, reps):
    """median seconds of a blocking call after one warm-up call; a call of more than a second is repeated twice only"""
    t0 = time.perf_counter()
    fn()
    if time.perf_counter() - t0 > 1.0:
        reps = min(reps, 2)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--ks", default="256,1024,4096,16384,65536,262144,1048576")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale-from", type=int, default=16384, help="above 4 x this many points kzg_poly_multi_eval is scaled from its time here")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_tree_bench.json"))
    a = ap.parse_args()
    ks, batches = [int(x) for x in a.ks.split(",")], [int(x) for x in a.batches.split(",")]
    n, B, kmax = 1 << a.log_n, max(batches), max(ks)
    e = kzg_amd.Engine(0)
    coeffs = e.alloc_scalars(B * n).fill_random(a.log_n)
    pts = e.alloc_scalars(kmax).fill_random(77)
    vals, out = e.alloc_scalars(B * kmax).fill_random(78), e.alloc_scalars(B * kmax)
    xs_all = pts.download()

    def ok(rc):
        if rc:
            _raise(e, rc)

    res = {"log_n": a.log_n, "library": os.path.relpath(os.environ["KZG_AMD_LIBRARY"], ROOT) if os.environ.get("KZG_AMD_LIBRARY") else "default",
           "per_k": {}}
    warm = ctypes.c_void_p()  # the first setup of a process loads the code objects
    ok(e.lib.kzg_point_tree_setup(e.ctx, xs_all[: 32 * 2048], 2048, CAN, ctypes.byref(warm)))
    e.lib.kzg_point_tree_free(e.ctx, warm)
    base_multi = {}  # batch -> kzg_poly_multi_eval ms at --scale-from points
    for k in ks:
        xs = xs_all[: 32 * k]
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        ok(e.lib.kzg_point_tree_setup(e.ctx, xs, k, CAN, ctypes.byref(h)))
        setup_ms = (time.perf_counter() - t0) * 1e3
        nbytes = ctypes.c_size_t()
        ok(e.lib.kzg_point_tree_shape(h, None, None, ctypes.byref(nbytes), None))
        ok(e.lib.kzg_point_tree_eval(e.ctx, h, coeffs.ptr, n, 1, CAN, DEV, out.ptr))
        got = out.download(k)
        for i in (0, k - 1):
            x = int.from_bytes(xs[32 * i:32 * i + 32], "little")
            assert int.from_bytes(got[32 * i:32 * i + 32], "little") == e.poly_eval(coeffs, x, n=n), "a value differs from kzg_poly_eval"
        rows = {}
        for batch in batches:
            row = {"eval_ms": timed(lambda: ok(e.lib.kzg_point_tree_eval(e.ctx, h, coeffs.ptr, n, batch, CAN, DEV, out.ptr)), a.reps) * 1e3}
            if k <= 4 * a.scale_from:
                row["multi_eval_ms"] = timed(lambda: ok(e.lib.kzg_poly_multi_eval(e.ctx, coeffs.ptr, n, batch, xs, k, CAN, DEV, out.ptr)), a.reps) * 1e3
                row["multi_eval_scaled"] = False
                if k == a.scale_from:
                    base_multi[batch] = row["multi_eval_ms"]
            elif batch in base_multi:
                row["multi_eval_ms"] = base_multi[batch] * k / a.scale_from
                row["multi_eval_scaled"] = True
            if "multi_eval_ms" in row:
                row["eval_ratio"] = row["eval_ms"] / row["multi_eval_ms"]
            row["interpolate_ms"] = timed(lambda: ok(e.lib.kzg_point_tree_interpolate(e.ctx, h, vals.ptr, batch, CAN, DEV, out.ptr)), a.reps) * 1e3
            if 1024 <= k <= OLD_INTERPOLATE_MAX:
                ys = vals.download(batch * k)
                host = ctypes.create_string_buffer(32 * batch * k)
                row["old_interpolate_ms"] = timed(lambda: ok(e.lib.kzg_interpolate(e.ctx, xs, ys, k, batch, CAN, 0, host)), a.reps) * 1e3
                row["host_interpolate_ms"] = timed(lambda: ok(e.lib.kzg_point_tree_interpolate(e.ctx, h, ys, batch, CAN, 0, host)), a.reps) * 1e3
                row["interpolate_ratio"] = row["host_interpolate_ms"] / row["old_interpolate_ms"]  # both with host values and results
            e.prof_enable(True)
            e.prof_reset()
            ok(e.lib.kzg_point_tree_eval(e.ctx, h, coeffs.ptr, n, batch, CAN, DEV, out.ptr))
            stage = {kn: round(ms, 4) for kn, (cnt, ms) in e.prof_all().items() if cnt}
            e.prof_enable(False)
            row = {key: (round(v, 4) if isinstance(v, float) else v) for key, v in row.items()}
            row["stage_ms"] = stage
            rows[str(batch)] = row
            print("k", k, "batch", batch, json.dumps(row), file=sys.stderr, flush=True)
        res["per_k"][str(k)] = {"setup_ms": round(setup_ms, 3), "plan_bytes": nbytes.value, "per_batch": rows}
        e.lib.kzg_point_tree_free(e.ctx, h)
    for d in (coeffs, pts, vals, out):
        d.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
