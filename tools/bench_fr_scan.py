#!/usr/bin/env python3
"""Scan, grand-product and batch-inversion measurements (not part of bench.py): writes profiles/fr_scan_bench.json and prints it as one
JSON line.  One GPU, device buffers, median wall time of blocking calls after a warm-up, everything in one process.  Per n in --log-ns
and per scalar format:
  scan_product / scan_sum   kzg_fr_scan, inclusive, at batch 1 and 8
  grand_t<t>                kzg_fr_grand_product at t = 1, 3, 4 and batch 1 and 8
  batch_inverse             kzg_fr_batch_inverse, out != in
each with two yardsticks measured beside it:
  copy_ms     a device-to-device hipMemcpy that moves the bytes the call moves.  The call reads `read` and writes `written` bytes of
              HBM (scan: the input twice, the output once; grand product: 2 t columns twice, z once; inversion: the input twice, the
              running products out and back, the output once); the copy is of (read + written) / 2 bytes, which it reads and writes
              (a copy longer than half the input buffer, 512 n bytes, is timed at that length and scaled: it streams at a flat rate).
  vec_mul_ms  kzg_fr_vec_mul over the call's n x batch elements: one Montgomery product per element, streamed
and the ratios over_copy, over_vec_mul.  kernels_ms: the per-kernel times of one call (kzg_prof_get).
   python tools/bench_fr_scan.py [--log-ns 16,20,24] [--reps 7]"""
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

DEV = L.IN_DEVICE | L.OUT_DEVICE
FORMATS = {"canonical": L.FR_CANONICAL, "montgomery": L.FR_MONT}
HIP_MEMCPY_D2D = 3
TS, BATCHES = (1, 3, 4), (1, 8)
SCAN_KERNELS = ("k_frscan_partials", "k_frscan_carry", "k_frscan_apply")
GRAND_KERNELS = ("k_grand_partials", "k_grand_carry", "k_grand_apply")


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
    ap.add_argument("--log-ns", default="16,20,24")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_scan_bench.json"))
    a = ap.parse_args()
    logs = [int(x) for x in a.log_ns.split(",")]
    e = kzg_amd.Engine(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int

    def ok(rc):
        if rc:
            _raise(e, rc)

    res = {"reps": a.reps, "per_n": {}}
    for k in logs:
        n = 1 << k
        cols = max(BATCHES) * max(TS) * n
        # uniform residues below r: valid words of either format
        num, den = e.alloc_scalars(cols).fill_random(2 * k), e.alloc_scalars(cols).fill_random(2 * k + 1)
        outb = e.alloc_scalars(max(BATCHES) * n)
        tot = ctypes.create_string_buffer(32 * max(BATCHES))
        zd = (ctypes.c_int * max(BATCHES))()

        def copy(nbytes):
            # (num -> den's tail would disturb the inputs: the copy runs inside num, second half from first; at most cols x 16 bytes)
            assert nbytes <= cols * 16
            dst = ctypes.c_void_p(num.ptr.value + cols * 16)
            if hip.hipMemcpy(dst, num.ptr, nbytes, HIP_MEMCPY_D2D) or hip.hipDeviceSynchronize():
                raise RuntimeError("hipMemcpy")

        def measure(fn, elems, read, written, kernels, sfmt):
            row = {"ms": timed(fn, a.reps)}
            moved = read + written
            half = min(moved // 2, cols * 16)
            row["copy_ms"] = timed(lambda: copy(half), a.reps) * (moved / 2 / half)
            row["vec_mul_ms"] = timed(lambda: ok(e.lib.kzg_fr_vec_mul(e.ctx, outb.ptr, den.ptr, elems, sfmt, L.IN_DEVICE)), a.reps)
            row = {key: round(v * 1e3, 4) for key, v in row.items()}
            row["over_copy"] = round(row["ms"] / row["copy_ms"], 2)
            row["over_vec_mul"] = round(row["ms"] / row["vec_mul_ms"], 2)
            row["moved_GBps"] = round(moved / row["ms"] / 1e6, 1)
            e.prof_enable(True)
            e.prof_reset()
            fn()
            row["kernels_ms"] = {kn: round(e.prof_get(kn)[1], 4) for kn in kernels}
            e.prof_enable(False)
            return row

        per_fmt = {}
        for fname, sfmt in FORMATS.items():
            rows = {}
            for b in BATCHES:
                by = b * n * 32
                for name, op in (("scan_product", L.SCAN_PRODUCT), ("scan_sum", L.SCAN_SUM)):
                    rows["%s_b%d" % (name, b)] = measure(
                        lambda: ok(e.lib.kzg_fr_scan(e.ctx, num.ptr, n, b, op, 0, sfmt, DEV, outb.ptr, tot)), b * n, 2 * by, by, SCAN_KERNELS, sfmt)
                for t in TS:
                    rows["grand_t%d_b%d" % (t, b)] = measure(
                        lambda: ok(e.lib.kzg_fr_grand_product(e.ctx, num.ptr, den.ptr, n, t, b, sfmt, DEV, outb.ptr, tot, zd)), b * n, 4 * t * by, by,
                        GRAND_KERNELS, sfmt)
            by = n * 32
            rows["batch_inverse"] = measure(lambda: ok(e.lib.kzg_fr_batch_inverse(e.ctx, num.ptr, n, sfmt, DEV, outb.ptr, None)), n, 3 * by, 2 * by,
                                            ("k_batch_inverse",), sfmt)
            per_fmt[fname] = rows
        res["per_n"][str(k)] = per_fmt
        for buf in (num, den, outb):
            buf.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
