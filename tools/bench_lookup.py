#!/usr/bin/env python3
"""Lookup measurements (not part of bench.py): writes profiles/lookup_bench.json and prints it as one JSON line.  One GPU, device
buffers, Montgomery form, median wall time of blocking calls after a warm-up, everything in one process.
  setup     kzg_lookup_setup per table size in --log-tables (a device table of uniform residues)
  count     kzg_lookup_count (multiplicities, indices and the missing report) per table size and n in --log-ns, for the query
            distributions
              uniform    rows drawn uniformly from the table
              equal      one row, n times
              hot256     rows drawn uniformly from 256 rows of the table (the 2^16 table only)
              missing1   uniform, with 1 % of the values in no row
  terms     kzg_logup_terms with table and multiplicities at t = 1 and 3 per n
each with two yardsticks measured beside it:
  copy_ms           a device-to-device hipMemcpy that moves the bytes the call must read and write.  count: per value its 32 bytes, one
                    8-byte slot and one 32-byte key, and its 4-byte index; per table row a 4-byte counter and a 32-byte multiplicity.
                    setup: the table in, keys and slots out.  terms: t + 2 columns in, one out.  The copy is of (read + written) / 2
                    bytes, which it reads and writes (a copy longer than 512 MiB is timed at that length and scaled: it streams at
                    a flat rate).
  batch_inverse_ms  kzg_fr_batch_inverse over n elements (setup: over the table rows)
and the ratios over_copy, over_batch_inverse.  kernels_ms: the per-kernel times of one call (kzg_prof_get).
   python tools/bench_lookup.py [--log-tables 8,16,20] [--log-ns 20,24] [--reps 7]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import _raise  # noqa: E402

DEV = L.IN_DEVICE | L.OUT_DEVICE
HIP_MEMCPY_D2D = 3
COPY_MAX = 512 << 20
COUNT_KERNELS = ("k_lookup_probe", "k_lookup_emit")
SETUP_KERNELS = ("k_lookup_reduce", "k_lookup_build")
TERMS_KERNELS = ("k_logup_den", "k_batch_inverse", "k_logup_combine")
U32P = ctypes.POINTER(ctypes.c_uint32)


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
    ap.add_argument("--log-tables", default="8,16,20")
    ap.add_argument("--log-ns", default="20,24")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
    a = ap.parse_args()
    log_ts, log_ns = [int(x) for x in a.log_tables.split(",")], [int(x) for x in a.log_ns.split(",")]
    n_max = 1 << max(log_ns)
    e = kzg_amd.Engine(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int

    def ok(rc):
        if rc:
            _raise(e, rc)

    scratch = e.alloc_scalars(2 * COPY_MAX // 32)
    inv_in, inv_out = e.alloc_scalars(n_max, L.FR_MONT).fill_random(99), e.alloc_scalars(n_max, L.FR_MONT)

    def copy(nbytes):
        if hip.hipMemcpy(ctypes.c_void_p(scratch.ptr.value + COPY_MAX), scratch.ptr, nbytes, HIP_MEMCPY_D2D) or hip.hipDeviceSynchronize():
            raise RuntimeError("hipMemcpy")

    inverse_ms = {}

    def measure(fn, elems, read, written, kernels):
        row = {"ms": timed(fn, a.reps)}
        moved = read + written
        half = min(moved // 2, COPY_MAX)
        row["copy_ms"] = timed(lambda: copy(half), a.reps) * (moved / 2 / half)
        if elems not in inverse_ms:
            inverse_ms[elems] = timed(lambda: ok(e.lib.kzg_fr_batch_inverse(e.ctx, inv_in.ptr, elems, L.FR_MONT, DEV, inv_out.ptr, None)), a.reps)
        row["batch_inverse_ms"] = inverse_ms[elems]
        row = {key: round(v * 1e3, 4) for key, v in row.items()}
        row["over_copy"] = round(row["ms"] / row["copy_ms"], 2)
        row["over_batch_inverse"] = round(row["ms"] / row["batch_inverse_ms"], 2)
        row["moved_GBps"] = round(moved / row["ms"] / 1e6, 1)
        e.prof_enable(True)
        e.prof_reset()
        fn()
        row["kernels_ms"] = {kn: round(e.prof_get(kn)[1], 4) for kn in kernels}
        e.prof_enable(False)
        return row

    rng = np.random.default_rng(2024)
    res = {"reps": a.reps, "setup": {}, "count": {}, "terms": {}}
    for kt in log_ts:
        n_t = 1 << kt
        d_table = e.alloc_scalars(n_t, L.FR_MONT).fill_random(1000 + kt)
        table = np.frombuffer(d_table.download(), dtype=np.uint64).reshape(n_t, 4)
        handles = []

        def setup():
            h = ctypes.c_void_p()
            ok(e.lib.kzg_lookup_setup(e.ctx, d_table.ptr, n_t, L.FR_MONT, L.IN_DEVICE, ctypes.byref(h)))
            handles.append(h)

        slots = 2 * n_t * 8
        res["setup"][str(kt)] = measure(setup, n_t, n_t * 32, n_t * 32 + slots, SETUP_KERNELS)
        plan = handles.pop()
        for h in handles:
            e.lib.kzg_lookup_free(e.ctx, h)
        d_mult = e.alloc_scalars(n_t, L.FR_MONT)
        for kn in log_ns:
            n = 1 << kn
            d_vals = e.alloc_scalars(n, L.FR_MONT)
            d_idx = e.alloc_scalars((n * 4 + 31) // 32)
            miss, first = ctypes.c_size_t(), ctypes.c_size_t()
            dists = ["uniform", "equal", "missing1"] + (["hot256"] if kt == 16 else [])
            rows = {}
            for dist in dists:
                if dist == "equal":
                    rows_idx = np.full(n, n_t // 3, dtype=np.int64)
                elif dist == "hot256":
                    rows_idx = rng.integers(0, n_t, 256)[rng.integers(0, 256, n)]
                else:
                    rows_idx = rng.integers(0, n_t, n)
                vals = table[rows_idx]
                want_missing = 0
                if dist == "missing1":
                    gone = rng.random(n) < 0.01
                    want_missing = int(gone.sum())
                    fresh = rng.integers(0, 1 << 63, (want_missing, 4), dtype=np.uint64)
                    fresh[:, 3] >>= np.uint64(3)            # below r: a valid Montgomery word, in no row (up to chance 2^-200)
                    vals[gone] = fresh
                d_vals.upload(vals.tobytes())
                del vals

                def count():
                    ok(e.lib.kzg_lookup_count(e.ctx, plan, d_vals.ptr, n, 1, L.FR_MONT, DEV, d_mult.ptr, ctypes.cast(d_idx.ptr, U32P),
                                              ctypes.byref(miss), ctypes.byref(first)))

                row = measure(count, n, n * (32 + 8 + 32) + n_t * 4, n * 4 + n_t * (4 + 32), COUNT_KERNELS)
                assert miss.value == want_missing, (dist, miss.value, want_missing)
                row["missing"] = want_missing
                rows[dist] = row
            res["count"]["t%d_n%d" % (kt, kn)] = rows
            d_vals.free()
            d_idx.free()
        e.lib.kzg_lookup_free(e.ctx, plan)
        d_table.free()
        d_mult.free()
    for kn in log_ns:
        n = 1 << kn
        d_cols, d_table, d_mult, d_out = (e.alloc_scalars(3 * n, L.FR_MONT).fill_random(7), e.alloc_scalars(n, L.FR_MONT).fill_random(8),
                                          e.alloc_scalars(n, L.FR_MONT).fill_random(9), e.alloc_scalars(n, L.FR_MONT))
        beta = e._host_scalar(0x1234567, L.FR_MONT)
        zd = (ctypes.c_int * 1)()
        rows = {}
        for t in (1, 3):
            rows["t%d" % t] = measure(lambda: ok(e.lib.kzg_logup_terms(e.ctx, d_cols.ptr, d_table.ptr, d_mult.ptr, beta, n, t, 1, L.FR_MONT, DEV, d_out.ptr, zd)),
                                      n, (t + 2) * n * 32, n * 32, TERMS_KERNELS)
        res["terms"][str(kn)] = rows
        for buf in (d_cols, d_table, d_mult, d_out):
            buf.free()
    for buf in (scratch, inv_in, inv_out):
        buf.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
