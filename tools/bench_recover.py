#!/usr/bin/env python3
"""kzg_recover_cosets measurements (not part of bench.py): writes profiles/recover_bench.json and prints it as one JSON line.
Per shape "2^k/l" (+ "xB" for a batch), half the cosets missing at random, cells and outputs in device buffers:
  call_ms          median wall time of one blocking kzg_recover_cosets call (coefficients out) after a warm-up
  call_evals_ms    the same with the N evaluations as a second output
  setup_ms         the once-per-call part (zero polynomial, its K values, the K inverses): HIP events around it on the call's
                   stream (prof entry "recover_setup"), taken from one call with per-kernel timing on
  tree_launches    kernel launches of that part's k_rec_* kernels in that call
  ntt3_ms          in the same process: median wall time of three blocking kzg_ntt_fr calls of size N on a device buffer -- the
                   floor of the algorithm per polynomial
  ratio_to_floor   call_ms / (batch * ntt3_ms)
   python tools/bench_recover.py [--reps 7] [--shapes 20/6,20/6x64,16/4,20/0]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import _raise  # noqa: E402

TREE_KERNELS = ("k_rec_roots", "k_rec_leaf", "k_rec_mul_small", "k_rec_pad", "k_rec_stage", "k_rec_tile", "k_rec_pointwise",
                "k_rec_combine", "k_rec_zs_load")


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="20/6,20/6x64,16/4,20/0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_bench.json"))
    a = ap.parse_args()
    shapes = []
    for s in a.shapes.split(","):
        nl, _, b = s.partition("x")
        k, j = (int(v) for v in nl.split("/"))
        shapes.append((k, j, int(b) if b else 1))
    res = {k: {} for k in ("call_ms", "call_evals_ms", "setup_ms", "tree_launches", "ntt3_ms", "ratio_to_floor")}
    e = kzg_amd.Engine(0)
    for k, j, B in shapes:
        rng = random.Random(100 * k + j)
        N, l = 1 << k, 1 << j
        K = N // l
        key = "2^%d/%d" % (k, l) + ("x%d" % B if B > 1 else "")
        known = K - K // 2
        n = known * l - 5
        ids = sorted(rng.sample(range(K), known))
        # one polynomial of n coefficients, its evaluations, the cells of `ids` (the same cells for every polynomial of a batch)
        rnd = e.alloc_scalars(n).fill_random(k + j)
        padded = np.zeros((N, 32), dtype=np.uint8)
        padded[:n] = np.frombuffer(rnd.download(), dtype=np.uint8).reshape(n, 32)
        rnd.free()
        buf = e.alloc_scalars(N).upload(padded.tobytes())
        e.ntt(buf, k)
        ev = np.frombuffer(buf.download(), dtype=np.uint8).reshape(l, K, 32)
        cells = np.ascontiguousarray(ev[:, ids, :].transpose(1, 0, 2))
        din = e.alloc_scalars(B * known * l).upload(np.tile(cells.reshape(-1), B).tobytes())
        dc, de = e.alloc_scalars(B * n), e.alloc_scalars(B * N)
        idv = (ctypes.c_size_t * known)(*ids)

        def call(evals=False):
            rc = e.lib.kzg_recover_cosets(e.ctx, k, j, n, idv, known, din.ptr, B, L.FR_CANONICAL, L.IN_DEVICE | L.OUT_DEVICE, dc.ptr,
                                          de.ptr if evals else None, None)
            if rc:
                _raise(e, rc)

        def ntt3():
            for _ in range(3):
                e.ntt(buf, k)
        reps = a.reps if B == 1 else max(3, a.reps // 2)
        res["call_ms"][key] = round(timed(call, reps) * 1e3, 3)
        res["call_evals_ms"][key] = round(timed(lambda: call(True), reps) * 1e3, 3)
        res["ntt3_ms"][key] = round(timed(ntt3, a.reps) * 1e3, 3)
        res["ratio_to_floor"][key] = round(res["call_ms"][key] / (B * res["ntt3_ms"][key]), 2)
        e.prof_enable(True)
        e.prof_reset()
        call()
        res["setup_ms"][key] = round(e.prof_get("recover_setup")[1], 3)
        res["tree_launches"][key] = sum(e.prof_get(name)[0] for name in TREE_KERNELS)
        e.prof_enable(False)
        for d in (buf, din, dc, de):
            d.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
