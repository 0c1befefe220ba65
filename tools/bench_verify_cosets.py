#!/usr/bin/env python3
"""kzg_verify_cosets measurements (not part of bench.py): writes profiles/verify_cosets_bench.json and prints it as one JSON line.
The K = 2^log_n / l honest cells of one polynomial (proofs from kzg_witness_cosets_coeff, cells in a device buffer), one call:
  cells_per_s        K / median wall time of one blocking kzg_verify_cosets call after a warm-up
  call_ms, setup_s   that median; kzg_cosets_verifier_setup wall time; table_mb: the plan's window table
  kernel_ms          k_vc_interp / k_vc_sum / k_vc_check of one call with per-kernel timing on (kzg_prof_get)
and two yardsticks of the same process, both older entry points:
  verify_eval_per_s  (a) kzg_verify_eval at the same count (the same proofs at random points: the verdicts are false, the work is
                     that of any opening)
  batched_loop_cell_ms  (b) the loop of kzg_verify_eval_batched over the 256 cells of a 2^12 / 16 polynomial, per cell
   python tools/bench_verify_cosets.py [--reps 5] [--shape 20/6]"""
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

TAU = 0x5EED_CE115


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def open_all(e, params, k, j, seed):
    """(commitment, cells blob in cell order, proofs blob, interpolants blob, coefficients blob) of one random polynomial of 2^k
    coefficients"""
    N, l = 1 << k, 1 << j
    K = N // l
    buf = e.alloc_scalars(N).fill_random(seed)
    coeffs = buf.download()
    commitment = e.msm(params.gs, buf, N)
    plan = kzg_amd.FK20CosetPlan(e, params.gs, k, j)
    w, r = ctypes.create_string_buffer(96 * K), ctypes.create_string_buffer(32 * N)
    rc = e.lib.kzg_witness_cosets_coeff(e.ctx, plan.handle, coeffs, N, 1, L.FR_CANONICAL, 0, w, L.G1_AFFINE_MONT, r)
    plan.free()
    if rc:
        _raise(e, rc)
    e.ntt(buf, k)
    ev = np.frombuffer(buf.download(), dtype=np.uint8).reshape(l, K, 32)  # value t of coset i at index i + t K
    buf.free()
    return commitment, np.ascontiguousarray(ev.transpose(1, 0, 2)).tobytes(), w.raw, r.raw, coeffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="20/6")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cosets_bench.json"))
    a = ap.parse_args()
    k, j = (int(v) for v in a.shape.split("/"))
    N, l = 1 << k, 1 << j
    K = N // l
    res = {"shape": "2^%d/%d" % (k, l), "cells": K}
    e = kzg_amd.Engine(0)
    params = kzg_amd.setup(e, TAU, N, g2_len=l + 1)
    commitment, cells, proofs, _r, _c = open_all(e, params, k, j, 7)
    t0 = time.perf_counter()
    ver = kzg_amd.CosetVerifier(e, params, k, j)
    res["setup_s"] = round(time.perf_counter() - t0, 3)
    res["table_mb"] = round(ver.table_bytes() / 1e6, 1)
    dcells = e.alloc_scalars(K * l).upload(cells)
    idx, ids = (ctypes.c_uint32 * K)(), (ctypes.c_size_t * K)(*range(K))
    ok = ctypes.create_string_buffer(K)

    def call():
        rc = e.lib.kzg_verify_cosets(e.ctx, ver.handle, commitment, 1, idx, ids, dcells.ptr, proofs, K, L.FR_CANONICAL, L.G1_AFFINE_MONT,
                                     L.IN_DEVICE, ok)
        if rc:
            _raise(e, rc)
    t = timed(call, a.reps)
    assert ok.raw == b"\x01" * K, "an honest cell did not verify"
    res["call_ms"], res["cells_per_s"] = round(t * 1e3, 3), round(K / t)
    e.prof_enable(True)
    e.prof_reset()
    call()
    res["kernel_ms"] = {name: round(e.prof_get(name)[1], 3) for name in ("k_vc_interp", "k_vc_sum", "k_vc_check")}
    e.prof_enable(False)
    dcells.free()
    ver.free()
    # (a) kzg_verify_eval at the same count
    xs = e.alloc_scalars(2 * K).fill_random(11)
    xy = xs.download()
    xs.free()
    ok2 = ctypes.create_string_buffer(K)

    def eval_call():
        rc = e.lib.kzg_verify_eval(e.ctx, params.gs.handle, params.hs.handle, xy[:32 * K], xy[32 * K:], L.FR_CANONICAL, commitment * K, proofs,
                                   L.G1_AFFINE_MONT, K, ok2)
        if rc:
            _raise(e, rc)
    t = timed(eval_call, a.reps)
    res["verify_eval_ms"], res["verify_eval_per_s"] = round(t * 1e3, 3), round(K / t)
    params.gs.free()
    params.hs.free()
    # (b) today's route: one kzg_verify_eval_batched call per cell, 256 cells of a 2^12 / 16 polynomial
    sp = kzg_amd.setup(e, TAU, 1 << 12, g2_len=17)
    c2, cells2, proofs2, r2, _c = open_all(e, sp, 12, 4, 8)
    plan = kzg_amd.FK20CosetPlan(e, sp.gs, 12, 4)
    pts = [kzg_amd.pack_scalars(plan.coset_points(i)) for i in range(256)]
    plan.free()
    okb = ctypes.c_int()

    def loop():
        for i in range(256):
            rc = e.lib.kzg_verify_eval_batched(e.ctx, sp.gs.handle, sp.hs.handle, pts[i], 16, r2[i * 512:(i + 1) * 512], 16, L.FR_CANONICAL, c2,
                                               proofs2[i * 96:(i + 1) * 96], L.G1_AFFINE_MONT, ctypes.byref(okb))
            if rc:
                _raise(e, rc)
            assert okb.value == 1
    res["batched_loop_cell_ms"] = round(timed(loop, max(2, a.reps // 2)) * 1e3 / 256, 3)
    sp.gs.free()
    sp.hs.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
