#!/usr/bin/env python3
"""Multi-point FK20 measurements (not part of bench.py): one JSON line with
  plan_s[N/l]            kzg_fk20_cosets_setup wall time
  call_ms[N/l]           median wall time of one blocking kzg_witness_cosets_coeff call (witnesses and interpolants, device
                         buffers) after a warm-up; 2^12: a batch of 64
  proofs_per_s[N/l]      coset proofs per second of that call
  per_term_call_ms[N/l]  the same call with option fk20_cosets_combine = 1 (mul256 per term), same process
  straus_ms / per_term_ms[N/l]  kernel time (HIP events) of the combination, k_coset_straus / k_coset_perterm (+ k_coset_reduce)
                                per call
  msm_route_s[N/l]       kzg_witness_coeff_batched on a few of the same cosets, extrapolated to all K
   python tools/bench_fk20_cosets.py [--reps 5] [--shapes 12/4x64,16/4,20/6]"""
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
from kzg_amd.api import _raise, pack_scalars  # noqa: E402
from oracle import c_oracle as C  # noqa: E402

TAU = 0x5EED_C05E7


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def kernel_ms(e, names):
    return sum(e.prof_get(n)[1] for n in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="12/4x64,16/4,20/6")
    ap.add_argument("--msm-calls", type=int, default=4)
    a = ap.parse_args()
    shapes = []
    for s in a.shapes.split(","):
        nl, _, b = s.partition("x")
        k, j = (int(v) for v in nl.split("/"))
        shapes.append((k, j, int(b) if b else 1))
    res = {k: {} for k in ("plan_s", "call_ms", "proofs_per_s", "per_term_call_ms", "straus_ms", "per_term_ms", "msm_route_s")}
    e = kzg_amd.Engine(0)
    top = max(k for k, _, _ in shapes)
    gs = kzg_amd.setup(e, TAU, 1 << top, g2_len=0).gs
    for k, j, B in shapes:
        N, l = 1 << k, 1 << j
        K = N // l
        key = "2^%d/%d" % (k, l) + ("x%d" % B if B > 1 else "")
        t0 = time.perf_counter()
        plan = kzg_amd.FK20CosetPlan(e, gs, k, j)
        res["plan_s"][key] = round(time.perf_counter() - t0, 4)
        din = e.alloc_scalars(N * B).fill_random(k)
        dw, dr = ctypes.c_void_p(), ctypes.c_void_p()
        assert e.lib.kzg_dev_alloc(e.ctx, K * B * 96, ctypes.byref(dw)) == 0
        assert e.lib.kzg_dev_alloc(e.ctx, N * B * 32, ctypes.byref(dr)) == 0

        def call():
            rc = e.lib.kzg_witness_cosets_coeff(e.ctx, plan.handle, din.ptr, N, B, L.FR_CANONICAL, L.IN_DEVICE | L.OUT_DEVICE, dw,
                                                L.G1_AFFINE_MONT, dr)
            if rc:
                _raise(e, rc)
        reps = a.reps if k < 20 else max(2, a.reps // 2)
        s = timed(call, reps)
        res["call_ms"][key] = round(s * 1e3, 3)
        res["proofs_per_s"][key] = round(K * B / s, 1)
        for route, names, out in ((0, ("k_coset_straus", "k_coset_reduce"), "straus_ms"),
                                  (1, ("k_coset_perterm", "k_coset_reduce"), "per_term_ms")):
            e.set_option("fk20_cosets_combine", route)
            if route == 1:
                res["per_term_call_ms"][key] = round(timed(call, max(2, reps // 2)) * 1e3, 3)
            e.prof_enable(True)
            e.prof_reset()
            call()
            res[out][key] = round(kernel_ms(e, names), 3)
            e.prof_enable(False)
        e.set_option("fk20_cosets_combine", 0)
        e.lib.kzg_dev_free(e.ctx, dw)
        e.lib.kzg_dev_free(e.ctx, dr)
        # the MSM route on the first cosets of one polynomial (same SRS), extrapolated
        raw = ctypes.create_string_buffer(N * 32)
        assert e.lib.kzg_dev_download(e.ctx, raw, din.ptr, N * 32) == 0
        blob = raw.raw
        coeffs = [int.from_bytes(blob[i * 32:(i + 1) * 32], "little") for i in range(N)]
        ev = C.fft(coeffs)
        calls = min(a.msm_calls, K)
        w = ctypes.create_string_buffer(96)
        r = ctypes.create_string_buffer(32 * max(l, 2))
        rlen = ctypes.c_size_t()
        t0 = time.perf_counter()
        for i in range(calls):
            xs = plan.coset_points(i)
            ys = [ev[i + t * K] for t in range(l)]
            rc = e.lib.kzg_witness_coeff_batched(e.ctx, gs.handle, blob, N, pack_scalars(xs), pack_scalars(ys), l, L.FR_CANONICAL, 0,
                                                 w, L.G1_AFFINE_MONT, r, ctypes.byref(rlen))
            if rc:
                _raise(e, rc)
        res["msm_route_s"][key] = round((time.perf_counter() - t0) / calls * K * B, 2)
        din.free()
        plan.free()
    gs.free()
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
