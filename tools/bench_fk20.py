#!/usr/bin/env python3
"""FK20 measurements (not part of bench.py): one JSON line with
  plan_s[N]          kzg_fk20_setup wall time
  call_ms[N]         median wall time of one blocking kzg_witness_all_coeff call after a warm-up (2^12: a batch of 64)
  proofs_per_s[N]    witnesses per second of that call
  eval_many_proofs_per_s  kzg_witness_eval_many on 256 indices of one 2^20 evaluation vector (the MSM route), same process
  g1dft_ms[N]        kernel time (HIP events) of one size-N inverse G1 DFT (kzg_test_g1_ntt, hooks build)
  lagrange_ms[N]     wall time of one kzg_srs_lagrange_from_monomial_g1 call (the same stages, a d-point scaling pass, the SRS rows)
   python tools/bench_fk20.py [--reps 5] [--sizes 12,16,20]"""
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

TAU = 0x5EED_F20


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="12,16,20")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    res = {"plan_s": {}, "call_ms": {}, "proofs_per_s": {}, "g1dft_ms": {}, "lagrange_ms": {}}
    e = kzg_amd.Engine(0)
    top = max(sizes)
    gs = kzg_amd.setup(e, TAU, 1 << top, g2_len=0).gs
    for k in sizes:
        N = 1 << k
        B = 64 if k <= 12 else 1
        t0 = time.perf_counter()
        plan = kzg_amd.FK20Plan(e, gs, k)
        res["plan_s"][N] = round(time.perf_counter() - t0, 4)
        din = e.alloc_scalars(N * B).fill_random(k)
        dout = ctypes.c_void_p()
        assert e.lib.kzg_dev_alloc(e.ctx, N * B * 96, ctypes.byref(dout)) == 0

        def call():
            rc = e.lib.kzg_witness_all_coeff(e.ctx, plan.handle, din.ptr, N, B, L.FR_CANONICAL, L.IN_DEVICE | L.OUT_DEVICE, dout,
                                             L.G1_AFFINE_MONT)
            if rc:
                _raise(e, rc)
        s = timed(call, a.reps if k < 20 else max(2, a.reps // 2))
        key = "%dx%d" % (N, B) if B > 1 else str(N)
        res["call_ms"][key] = round(s * 1e3, 3)
        res["proofs_per_s"][key] = round(N * B / s, 1)
        e.lib.kzg_dev_free(e.ctx, dout)
        din.free()
        plan.free()
    # the MSM route, 256 openings of one evaluation vector
    d = 1 << top
    lag = kzg_amd.setup_lagrange(e, TAU, d)
    ev = e.alloc_scalars(d).fill_random(99)
    idx = (ctypes.c_size_t * 256)(*[(i * 4099) % d for i in range(256)])
    out = ctypes.create_string_buffer(96 * 256)

    def many():
        rc = e.lib.kzg_witness_eval_many(e.ctx, lag.handle, ev.ptr, d, idx, 256, L.FR_CANONICAL, L.IN_DEVICE, out, L.G1_AFFINE_MONT)
        if rc:
            _raise(e, rc)
    s = timed(many, 2)
    res["eval_many_proofs_per_s"] = {str(d): round(256 / s, 1)}
    ev.free()
    lag.free()
    # the G1 DFT alone (kernel time by HIP events) and compute_lagrange_basis, which runs on it (wall time)
    from tests.gpu_common import HooksEngine
    for k in [s for s in (16, 20) if s <= top]:
        N = 1 << k
        sub = kzg_amd.setup(e, TAU, N, g2_len=0).gs
        lg = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = e.lib.kzg_srs_lagrange_from_monomial_g1(e.ctx, sub.handle, ctypes.byref(lg))
        if rc:
            _raise(e, rc)
        res["lagrange_ms"][N] = round((time.perf_counter() - t0) * 1e3, 2)
        e.lib.kzg_srs_free(e.ctx, lg)
        pts = sub.download()
        sub.free()
        h = HooksEngine(0)
        h.lib.kzg_test_g1_ntt.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        h.lib.kzg_prof_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        h.lib.kzg_prof_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
        h.lib.kzg_prof_enable(h.ctx, 1)
        o = ctypes.create_string_buffer(96 * N)
        assert h.lib.kzg_test_g1_ntt(h.ctx, pts, k, 1, o) == 0, h.last_error()
        tot = 0.0
        for name in ("k_g1ntt_dit", "k_g1ntt_trivial"):
            n_, ms = ctypes.c_uint64(), ctypes.c_double()
            h.lib.kzg_prof_get(h.ctx, name.encode(), ctypes.byref(n_), ctypes.byref(ms))
            tot += ms.value
        res["g1dft_ms"][N] = round(tot, 2)
        h.close()
    gs.free()
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
