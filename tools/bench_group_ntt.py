#!/usr/bin/env python3
"""Group-DFT measurements (not part of bench.py): one JSON line with
  g2_ntt_ms[N]            median wall time of one blocking kzg_ntt_g2 call (inverse, one array of N points, host buffers, affine
                          Montgomery in and out, points checked for the subgroup) after a warm-up
  g2_ntt_trusted_ms[N]    the same with option trusted_points = 1 (curve check only): what the subgroup check of the input costs
  g2_route_ms[N]          {"psi": .., "plain": ..}: option g2_ntt_mul = 0 against 1, trusted points, same process
  g2_lagrange_ms[d]       {"rows": .., "dft": ..}: kzg_srs_lagrange_from_monomial_g2 through the d-term sums (default below 2048) and
                          through the inverse DFT (option g2_lagrange_dft_from = 2)
  g1_ntt_ms[N]            one blocking kzg_ntt_g1 call (inverse, host buffers)
  g1_lagrange_ms[N]       one kzg_srs_lagrange_from_monomial_g1 call at the same size: the same DFT stages and scaling as FK20's
                          transforms run them, plus the SRS rows (resident input, no point check, no host copies)
  batch_ms["64x1024"]     {"g1": .., "g2": ..}: one call over 64 arrays of 1,024 points
   python tools/bench_group_ntt.py [--reps 3] [--g2-sizes 10,12,14,16,18,20] [--g1-sizes 16,20]"""
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
from kzg_amd.api import _raise  # noqa: E402

TAU = 0x5EED_6D7


def timed(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--g2-sizes", default="10,12,14,16,18,20")
    ap.add_argument("--g1-sizes", default="16,20")
    a = ap.parse_args()
    g2_sizes = [int(s) for s in a.g2_sizes.split(",")]
    g1_sizes = [int(s) for s in a.g1_sizes.split(",")]
    res = {"g2_ntt_ms": {}, "g2_ntt_trusted_ms": {}, "g2_route_ms": {}, "g2_lagrange_ms": {}, "g1_ntt_ms": {}, "g1_lagrange_ms": {},
           "batch_ms": {}}
    e = kzg_amd.Engine(0)

    def reps_for(k):
        return a.reps if k < 18 else 1

    def call(fn, blob, out, k, batch):
        def run():
            rc = fn(e.ctx, blob, k, batch, 1, 0, 0, out, 0)
            if rc:
                _raise(e, rc)
        return run

    hs = kzg_amd.setup_g2(e, TAU, 1 << max(g2_sizes + [16]))
    h_blob = hs.download()
    hs.free()
    out = ctypes.create_string_buffer(len(h_blob))
    for k in g2_sizes:
        N = 1 << k
        run = call(e.lib.kzg_ntt_g2, h_blob[:192 * N], out, k, 1)
        res["g2_ntt_ms"][N] = timed(run, reps_for(k))
        e.set_option("trusted_points", 1)
        res["g2_ntt_trusted_ms"][N] = timed(run, reps_for(k))
        e.set_option("trusted_points", 0)
    e.set_option("trusted_points", 1)
    for k in (12, 16):
        N = 1 << k
        run = call(e.lib.kzg_ntt_g2, h_blob[:192 * N], out, k, 1)
        r = {}
        for name, route in (("psi", 0), ("plain", 1)):
            e.set_option("g2_ntt_mul", route)
            r[name] = timed(run, a.reps)
        e.set_option("g2_ntt_mul", 0)
        res["g2_route_ms"][N] = r
    res["batch_ms"]["64x1024"] = {"g2": timed(call(e.lib.kzg_ntt_g2, h_blob[:192 << 16], out, 10, 64), a.reps)}
    e.set_option("trusted_points", 0)
    for d in (256, 1024):
        p = kzg_amd.setup(e, TAU, 1, g2_len=d)
        r = {}
        for name, frm in (("rows", 2048), ("dft", 2)):
            e.set_option("g2_lagrange_dft_from", frm)
            # the d-term sums take seconds at 1,024 points: one run, after the DFT path has warmed the context up at 256
            r[name] = timed(lambda: kzg_amd.compute_lagrange_basis_g2(p).free(), 1 if name == "rows" else a.reps, warm=name == "dft" or d == 256)
        e.set_option("g2_lagrange_dft_from", 2048)
        res["g2_lagrange_ms"][d] = r
        p.gs.free()
        p.hs.free()
    del h_blob, out

    p = kzg_amd.setup(e, TAU, 1 << max(g1_sizes + [16]), g2_len=0)
    g_blob = p.gs.download()
    p.gs.free()
    out = ctypes.create_string_buffer(len(g_blob))
    for k in g1_sizes:
        N = 1 << k
        res["g1_ntt_ms"][N] = timed(call(e.lib.kzg_ntt_g1, g_blob[:96 * N], out, k, 1), reps_for(k))
        q = kzg_amd.setup(e, TAU, N, g2_len=0)
        res["g1_lagrange_ms"][N] = timed(lambda: kzg_amd.compute_lagrange_basis(q).free(), reps_for(k))
        q.gs.free()
    res["batch_ms"]["64x1024"]["g1"] = timed(call(e.lib.kzg_ntt_g1, g_blob[:96 << 16], out, 10, 64), a.reps)
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
