#!/usr/bin/env python3
"""Polynomial division measurements (not part of bench.py): writes profiles/poly_divide_bench.json and prints it as one JSON line.
Dividends of na = 2^log_na coefficients and the divisor resident on the device (kzg_fill_random_fr), quotients and remainders to
device buffers, median wall time of blocking calls after a warm-up, one process; per nb in --nbs and batch in --batches:
  divide_ms       kzg_poly_divide: quotient, remainder and `exact`
  per_dividend_ms divide_ms / batch
  quotient_ms     the same call with r_out = exact = NULL (no remainder stage)
  mul_ms          one kzg_poly_mul of the quotient stage's product size (two operands of na - nb + 1 coefficients), same run
  over_mul        divide_ms / (batch x mul_ms): the call as a multiple of one product per dividend
  linear_ms       nb = 2 only: `batch` kzg_quotient_linear calls on the same dividends (x = -b[0] / b[1], y = the remainder)
  stage_ms        per-kernel time of one call (kzg_prof_get)
Before anything is timed a(z) = q(z) b(z) + r(z) is checked at one point through kzg_poly_eval.
   python tools/bench_poly_divide.py [--log-na 20] [--nbs 2,257,1025,524289] [--batches 1,16] [--reps 5]"""
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
from kzg_amd.api import R_MODULUS, _raise, unpack_scalars  # noqa: E402

CAN = L.FR_CANONICAL
DEV = L.IN_DEVICE | L.OUT_DEVICE
KERNELS = ("k_pd_load", "k_pd_fold_b", "k_pd_inv_base", "k_pd_newton", "k_pd_mul", "k_pd_emit_rev", "k_pd_fold", "k_pd_rem",
           "k_ntt_single", "k_ntt_pass1", "k_ntt_pass2", "k_ntt_pass2_short")
Z = 0x123456789ABCDEF


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-na", type=int, default=20)
    ap.add_argument("--nbs", default="2,257,1025,524289")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_divide_bench.json"))
    a = ap.parse_args()
    nbs, batches = [int(x) for x in a.nbs.split(",")], [int(x) for x in a.batches.split(",")]
    na, B = 1 << a.log_na, max(batches)
    e = kzg_amd.Engine(0)
    dividends = e.alloc_scalars(B * na).fill_random(a.log_na)
    q, r, prod = e.alloc_scalars(B * na), e.alloc_scalars(B * na), e.alloc_scalars(2 * na)
    ex = (ctypes.c_int * B)()

    def ok(rc):
        if rc:
            _raise(e, rc)

    res = {"log_na": a.log_na, "library": os.path.relpath(os.environ["KZG_AMD_LIBRARY"], ROOT) if os.environ.get("KZG_AMD_LIBRARY") else "default",
           "per_nb": {}}
    for nb in nbs:
        m = na - nb + 1
        b = e.alloc_scalars(nb).fill_random(1000 + nb)
        assert any(b.download(1, nb - 1)), "the divisor's top coefficient is zero"

        def call(batch, remainder=True):
            ok(e.lib.kzg_poly_divide(e.ctx, dividends.ptr, na, batch, b.ptr, nb, CAN, DEV, q.ptr, r.ptr if remainder else None, ex if remainder else None))

        call(1)
        az, qz, bz = e.poly_eval(dividends, Z, n=na), e.poly_eval(q, Z, n=m), e.poly_eval(b, Z, n=nb)
        rz = e.poly_eval(r, Z, n=nb - 1) if nb > 1 else 0
        assert az == (qz * bz + rz) % R_MODULUS, "a(z) != q(z) b(z) + r(z)"
        mul_ms = timed(lambda: ok(e.lib.kzg_poly_mul(e.ctx, dividends.ptr, m, q.ptr, m, CAN, DEV, prod.ptr)), a.reps) * 1e3
        rows = {}
        for batch in batches:
            row = {"divide_ms": timed(lambda: call(batch), a.reps) * 1e3, "quotient_ms": timed(lambda: call(batch, False), a.reps) * 1e3}
            row["per_dividend_ms"] = row["divide_ms"] / batch
            row["mul_ms"] = mul_ms
            row["over_mul"] = row["divide_ms"] / (batch * mul_ms)
            if nb == 2:
                b0, b1 = unpack_scalars(b.download())
                x = (-b0) * pow(b1, -1, R_MODULUS) % R_MODULUS
                xb = x.to_bytes(32, "little")
                srcs = [ctypes.c_void_p(dividends.ptr.value + 32 * na * i) for i in range(batch)]
                ys = []
                for s in srcs:
                    y = ctypes.create_string_buffer(32)
                    ok(e.lib.kzg_poly_eval(e.ctx, s, na, xb, CAN, L.IN_DEVICE, y))
                    ys.append(y.raw)

                def linear():
                    for s, y in zip(srcs, ys):
                        ok(e.lib.kzg_quotient_linear(e.ctx, s, na, xb, y, CAN, DEV, prod.ptr))
                row["linear_ms"] = timed(linear, a.reps) * 1e3
                row["over_linear"] = row["divide_ms"] / row["linear_ms"]
            e.prof_enable(True)
            e.prof_reset()
            call(batch)
            stage = {kn: round(e.prof_get(kn)[1], 4) for kn in KERNELS if e.prof_get(kn)[0]}
            e.prof_enable(False)
            row = {key: round(v, 4) for key, v in row.items()}
            row["stage_ms"] = stage
            rows[str(batch)] = row
            print("nb", nb, "batch", batch, json.dumps(row), file=sys.stderr, flush=True)
        res["per_nb"][str(nb)] = rows
        b.free()
    for d in (dividends, q, r, prod):
        d.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
