#!/usr/bin/env python3
"""kzg_sumcheck_round / kzg_mle_* measurements (not part of bench.py): writes profiles/sumcheck.txt (one line per measurement, then the
whole result as one JSON line) and prints it.  One GPU, device buffers, Montgomery form, median wall time of blocking calls after a
warm-up, everything in one process.  Per n in --log-ns:
  round_product   one kzg_sumcheck_round of col0 col1 (2 columns, n_eval 3)
  round_eq_gate   one round of eq (q_L a + q_R b + q_O c + q_M a b + q_C) (9 columns, n_eval 5)
  bind            kzg_mle_bind over the nine columns, in place
  eq              kzg_mle_eq of log2 n coordinates
  eval, eval_q    kzg_mle_eval of one table, without and with the Zeromorph quotients
  prove           kzg_amd.sumcheck.prove of eq x gate: log2 n rounds, each round, a SHA-256 challenge on the host and a bind
each beside two yardsticks that exist without these calls:
  copy_ms         a device-to-device hipMemcpy of (read + written) / 2 bytes, which it reads and writes: the bytes the call must move
  program_ms      (rounds only) n_eval x kzg_fr_program_run of the same plan over n / 2 rows: the cheapest route a caller had, and it
                  does not even include the extrapolation of the columns to X and the sum
kernel_ms: the time of k_sumcheck_round alone in one call (kzg_prof_get).
   python tools/bench_sumcheck.py [--log-ns 20,24] [--reps 9] [--out profiles/sumcheck.txt]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd import frp  # noqa: E402
from kzg_amd.api import R_MODULUS, _raise  # noqa: E402

DEV = L.IN_DEVICE | L.OUT_DEVICE
HIP_MEMCPY_D2D = 3
COPY_MAX = 512 << 20


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def challenge(k, sums):
    h = hashlib.sha256(b"%d" % k)
    for s in sums:
        for v in s:
            h.update(v.to_bytes(32, "little"))
    return int.from_bytes(h.digest(), "little") % R_MODULUS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-ns", default="20,24")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck.txt"))
    a = ap.parse_args()
    e = kzg_amd.Engine(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int

    def ok(rc):
        if rc:
            _raise(e, rc)

    scratch = e.alloc_scalars(2 * COPY_MAX // 32)

    def copy_ms(moved):
        half = min(moved // 2, COPY_MAX)

        def fn():
            if hip.hipMemcpy(ctypes.c_void_p(scratch.ptr.value + COPY_MAX), scratch.ptr, half, HIP_MEMCPY_D2D) or hip.hipDeviceSynchronize():
                raise RuntimeError("hipMemcpy")
        return timed(fn, a.reps) * (moved / 2 / half) * 1e3

    c = [frp.col(k) for k in range(9)]
    programs = {"round_product": (frp.compile([c[0] * c[1]]), 3),
                "round_eq_gate": (frp.compile([c[8] * (c[3] * c[0] + c[4] * c[1] + c[5] * c[2] + c[6] * c[0] * c[1] + c[7])]), 5)}
    res = {"reps": a.reps, "n": {}}
    lines = []
    for kn in [int(x) for x in a.log_ns.split(",")]:
        n = 1 << kn
        cols = [e.alloc_scalars(n, L.FR_MONT).fill_random(300 + k) for k in range(9)]
        out = e.alloc_scalars(n, L.FR_MONT)
        rows = {}

        def row(name, ms, moved, **extra):
            r = {"ms": round(ms, 4), "copy_ms": round(copy_ms(moved), 4)}
            r["over_copy"] = round(r["ms"] / r["copy_ms"], 2)
            r.update(extra)
            rows[name] = r
            lines.append("n=2^%d %-14s %s" % (kn, name, " ".join("%s=%s" % kv for kv in r.items())))

        for name, (prog, n_eval) in programs.items():
            use = cols[:prog.n_cols]
            cp = (ctypes.c_void_p * len(use))(*[b.ptr.value for b in use])
            cl = (ctypes.c_size_t * len(use))(*[n // 2] * len(use))
            op = (ctypes.c_void_p * 1)(out.ptr.value)
            sums = ctypes.create_string_buffer(32 * n_eval)
            with e.fr_program(prog) as plan:
                assert max(plan.degrees()) + 1 == n_eval
                fn = lambda: ok(e.lib.kzg_sumcheck_round(e.ctx, plan.handle, cp, None, n, n_eval, L.FR_MONT, L.IN_DEVICE, sums))  # noqa: E731
                ms = timed(fn, a.reps) * 1e3

                def through_program():
                    for _ in range(n_eval):
                        ok(e.lib.kzg_fr_program_run(e.ctx, plan.handle, cp, cl, None, n // 2, L.FR_MONT, DEV, op))
                program_ms = timed(through_program, a.reps) * 1e3
                e.prof_enable(True)
                e.prof_reset()
                fn()
                kernel_ms = e.prof_get("k_sumcheck_round")[1]
                e.prof_enable(False)
                row(name, ms, 32 * n * len(use), program_ms=round(program_ms, 4), program_over_round=round(program_ms / ms, 2), kernel_ms=round(kernel_ms, 4),
                    products_per_s=round(prog.n_mul * n_eval * (n // 2) / ms * 1e3))
        cp = (ctypes.c_void_p * 9)(*[b.ptr.value for b in cols])
        rho = e._host_scalar(12345, L.FR_MONT)
        row("bind", timed(lambda: ok(e.lib.kzg_mle_bind(e.ctx, cp, 9, n, rho, L.FR_MONT, DEV, cp)), a.reps) * 1e3, 9 * 48 * n)
        pt = b"".join(e._host_scalar(1000 + j, L.FR_MONT) for j in range(kn))
        row("eq", timed(lambda: ok(e.lib.kzg_mle_eq(e.ctx, pt, kn, L.FR_MONT, L.OUT_DEVICE, out.ptr)), a.reps) * 1e3, 32 * n)
        ys = ctypes.create_string_buffer(32)
        row("eval", timed(lambda: ok(e.lib.kzg_mle_eval(e.ctx, cols[0].ptr, kn, 1, pt, L.FR_MONT, DEV, ys, None)), a.reps) * 1e3, 32 * n)
        row("eval_q", timed(lambda: ok(e.lib.kzg_mle_eval(e.ctx, cols[0].ptr, kn, 1, pt, L.FR_MONT, DEV, ys, out.ptr)), a.reps) * 1e3, 64 * n)
        with e.fr_program(programs["round_eq_gate"][0]) as plan:
            # (the columns are folded in place: every repetition proves over what the last one left, the same work)
            prove_ms = timed(lambda: kzg_amd.sumcheck.prove(e, plan, cols, [], challenge), max(1, a.reps // 3)) * 1e3
        row("prove", prove_ms, 2 * (9 * 32 * n + 9 * 48 * n), rounds=kn)          # the rounds halve: twice the first round's round + bind
        res["n"][str(kn)] = rows
        for buf in cols + [out]:
            buf.free()
    scratch.free()
    e.close()
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="", flush=True)


if __name__ == "__main__":
    main()
