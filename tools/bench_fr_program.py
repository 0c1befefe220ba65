#!/usr/bin/env python3
"""kzg_fr_program_run measurements (not part of bench.py): writes profiles/fr_program_bench.json and prints it as one JSON line.  One
GPU, device buffers, Montgomery form, median wall time of blocking calls after a warm-up, everything in one process.
  gate      the standard gate q_L a + q_R b + q_O c + q_M a b + q_C: 8 columns in, 1 out, 5 products
  gate_perm the gate plus alpha times a three-wire permutation term with a rotation, times the periodic 1 / Z_H
  temps16   sixteen temporaries alive at once (the program of tests/test_gpu_fr_program.py), also at every "fr_program_block"
per n in --log-ns, each with yardsticks measured beside it:
  copy_ms       a device-to-device hipMemcpy of (read + written) / 2 bytes, which it reads and writes: the bytes the program must
                move (32 B per row and full-length column it names, 32 B per row and output)
  vec_mul_ms    kzg_fr_vec_mul over n elements; products_per_s of the program = its multiplications x n / its time, beside
                vec_mul_products_per_s = n / vec_mul_ms
  calls_ms      (gate only) the same gate through the calls a caller had before: four device-to-device copies and five kzg_fr_vec_mul
                for the products, one copy of q_C and one kzg_fr_lincomb for the sum
                (the device is drained behind every copy: the copies run on the null stream, the calls on lane streams)
kernel_ms: the time of k_fr_program alone in one call (kzg_prof_get).
   python tools/bench_fr_program.py [--log-ns 20,24] [--reps 9]"""
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
from kzg_amd import frp  # noqa: E402
from kzg_amd.api import _raise  # noqa: E402

DEV = L.IN_DEVICE | L.OUT_DEVICE
HIP_MEMCPY_D2D = 3
COPY_MAX = 512 << 20
E = 4     # the extension factor of the permutation term's rotation and of the 1 / Z_H column


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def gate_expr():
    a, b, c, ql, qr, qo, qm, qc = (frp.col(k) for k in range(8))
    return ql * a + qr * b + qo * c + qm * a * b + qc


def gate_perm_program():
    w, sig, ident, z, zh_inv = [frp.col(k) for k in range(3)], [frp.col(8 + k) for k in range(3)], frp.col(11), frp.col(12), frp.col(13)
    alpha, beta, gamma, ks = frp.const(0), frp.const(1), frp.const(2), [frp.const(3 + k) for k in range(3)]
    lhs, rhs = frp.col(12, E), z
    for j in range(3):
        lhs = lhs * (w[j] + beta * sig[j] + gamma)
        rhs = rhs * (w[j] + beta * ks[j] * ident + gamma)
    return frp.compile([(gate_expr() + alpha * (lhs - rhs)) * zh_inv])


def temps16_program():
    I, A, M, C, K, T, O = frp.insn, L.FRP_ADD, L.FRP_MUL, L.FRP_COL, L.FRP_CONST, L.FRP_TEMP, L.FRP_OUT
    words = []
    for k in range(16):
        words += I(A, T, k, C, k, K, k)
    for k in range(8):
        words += I(M, T, k, T, k, T, 15 - k)
    for k in range(8, 16):
        words += I(M, T, k, T, k, K, k - 8)
    for k in range(1, 16):
        words += I(A, T, 0, T, 0, T, k)
    words += I(A, O, 0, T, 0, T, 0)
    return frp.Compiled(words, 16, 16, 1, 16, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-ns", default="20,24")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_program_bench.json"))
    a = ap.parse_args()
    log_ns = [int(x) for x in a.log_ns.split(",")]
    e = kzg_amd.Engine(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipDeviceSynchronize.restype = ctypes.c_int

    def ok(rc):
        if rc:
            _raise(e, rc)

    def d2d(dst, src, nbytes):
        # the copy runs on the null stream, the library's calls on lane streams: the device is drained behind every copy, so the
        # call that follows sees it (the few microseconds of each wait are part of calls_ms)
        if hip.hipMemcpy(dst, src, nbytes, HIP_MEMCPY_D2D) or hip.hipDeviceSynchronize():
            raise RuntimeError("hipMemcpy")

    scratch = e.alloc_scalars(2 * COPY_MAX // 32)

    def copy(nbytes):
        d2d(ctypes.c_void_p(scratch.ptr.value + COPY_MAX), scratch.ptr, nbytes)

    programs = {"gate": frp.compile([gate_expr()]), "gate_perm": gate_perm_program(), "temps16": temps16_program()}
    res = {"reps": a.reps, "programs": {k: {"insns": p.n_insns, "cols": p.n_cols, "consts": p.n_consts, "temps": p.n_temps, "mul": p.n_mul}
                                        for k, p in programs.items()}, "n": {}}
    for kn in log_ns:
        n = 1 << kn
        cols = [e.alloc_scalars(n, L.FR_MONT).fill_random(100 + k) for k in range(16)]
        zh = e.alloc_scalars(E, L.FR_MONT).fill_random(200)
        out = e.alloc_scalars(n, L.FR_MONT).fill_random(201)
        work = e.alloc_scalars(5 * n, L.FR_MONT)
        vec_mul_ms = timed(lambda: ok(e.lib.kzg_fr_vec_mul(e.ctx, out.ptr, cols[0].ptr, n, L.FR_MONT, L.IN_DEVICE)), a.reps) * 1e3
        rows = {"vec_mul_ms": round(vec_mul_ms, 4), "vec_mul_products_per_s": round(n / vec_mul_ms * 1e3)}
        for name, prog in programs.items():
            use = cols[:13] + [zh] if name == "gate_perm" else cols[:prog.n_cols]
            consts = [1000 + k for k in range(prog.n_consts)]
            blocks = (0, 64, 128, 256) if name == "temps16" else (0,)
            cp = (ctypes.c_void_p * len(use))(*[c.ptr.value for c in use])
            cl = (ctypes.c_size_t * len(use))(*[c.n for c in use])
            kb = b"".join(e._host_scalar(k, L.FR_MONT) for k in consts) or None
            op = (ctypes.c_void_p * 1)(out.ptr.value)
            with e.fr_program(prog) as plan:
                for block in blocks:
                    e.set_option("fr_program_block", block)
                    fn = lambda: ok(e.lib.kzg_fr_program_run(e.ctx, plan.handle, cp, cl, kb, n, L.FR_MONT, DEV, op))  # noqa: E731
                    row = {"ms": round(timed(fn, a.reps) * 1e3, 4)}
                    moved = 32 * n * (sum(1 for c in use if c.n == n) + 1)
                    half = min(moved // 2, COPY_MAX)
                    row["copy_ms"] = round(timed(lambda: copy(half), a.reps) * (moved / 2 / half) * 1e3, 4)
                    row["over_copy"] = round(row["ms"] / row["copy_ms"], 2)
                    row["moved_GBps"] = round(moved / row["ms"] / 1e6, 1)
                    row["products_per_s"] = round(prog.n_mul * n / row["ms"] * 1e3)
                    row["of_vec_mul_rate"] = round(row["products_per_s"] / rows["vec_mul_products_per_s"], 3)
                    e.prof_enable(True)
                    e.prof_reset()
                    fn()
                    row["kernel_ms"] = round(e.prof_get("k_fr_program")[1], 4)
                    e.prof_enable(False)
                    rows[name if not block else "%s_block%d" % (name, block)] = row
                e.set_option("fr_program_block", 0)
        # the gate through the calls of before: products in the slots of `work`, q_C in the fifth, one lincomb with weights 1
        a_, b_, c_, ql, qr, qo, qm, qc = (c.ptr for c in cols[:8])
        slot = [ctypes.c_void_p(work.ptr.value + 32 * n * k) for k in range(5)]
        idx = (ctypes.c_uint32 * 5)(0, 1, 2, 3, 4)
        ones = b"".join(e._host_scalar(1, L.FR_MONT) for _ in range(5))

        def calls():
            for dst, sel, wires in ((slot[0], ql, (a_,)), (slot[1], qr, (b_,)), (slot[2], qo, (c_,)), (slot[3], qm, (a_, b_))):
                d2d(dst, sel, 32 * n)
                for w in wires:
                    ok(e.lib.kzg_fr_vec_mul(e.ctx, dst, w, n, L.FR_MONT, L.IN_DEVICE))
            d2d(slot[4], qc, 32 * n)
            ok(e.lib.kzg_fr_lincomb(e.ctx, work.ptr, n, 5, idx, ones, 5, L.FR_MONT, DEV, out.ptr))

        rows["gate"]["calls_ms"] = round(timed(calls, a.reps) * 1e3, 4)
        rows["gate"]["calls_over_program"] = round(rows["gate"]["calls_ms"] / rows["gate"]["ms"], 2)
        # the two routes agree on the bytes
        programs_out = e.alloc_scalars(n, L.FR_MONT)
        with e.fr_program(programs["gate"]) as plan:
            plan.run(cols[:8], [], n=n, outs=[programs_out])
        piece = min(n, 1 << 16)                   # every row up to 2^16; beyond, the first, a middle and the last 2^16 rows
        for at in sorted({0, (n - piece) // 2, n - piece}):
            assert programs_out.download(piece, at) == out.download(piece, at), at
        res["n"][str(kn)] = rows
        for buf in cols + [zh, out, work, programs_out]:
            buf.free()
    scratch.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
