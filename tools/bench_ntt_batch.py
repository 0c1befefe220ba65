#!/usr/bin/env python3
"""kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch measurements (not part of bench.py): prints one JSON line and writes it to --out.
Device buffers, one process.  Per shape "2^k x B" (prefix "coset " for the coset call), medians of wall time around blocking calls
after a warm-up, in ms:
  batch_ms     one kzg_ntt_fr_batch (kzg_coset_ntt_fr_batch) call over the B vectors
  loop_ms      B kzg_ntt_fr (kzg_coset_ntt_fr) calls over the same buffer, one per vector
  loop2_ms     the same loop measured a second time: |loop_ms - loop2_ms| is the spread of this box for this shape
  copy_ms      a device-to-device copy of the same bytes, synchronised: the bandwidth floor
  batch/loop, batch/copy   the ratios
A library without the batch calls (an older commit) gives the loop and copy columns alone, so the loop can be measured there with
the same script.  The transforms run in place on whatever the previous one left: full-width residues at every step.
   python tools/bench_ntt_batch.py [--reps 9] [--shapes 6x16384,12x256,c12x256] [--option ntt_batch_loop_from=21]"""
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

SHAPES = "6x16384,8x4096,12x64,12x256,13x128,14x64,16x16,18x8,20x4,c12x256,c16x16"


def timed(fn, reps):
    fn()  # warm-up: code objects, plans and tables of this shape
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def bind(lib, name, argtypes):
    """the batch entry point, or None where the library does not have it"""
    try:
        fn = getattr(lib, name)
    except AttributeError:
        return None
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--option", action="append", default=[], help="key=value for kzg_ctx_set_option, repeatable")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_batch_bench.json"))
    a = ap.parse_args()
    e = kzg_amd.Engine(0)
    for kv in a.option:
        k, _, v = kv.partition("=")
        rc = e.lib.kzg_ctx_set_option(e.ctx, k.encode(), int(v))
        if rc:
            _raise(e, rc)
    vp, sz, i32, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    batch_fn = bind(e.lib, "kzg_ntt_fr_batch", [vp, vp, u32, sz, sz, i32, i32])
    coset_batch_fn = bind(e.lib, "kzg_coset_ntt_fr_batch", [vp, vp, u32, sz, sz, i32, i32, i32])
    info = ctypes.create_string_buffer(1024)
    e.lib.kzg_runtime_info(info, 1024)
    hip = ctypes.CDLL(info.value.decode().split("hip=")[1].split()[0])  # the runtime the library itself is bound to
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [vp, vp, sz, i32], i32
    hip.hipDeviceSynchronize.restype = i32
    res = {"options": a.option, "reps": a.reps, "shapes": {}}
    for s in a.shapes.split(","):
        coset = s.startswith("c")
        k, B = (int(v) for v in s.lstrip("c").split("x"))
        n = 1 << k
        key = ("coset " if coset else "") + "2^%d x %d" % (k, B)
        buf = e.alloc_scalars(B * n).fill_random(k + B)
        dst = e.alloc_scalars(B * n)
        ptrs = [ctypes.c_void_p(buf.ptr.value + b * n * 32) for b in range(B)]

        def ok(rc):
            if rc:
                _raise(e, rc)

        def loop():
            if coset:
                for p in ptrs:
                    ok(e.lib.kzg_coset_ntt_fr(e.ctx, p, k, 0, L.FR_CANONICAL, L.IN_DEVICE))
            else:
                for p in ptrs:
                    ok(e.lib.kzg_ntt_fr(e.ctx, p, k, 0, L.IN_DEVICE))

        def batch():
            if coset:
                ok(coset_batch_fn(e.ctx, buf.ptr, k, B, 0, 0, L.FR_CANONICAL, L.IN_DEVICE))
            else:
                ok(batch_fn(e.ctx, buf.ptr, k, B, 0, 0, L.IN_DEVICE))

        def copy():
            assert hip.hipMemcpy(dst.ptr, buf.ptr, B * n * 32, 3) == 0  # hipMemcpyDeviceToDevice
            assert hip.hipDeviceSynchronize() == 0

        row = {}
        if (coset_batch_fn if coset else batch_fn) is not None:
            row["batch_ms"] = round(timed(batch, a.reps), 4)
        row["loop_ms"] = round(timed(loop, a.reps), 4)
        if "batch_ms" in row:
            row["batch_ms_again"] = round(timed(batch, a.reps), 4)
        row["loop2_ms"] = round(timed(loop, a.reps), 4)
        row["copy_ms"] = round(timed(copy, a.reps), 4)
        if "batch_ms" in row:
            row["batch/loop"] = round(row["batch_ms"] / row["loop_ms"], 4)
            row["batch/copy"] = round(row["batch_ms"] / row["copy_ms"], 2)
        res["shapes"][key] = row
        buf.free()
        dst.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
