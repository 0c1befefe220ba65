#!/usr/bin/env python3
"""kzg_verify_cosets_batch measurements (not part of bench.py): writes profiles/verify_cosets_batch_bench.json and prints it as one
JSON line.  Honest cells of one 2^20 / 64 polynomial (proofs from kzg_witness_cosets_coeff, cells in a device buffer); counts above
the polynomial's 16,384 cells repeat them (duplicate (commitment, coset) pairs are allowed).  Per count (64, 16,384 = one chunk,
131,072 = eight chunks) and per configuration (trusted_points 0 / 1 x host_pairing 0 / 1), in one process on the same inputs:
  batch_ms           median wall time of one blocking kzg_verify_cosets_batch call after a warm-up
  per_cell_ms        the same for kzg_verify_cosets (host_pairing does not touch it: measured once per trusted_points)
  kernel_ms          the batch call's kernels with per-kernel timing on (kzg_prof_get); vcb_host_finish is the calling thread's share
and the gate: at 16,384 cells the batch call is faster than kzg_verify_cosets in every configuration (exit status 1 otherwise).
   python tools/bench_verify_cosets_batch.py [--reps 5] [--shape 20/6] [--counts 64,16384,131072]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import _raise  # noqa: E402
from bench_verify_cosets import TAU, open_all, timed  # noqa: E402

KERNELS = ("k_decode_points", "k_powers", "k_vc_interp", "k_vcb_scalars", "k_vcb_fold", "k_vcb_fold2", "k_vcb_cweights", "k_vcb_bucket",
           "k_vcb_canon", "k_vcb_reduce", "k_vc_sum", "k_vcb_finish", "vcb_host_finish")
R_CHALLENGE = 0x1234567_89ABCDEF_0FEDCBA9_87654321_0F1E2D3C_4B5A6978


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="20/6")
    ap.add_argument("--counts", default="64,16384,131072")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cosets_batch_bench.json"))
    a = ap.parse_args()
    k, j = (int(v) for v in a.shape.split("/"))
    N, l = 1 << k, 1 << j
    K = N // l
    counts = [int(c) for c in a.counts.split(",")]
    res = {"shape": "2^%d/%d" % (k, l), "reps": a.reps, "runs": []}
    e = kzg_amd.Engine(0)
    params = kzg_amd.setup(e, TAU, N, g2_len=l + 1)
    commitment, cells, proofs, _r, _c = open_all(e, params, k, j, 7)
    ver = kzg_amd.CosetVerifier(e, params, k, j)
    top = max(counts)
    rep = (top + K - 1) // K
    dcells = e.alloc_scalars(rep * K * l)
    for t in range(rep):
        rc = e.lib.kzg_dev_upload(e.ctx, ctypes.c_void_p(dcells.ptr.value + t * K * l * 32), cells, K * l * 32)
        if rc:
            _raise(e, rc)
    proofs = proofs * rep
    idx, ids = (ctypes.c_uint32 * top)(), (ctypes.c_size_t * top)(*[i % K for i in range(top)])
    r = R_CHALLENGE.to_bytes(32, "little")
    gate_ok = True
    for count in counts:
        ok1, okn = ctypes.c_int(-1), ctypes.create_string_buffer(count)

        def batch():
            rc = e.lib.kzg_verify_cosets_batch(e.ctx, ver.handle, commitment, 1, idx, ids, dcells.ptr, proofs, count, r, L.FR_CANONICAL,
                                               L.G1_AFFINE_MONT, L.IN_DEVICE, ctypes.byref(ok1))
            if rc:
                _raise(e, rc)

        def per_cell():
            rc = e.lib.kzg_verify_cosets(e.ctx, ver.handle, commitment, 1, idx, ids, dcells.ptr, proofs, count, L.FR_CANONICAL, L.G1_AFFINE_MONT,
                                         L.IN_DEVICE, okn)
            if rc:
                _raise(e, rc)
        for trusted in (0, 1):
            e.set_option("trusted_points", trusted)
            t_cell = timed(per_cell, a.reps)
            assert okn.raw == b"\x01" * count, "an honest cell did not verify"
            for hp in (0, 1):
                e.set_option("host_pairing", hp)
                t_batch = timed(batch, a.reps)
                assert ok1.value == 1, "the honest cells did not verify as a batch"
                e.prof_enable(True)
                e.prof_reset()
                batch()
                kern = {name: round(e.prof_get(name)[1], 3) for name in KERNELS if e.prof_get(name)[0]}
                e.prof_enable(False)
                run = {"cells": count, "trusted_points": trusted, "host_pairing": hp, "batch_ms": round(t_batch * 1e3, 3),
                       "per_cell_ms": round(t_cell * 1e3, 3), "speedup": round(t_cell / t_batch, 2), "kernel_ms": kern}
                res["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
                if count == 16384 and not t_batch < t_cell:
                    gate_ok = False
    e.set_option("trusted_points", 0)
    e.set_option("host_pairing", 1)
    small = [x for x in res["runs"] if x["cells"] == min(counts) and x["trusted_points"] == 0]
    res["host_pairing_at_%d_cells_ms" % min(counts)] = {str(x["host_pairing"]): x["batch_ms"] for x in small}
    res["host_finish_ms"] = [x["kernel_ms"].get("vcb_host_finish") for x in res["runs"] if x["host_pairing"] == 1]
    res["gate_16384_batch_faster"] = gate_ok
    dcells.free()
    ver.free()
    params.gs.free()
    params.hs.free()
    e.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if gate_ok else 1


if __name__ == "__main__":
    sys.exit(main())
