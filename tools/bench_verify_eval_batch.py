#!/usr/bin/env python3
"""kzg_verify_eval_batch measurements (not part of bench.py): writes profiles/verify_eval_batch_bench.json and prints it as one JSON
line.  Honest openings of four polynomials of 2^12 coefficients at every point of their domain (proofs from kzg_witness_all_coeff,
FK20), everything in host memory; counts above the 16,384 generated openings repeat them (duplicates are allowed).  Per count (64,
16,384 = one chunk, 131,072 = eight chunks) and per configuration (trusted_points 0 / 1 x host_pairing 1 / 0), in one process on the
same inputs:
  batch_ms           median wall time of one blocking kzg_verify_eval_batch call after a warm-up, four commitments named by indices
  batch_no_idx_ms    the same with one commitment per opening (commitment_idx = NULL: the blob shape)
  per_opening_ms     the same for kzg_verify_eval (host_pairing does not touch it: measured once per trusted_points)
  kernel_ms          the indexed batch call's kernels with per-kernel timing on (kzg_prof_get); vcb_host_finish is the calling thread's
                     share
and the gate: at 16,384 openings both batch calls are faster than kzg_verify_eval with host_pairing = 1, for both trusted_points values
(exit status 1 otherwise).
   python tools/bench_verify_eval_batch.py [--reps 5] [--counts 64,16384,131072]"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import R_MODULUS, _raise, pack_scalars  # noqa: E402
from bench_verify_cosets import TAU, timed  # noqa: E402

KERNELS = ("k_decode_points", "k_powers", "k_veb_scalars", "k_vcb_fold", "k_vcb_fold2", "k_vcb_cweights", "k_vcb_bucket", "k_vcb_canon",
           "k_veb_yagg", "k_vcb_reduce", "k_vcb_finish", "vcb_host_finish")
R_CHALLENGE = 0x1234567_89ABCDEF_0FEDCBA9_87654321_0F1E2D3C_4B5A6978
LOG_N, POLYS = 12, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="64,16384,131072")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_eval_batch_bench.json"))
    a = ap.parse_args()
    N = 1 << LOG_N
    counts = [int(c) for c in a.counts.split(",")]
    res = {"polynomials": "%d x 2^%d" % (POLYS, LOG_N), "reps": a.reps, "runs": []}
    e = kzg_amd.Engine(0)
    params = kzg_amd.setup(e, TAU, N, g2_len=2)
    prover, plan = kzg_amd.KZGProver(params), kzg_amd.FK20Plan(e, params.gs, LOG_N)
    rng = random.Random(7)
    w = kzg_amd.compute_omega(N)[2]
    dom, x = [], 1
    for _ in range(N):
        dom.append(x)
        x = x * w % R_MODULUS
    xs1, ys1, cm, ws1 = pack_scalars(dom) * POLYS, b"", [], b""
    for _ in range(POLYS):
        coeffs = [rng.randrange(R_MODULUS) for _ in range(N)]
        poly = kzg_amd.Polynomial.new_from_coeffs(coeffs, N - 1)
        cm.append(prover.commit(poly))
        ys1 += pack_scalars(e.ntt(coeffs, LOG_N))
        ws1 += b"".join(prover.create_witness_all_points(poly, plan))
    plan.free()
    gen = POLYS * N
    top = max(counts)
    rep = (top + gen - 1) // gen
    xs, ys, ws = xs1 * rep, ys1 * rep, ws1 * rep
    which = [k // N % POLYS for k in range(top)]
    idx = (ctypes.c_uint32 * top)(*which)
    commitments, per_opening = b"".join(cm), b"".join(cm[m] * N for m in range(POLYS)) * rep
    r = R_CHALLENGE.to_bytes(32, "little")
    gs, hs = params.gs.handle, params.hs.handle
    gate_ok = True
    for count in counts:
        ok1, okn = ctypes.c_int(-1), ctypes.create_string_buffer(count)

        def batch():
            rc = e.lib.kzg_verify_eval_batch(e.ctx, gs, hs, xs, ys, L.FR_CANONICAL, commitments, POLYS, idx, ws, L.G1_AFFINE_MONT, count, r,
                                             ctypes.byref(ok1))
            if rc:
                _raise(e, rc)

        def batch_no_idx():
            rc = e.lib.kzg_verify_eval_batch(e.ctx, gs, hs, xs, ys, L.FR_CANONICAL, per_opening, count, None, ws, L.G1_AFFINE_MONT, count, r,
                                             ctypes.byref(ok1))
            if rc:
                _raise(e, rc)

        def per():
            rc = e.lib.kzg_verify_eval(e.ctx, gs, hs, xs, ys, L.FR_CANONICAL, per_opening, ws, L.G1_AFFINE_MONT, count, okn)
            if rc:
                _raise(e, rc)
        for trusted in (0, 1):
            e.set_option("trusted_points", trusted)
            t_per = timed(per, a.reps)
            assert okn.raw == b"\x01" * count, "an honest opening did not verify"
            for hp in (1, 0):
                e.set_option("host_pairing", hp)
                t_batch = timed(batch, a.reps)
                assert ok1.value == 1, "the honest openings did not verify as a batch"
                ok1.value = -1
                t_blob = timed(batch_no_idx, a.reps)
                assert ok1.value == 1, "the honest openings did not verify as a batch without indices"
                e.prof_enable(True)
                e.prof_reset()
                batch()
                kern = {name: round(e.prof_get(name)[1], 3) for name in KERNELS if e.prof_get(name)[0]}
                e.prof_enable(False)
                run = {"openings": count, "trusted_points": trusted, "host_pairing": hp, "batch_ms": round(t_batch * 1e3, 3),
                       "batch_no_idx_ms": round(t_blob * 1e3, 3), "per_opening_ms": round(t_per * 1e3, 3),
                       "speedup": round(t_per / t_batch, 2), "kernel_ms": kern}
                res["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
                if count == 16384 and hp == 1 and not (t_batch < t_per and t_blob < t_per):
                    gate_ok = False
    e.set_option("trusted_points", 0)
    e.set_option("host_pairing", 1)
    split = [x for x in res["runs"] if x["openings"] == 16384 and x["trusted_points"] == 0 and x["host_pairing"] == 1]
    res["split_16384_ms"] = split[0]["kernel_ms"] if split else None
    res["gate_16384_batch_faster"] = gate_ok
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
