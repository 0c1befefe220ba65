#!/usr/bin/env python3
"""Measurements of kzg_msm_g2_bucket and kzg_verify_eval_tree (not part of bench.py): writes profiles/witness_tree_bench.json and prints it
as one JSON line.  One MI355X, one process; SRSs and plans are built outside the timed region; every figure is the median wall time
of --reps blocking calls after one warm-up call.
  (a) g2_msm     kzg_msm_g2_bucket against kzg_msm_g2 on the same host scalars at n = 64, 1024, 16385, 2^16; the bucket call alone at
                 2^18 and 2^20, also with device-resident scalars; the per-kernel split at 16385 (kzg_prof_get, a run of its own)
  (b) prover     kzg_witness_coeff_tree (batch 1 and 16, n = 2^20, coefficients resident, witnesses and remainders to the host) against
                 kzg_witness_coeff_batched (one call per polynomial, after one warming call so that its point-set cache is hot) at
                 k = 1024, 4096, 16384; the tree call alone at 2^16, 2^18 and 2^20 - 2^10
  (c) verifier   kzg_verify_eval_tree (count 1 and 16) against kzg_verify_eval_batched (one call per opening; it rebuilds z and hz in
                 every call) at k = 1024, 4096, 16384; the tree call alone at 2^16 and 2^18.  The tuples are valid points that do not
                 verify: the work of a check does not depend on its verdict.
THE GATE: at n = 16385 the bucket call must take less time than kzg_msm_g2 in the same run; exit status 1 otherwise.
   python tools/bench_witness_tree.py [--reps 5]"""
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

CAN = L.FR_CANONICAL
GATE_N = 16385
OLD_MAX = 16384


def timed(fn, reps):
    """median seconds of `reps` blocking calls after one warm-up call"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--g2-both", default="64,1024,16385,65536")
    ap.add_argument("--g2-alone", default="262144,1048576")
    ap.add_argument("--ks-both", default="1024,4096,16384")
    ap.add_argument("--ks-alone", default="65536,262144")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--pk-alone", default="65536,262144,1047552")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_tree_bench.json"))
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    g2_both, g2_alone, ks_both, ks_alone = ints(a.g2_both), ints(a.g2_alone), ints(a.ks_both), ints(a.ks_alone)
    e = kzg_amd.Engine(0)

    def ok(rc):
        if rc:
            _raise(e, rc)

    nmax, kmax = max(g2_both + g2_alone + [k + 1 for k in ks_both + ks_alone]), max(ks_both + ks_alone)
    t0 = time.perf_counter()
    n_poly, pk_alone = 1 << a.log_n, ints(a.pk_alone)
    params = kzg_amd.setup(e, 0x5EED5EED, max(kmax, n_poly), g2_len=nmax)
    setup_s = time.perf_counter() - t0
    hs, gs = params.hs, params.gs
    sc_dev = e.alloc_scalars(nmax).fill_random(91)
    sc = sc_dev.download()
    res = {"device": "MI355X", "reps": a.reps, "setup_s": round(setup_s, 2), "g2_msm": {}, "verifier": {},
           "prover": {}}
    out, out2 = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192)

    # ---- (a) the G2 sum ----
    for n in g2_both + g2_alone:
        row = {}
        bucket = lambda: ok(e.lib.kzg_msm_g2_bucket(e.ctx, hs.handle, 0, sc, n, CAN, 0, out, L.G2_AFFINE_MONT))  # noqa: E731
        row["bucket_ms"] = timed(bucket, a.reps) * 1e3
        row["bucket_device_scalars_ms"] = timed(lambda: ok(e.lib.kzg_msm_g2_bucket(e.ctx, hs.handle, 0, sc_dev.ptr, n, CAN, L.IN_DEVICE, out,
                                                                                   L.G2_AFFINE_MONT)), a.reps) * 1e3
        if n in g2_both:
            row["msm_g2_ms"] = timed(lambda: ok(e.lib.kzg_msm_g2(e.ctx, hs.handle, 0, sc, n, CAN, out2, L.G2_AFFINE_MONT)), a.reps) * 1e3
            assert out.raw == out2.raw, "the two calls disagree at n = %d" % n
            row["bucket_over_msm_g2"] = row["bucket_ms"] / row["msm_g2_ms"]
        if n == GATE_N:
            e.prof_enable(True)
            e.prof_reset()
            bucket()
            row["stage_ms"] = {kn: round(ms, 4) for kn, (cnt, ms) in e.prof_all().items() if cnt}
            e.prof_reset()
            ok(e.lib.kzg_msm_g2(e.ctx, hs.handle, 0, sc, n, CAN, out2, L.G2_AFFINE_MONT))
            row["msm_g2_stage_ms"] = {kn: round(ms, 4) for kn, (cnt, ms) in e.prof_all().items() if cnt}
            e.prof_enable(False)
        row = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}
        res["g2_msm"][str(n)] = row
        print("g2 n", n, json.dumps(row), file=sys.stderr, flush=True)

    # ---- (b) the prover ----
    xs_all = e.alloc_scalars(max(kmax, max(pk_alone))).fill_random(92).download()
    coeffs = e.alloc_scalars(16 * n_poly).fill_random(93)
    for k in ks_both + pk_alone:
        xs = xs_all[:32 * k]
        tree = e.point_tree(kzg_amd.api.unpack_scalars(xs))
        row = {}
        ow, orr = ctypes.create_string_buffer(96 * 16), ctypes.create_string_buffer(32 * 16 * k)
        for batch in (1, 16):
            row["tree_batch%d_ms" % batch] = timed(lambda: ok(e.lib.kzg_witness_coeff_tree(e.ctx, gs.handle, tree.handle, coeffs.ptr, n_poly, batch, None, CAN,
                                                                                           L.IN_DEVICE, ow, L.G1_AFFINE_MONT, orr, None)), a.reps) * 1e3
        if k <= OLD_MAX:
            ys = kzg_amd.api.pack_scalars([v for vs in tree.eval_batch(coeffs, n=n_poly, batch=16) for v in vs])
            rl = ctypes.c_size_t()
            w2, r2 = ctypes.create_string_buffer(96), ctypes.create_string_buffer(32 * max(k, 2))
            for batch in (1, 16):
                def old():
                    for b in range(batch):
                        ok(e.lib.kzg_witness_coeff_batched(e.ctx, gs.handle, ctypes.c_void_p(coeffs.ptr.value + 32 * b * n_poly), n_poly, xs,
                                                           ys[32 * b * k:32 * (b + 1) * k], k, CAN, L.IN_DEVICE, w2, L.G1_AFFINE_MONT, r2, ctypes.byref(rl)))
                row["batched_batch%d_ms" % batch] = timed(old, a.reps) * 1e3  # (timed() warms once: the point-set cache is hot)
                row["tree_over_batched_batch%d" % batch] = row["tree_batch%d_ms" % batch] / row["batched_batch%d_ms" % batch]
            assert w2.raw == ow.raw[96 * 15:96 * 16], "the two provers disagree at k = %d" % k
        tree.close()
        row = {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in row.items()}
        res["prover"][str(k)] = row
        print("prove k", k, json.dumps(row), file=sys.stderr, flush=True)
    coeffs.free()

    # ---- (c) the verifier ----
    pts = gs.download(1, 2)
    cm, wt = pts[:96], pts[96:]
    for k in ks_both + ks_alone:
        xs = xs_all[:32 * k]
        t0 = time.perf_counter()
        tree = e.point_tree(kzg_amd.api.unpack_scalars(xs))
        row = {"plan_setup_ms": round((time.perf_counter() - t0) * 1e3, 2)}
        r = sc[:32 * k]
        for count in (1, 16):
            okb = ctypes.create_string_buffer(count)
            row["tree_count%d_ms" % count] = timed(lambda: ok(e.lib.kzg_verify_eval_tree(e.ctx, gs.handle, hs.handle, tree.handle, r * count, CAN, cm * count,
                                                                                         wt * count, L.G1_AFFINE_MONT, count, okb)), a.reps) * 1e3
            if k <= OLD_MAX:
                v = ctypes.c_int()

                def old():
                    for _ in range(count):
                        ok(e.lib.kzg_verify_eval_batched(e.ctx, gs.handle, hs.handle, xs, k, r, k, CAN, cm, wt, L.G1_AFFINE_MONT, ctypes.byref(v)))
                row["batched_count%d_ms" % count] = timed(old, a.reps) * 1e3
                row["tree_over_batched_count%d" % count] = row["tree_count%d_ms" % count] / row["batched_count%d_ms" % count]
        tree.close()
        row = {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in row.items()}
        res["verifier"][str(k)] = row
        print("verify k", k, json.dumps(row), file=sys.stderr, flush=True)

    gate = res["g2_msm"].get(str(GATE_N))
    res["gate"] = None if gate is None else {"n": GATE_N, "bucket_ms": gate["bucket_ms"], "msm_g2_ms": gate["msm_g2_ms"],
                                             "passed": gate["bucket_ms"] < gate["msm_g2_ms"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    e.close()
    return 0 if res["gate"] and res["gate"]["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
