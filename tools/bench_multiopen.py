#!/usr/bin/env python3
"""Multiproof measurements (not part of bench.py): writes profiles/multiopen_bench.json and prints it as one JSON line.
At d = 2^log_d, evaluations, g and the group elements in device buffers, medians of blocking calls after a warm-up, one process, the
variants of a comparison alternated call by call; per N in --ns (N claims on N polynomials):
  multi_distinct_ms   (a) kzg_multiopen_eval_commit + kzg_multiopen_eval_finish, N distinct off-domain points: N values, TWO elements
  singles_ms              kzg_open_eval of the same N claims: N values, N witnesses
  multi_shared_ms     (b) the same two calls with ONE shared point          fold_open_ms   kzg_open_fold_eval of the same polynomials
  accum_ms, lincomb_ms, fold_ms   (c) k_multiopen_accum (all its launches of one first phase, U = N distinct points), k_fr_lincomb of the
                      second phase over the N vectors, and k_fr_fold over the same N vectors (kzg_prof_get); fold_spread_ms: max - min
                      of the fold over the repetitions; accum_bound_ms = fold_ms (N + U) / N + fold_spread_ms: the accumulation pass
                      moves (N + U) / N times the fold's bytes; accum_within_bound says whether accum_ms keeps to it
  verify_multi_ms     (d) kzg_verify_multiopen of the N claims             verify_singles_ms   kzg_verify_eval of the N openings
  kernels_ms          per-kernel time of one first and one second phase with N distinct points (kzg_prof_get)
   python tools/bench_multiopen.py [--log-d 20] [--ns 4,16,64] [--reps 7]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kzg_amd  # noqa: E402
from kzg_amd import _lib as L  # noqa: E402
from kzg_amd.api import R_MODULUS, _raise  # noqa: E402

KERNELS = ("k_multiopen_accum", "k_multiopen_ysum", "k_fr_lincomb", "k_open_powtab", "k_open_denoms", "k_batch_inverse", "k_open_eval_partials_idx",
           "k_open_eval_finish_idx", "k_open_eval_partials", "k_open_eval_finish", "k_open_quotient", "k_accum_affine")
AFF = L.G1_AFFINE_MONT
DEV = L.IN_DEVICE | L.OUT_DEVICE
CAN = L.FR_CANONICAL


def alternated(fns, reps):
    """medians of the blocking calls fns[0], fns[1], ... taken in turn, after one warm-up each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [statistics.median(t) * 1e3 for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-d", type=int, default=20)
    ap.add_argument("--ns", default="4,16,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiopen_bench.json"))
    a = ap.parse_args()
    k, ns = a.log_d, [int(x) for x in a.ns.split(",")]
    d, T = 1 << k, max(ns)
    rng = random.Random(k)
    tau = rng.randrange(R_MODULUS)
    le = lambda v: (v % R_MODULUS).to_bytes(32, "little")  # noqa: E731
    e = kzg_amd.Engine(0)
    lag = kzg_amd.setup_lagrange(e, tau, d)
    small = kzg_amd.setup(e, tau, 2, g2_len=2)  # gs[0], hs[0], hs[1]: all the verifiers read
    evals = e.alloc_scalars(T * d).fill_random(k)
    g = e.alloc_scalars(d)
    folded = e.alloc_scalars(d)
    out = e.alloc_scalars(T * 3)  # T x 96 bytes
    ys = ctypes.create_string_buffer(32 * T)
    vt = ctypes.create_string_buffer(32)
    zs_all = [rng.randrange(R_MODULUS) for _ in range(T)]
    r, t = le(rng.randrange(1, R_MODULUS)), le(rng.randrange(R_MODULUS))  # (a benchmark: a protocol hashes D into t)

    def ok(rc):
        if rc:
            _raise(e, rc)

    def multi(n, zb):
        ok(e.lib.kzg_multiopen_eval_commit(e.ctx, lag.handle, evals.ptr, d, n, None, zb, n, r, CAN, DEV, ys, g.ptr, out.ptr, AFF))
        ok(e.lib.kzg_multiopen_eval_finish(e.ctx, lag.handle, evals.ptr, d, n, None, zb, n, r, t, g.ptr, CAN, DEV, vt,
                                           ctypes.c_void_p(out.ptr.value + 96), AFF))

    def singles(n, zb):
        ok(e.lib.kzg_open_eval(e.ctx, lag.handle, evals.ptr, d, n, zb, CAN, DEV, ys, out.ptr, AFF))

    def fold_open(n, zb):
        ok(e.lib.kzg_open_fold_eval(e.ctx, lag.handle, evals.ptr, d, n, 1, zb[:32], r, CAN, DEV, ys, out.ptr, AFF))

    def points(n):
        return out.download(n * 3)

    res = {"log_d": k, "ns": ns, "per_n": {}}
    ok(e.lib.kzg_msm_g1_batch(e.ctx, lag.handle, 0, evals.ptr, d, T, CAN, DEV, out.ptr, AFF))
    commitments = points(T)
    for n in ns:
        reps = a.reps if n <= 16 else max(3, a.reps // 2)
        zb = b"".join(le(z) for z in zs_all[:n])
        zb1 = le(zs_all[0]) * n
        row = {}
        row["multi_distinct_ms"], row["singles_ms"] = alternated([lambda: multi(n, zb), lambda: singles(n, zb)], reps)
        row["multi_shared_ms"], row["fold_open_ms"] = alternated([lambda: multi(n, zb1), lambda: fold_open(n, zb1)], reps)
        # (d) the verifiers on honest proofs of the distinct-point claims
        singles(n, zb)
        ys_single, w_single = ys.raw[:32 * n], points(n)
        multi(n, zb)
        assert ys.raw[:32 * n] == ys_single, "the two routes disagree on the values"
        proof = points(2)
        okv, oks = ctypes.c_int(-1), ctypes.create_string_buffer(n)
        row["verify_multi_ms"], row["verify_singles_ms"] = alternated([
            lambda: ok(e.lib.kzg_verify_multiopen(e.ctx, small.gs.handle, small.hs.handle, zb, ys_single, CAN, commitments[:96 * n], n, None, n, r, t,
                                                  proof[:96], proof[96:], AFF, ctypes.byref(okv))),
            lambda: ok(e.lib.kzg_verify_eval(e.ctx, small.gs.handle, small.hs.handle, zb, ys_single, CAN, commitments[:96 * n], w_single, AFF, n, oks))], reps)
        assert okv.value == 1 and oks.raw == b"\x01" * n, "an honest opening was rejected"
        # (c) the kernels: the accumulation pass and the second phase's combination against the fold of the same n vectors
        e.prof_enable(True)
        acc, lin, fold, kernels = [], [], [], {}
        for _ in range(reps + 1):
            e.prof_reset()
            multi(n, zb)
            kernels = {kn: round(e.prof_get(kn)[1], 3) for kn in KERNELS}
            acc.append(e.prof_get("k_multiopen_accum")[1])
            lin.append(e.prof_get("k_fr_lincomb")[1])
            e.prof_reset()
            ok(e.lib.kzg_fr_fold(e.ctx, evals.ptr, d, n, 1, r, CAN, DEV, folded.ptr))
            fold.append(e.prof_get("k_fr_fold")[1])
        e.prof_enable(False)
        acc, lin, fold = acc[1:], lin[1:], fold[1:]  # (the first round warms up)
        row["accum_ms"], row["lincomb_ms"], row["fold_ms"] = statistics.median(acc), statistics.median(lin), statistics.median(fold)
        row["fold_spread_ms"] = max(fold) - min(fold)
        row["accum_bound_ms"] = row["fold_ms"] * (n + n) / n + row["fold_spread_ms"]
        row = {key: round(v, 3) for key, v in row.items()}
        row["accum_within_bound"] = row["accum_ms"] <= row["accum_bound_ms"]
        row["a_multi_over_singles"] = round(row["multi_distinct_ms"] / row["singles_ms"], 3)
        row["b_multi_over_fold"] = round(row["multi_shared_ms"] / row["fold_open_ms"], 3)
        row["d_verify_multi_over_singles"] = round(row["verify_multi_ms"] / row["verify_singles_ms"], 3)
        row["kernels_ms"] = kernels
        res["per_n"][str(n)] = row
    for buf in (evals, g, folded, out):
        buf.free()
    lag.free()
    small.gs.free()
    small.hs.free()
    e.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
