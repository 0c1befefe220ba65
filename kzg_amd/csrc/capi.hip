// capi.hip -- the extern "C" entry points declared in include/kzg_mi355x.h that mirror KZGProver / KZGProverEvalForm / EvaluationDomain
// method by method (MSM / commit, the batched pipeline, witnesses, NTT, polynomial helpers, verify_poly, the unit-test hooks), with the
// staging and result helpers they share.  The context, lanes, streams and profiling they run on live in runtime.hip.
#include <algorithm>

#include "common.h"
#include "emit.h"
#include "multiopen_plan.h"

namespace kzg {

// ---------------------------------------------------------------------------------------------
// helpers shared by the entry points
// ---------------------------------------------------------------------------------------------
static int host_scalar(kzg_ctx *ctx, const void *s, int sfmt, Fr *mont) {
    Fr v;
    memcpy(v.v, s, 32);
    if (sfmt == KZG_FR_CANONICAL_LE_32) {
        if (!is_canonical(v)) return fail(ctx, KZG_ERR_SHAPE, "scalar not canonical (>= r)");
        v = to_mont(v);
    } else if (sfmt != KZG_FR_MONT_LE_32) {
        return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    }
    *mont = v;
    return KZG_OK;
}

static void scalar_out(const Fr &mont, int sfmt, void *dst) {
    Fr v = sfmt == KZG_FR_CANONICAL_LE_32 ? from_mont(mont) : mont;
    memcpy(dst, v.v, 32);
}

// bring `bytes` of input to the device (no-op for device-resident input)
static int stage_in(kzg_ctx *ctx, int lane, const void *src, size_t bytes, int flags, const void **dptr) {
    if (flags & KZG_IN_DEVICE) {
        *dptr = src;
        return KZG_OK;
    }
    void *d = lane_alloc(ctx, lane, bytes ? bytes : 16);
    if (!d) return fail(ctx, KZG_ERR_ALLOC, "input staging not reserved");
    if (bytes) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->lanes[lane].stream));
    *dptr = d;
    return KZG_OK;
}

static size_t stage_bytes(size_t bytes, int flags) { return (flags & KZG_IN_DEVICE) ? 0 : align_up(bytes + 256, 256); }

// The lane's last sort with the result (oversized bins: what the next calls decide on, common.h heavy_last): 4 bytes into the
// lane's pinned buffer before the wait, looked at after it.
static int heavy_pickup_enqueue(kzg_ctx *ctx, int lane) {
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(ctx->lanes[lane].pinned + 512, ctx->d_lane_heavy + lane, 4, hipMemcpyDeviceToHost, ctx->lanes[lane].stream));
    return KZG_OK;
}
static void heavy_pickup_read(kzg_ctx *ctx, int lane) {
    uint32_t hseq;
    memcpy(&hseq, ctx->lanes[lane].pinned + 512, 4);
    Lane &l = ctx->lanes[lane];
    if (l.heavy_seq == l.heavy_seen) return;  // no MSM on this lane since the last look
    l.heavy_seen = l.heavy_seq;
    if (hseq == l.heavy_seq) ctx->heavy_last.store(ctx->msm_count.load(std::memory_order_relaxed), std::memory_order_relaxed);
}

// result point: XYZZ on device -> ofmt at `out` (host or device)
int finish_point(kzg_ctx *ctx, int lane, const MsmPoint *d_pt, void *out, int ofmt, int flags) {
    size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_TRY(lane_pinned(ctx, lane, 4096));
    if (flags & KZG_OUT_DEVICE) {
        KZG_TRY(emit_point(ctx, lane, d_pt, out, ofmt));
        KZG_TRY(heavy_pickup_enqueue(ctx, lane));
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    } else {
        if (ctx->opt_host_affine) {
            // A lone result for the host: copy the XYZZ point out and convert it on the calling thread with the same code
            // (emit.h, compiled for the host): a CPU core does the Fq inversion of to_affine in a few microseconds, one GPU lane
            // needs ~90 us for it, and this sits on the critical path of every blocking commit / create_witness.
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(ctx->lanes[lane].pinned, d_pt, sizeof(MsmPoint), hipMemcpyDeviceToHost, st));
            KZG_TRY(heavy_pickup_enqueue(ctx, lane));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
            MsmPoint pt;
            memcpy(&pt, ctx->lanes[lane].pinned, sizeof pt);
            alignas(16) uint8_t buf[144];
            emit_one(pt, buf, ofmt);
            memcpy(out, buf, psz);
        } else {
            // the kernel writes the <= 144 bytes straight into the lane's pinned host buffer (device-mapped, coherent)
            KZG_TRY(emit_point(ctx, lane, d_pt, ctx->lanes[lane].pinned, ofmt));
            KZG_TRY(heavy_pickup_enqueue(ctx, lane));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
            memcpy(out, ctx->lanes[lane].pinned, psz);
        }
    }
    heavy_pickup_read(ctx, lane);
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

static int check_sfmt(kzg_ctx *ctx, int sfmt) {
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    return KZG_OK;
}

static bool is_pow2(size_t x) { return x && !(x & (x - 1)); }
// element counts whose byte sizes cannot overflow the arena arithmetic (2^40 Fr elements = 32 TiB: far beyond any device)
static bool count_ok(size_t n) { return n <= ((size_t)1 << 40); }

#ifdef KZG_TEST_HOOKS
// ---------------------------------------------------------------------------------------------
// device unit-test kernels (only in the -DKZG_TEST_HOOKS build: kzg_amd/libkzg_mi355x_hooks.so, include/kzg_mi355x_test.h)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_test_fr_mul(const Fr *a, const Fr *b, size_t n, Fr *o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = mul(a[i], b[i]);
}
__global__ __launch_bounds__(256) void k_test_fq_mul(const Fq *a, const Fq *b, size_t n, Fq *o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = mul(a[i], b[i]);
}
__global__ __launch_bounds__(256) void k_test_fr_inv(const Fr *a, size_t n, Fr *o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i].is_zero() ? Fr::zero() : inv(a[i]);
}
__global__ __launch_bounds__(256) void k_test_g1_add(const G1Affine *a, const G1Affine *b, size_t n, G1Affine *o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // exercise both the mixed and the general addition on de-normalised operands
    G1Xyzz p = g1_madd(G1Xyzz::from_affine(a[i]), b[i]);
    G1Xyzz pa = g1_madd(g1_dbl(G1Xyzz::from_affine(a[i])), g1_neg(a[i]));
    G1Xyzz pb = g1_madd(g1_dbl(G1Xyzz::from_affine(b[i])), g1_neg(b[i]));
    G1Xyzz q = g1_add(pa, pb);
    G1Affine r1 = g1_to_affine(p), r2 = g1_to_affine(q);
    bool same = (r1.x == r2.x) && (r1.y == r2.y);
    o[i] = same ? r1 : G1Affine{Fq::one(), Fq::one()};  // (1,1) is not on the curve: flags a mismatch
}
__global__ __launch_bounds__(256) void k_test_g1_mul(const G1Affine *p, const Fr *k, size_t n, G1Affine *o) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr kk = k[i];
    o[i] = g1_to_affine(g1_scalar_mul(p[i], kk.v));
}

#endif  // KZG_TEST_HOOKS

}  // namespace kzg

using namespace kzg;

// ---------------------------------------------------------------------------------------------
// MSM
// ---------------------------------------------------------------------------------------------
extern "C" int kzg_msm_g1(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n, int sfmt,
                          int flags, void *out, int ofmt) {
    if (!ctx || !srs || !out || (!scalars && n)) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (n > srs->n || offset > srs->n - n) return fail(ctx, KZG_ERR_SHAPE, "MSM range exceeds the SRS (reference: slice index panic)");
    KZG_TRY(lane_reserve(ctx, lane, msm_workspace_bytes(srs, n) + stage_bytes(n * 32, flags) + 8192));
    const void *d_sc = nullptr;
    KZG_TRY(stage_in(ctx, lane, scalars, n * 32, flags, &d_sc));
    MsmPoint *res = nullptr;
    KZG_TRY(lease_msm(ctx, ls, srs, offset, d_sc, n, sfmt, &res));
    return finish_point(ctx, lane, res, out, ofmt, flags);
}

extern "C" int kzg_commit_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, int sfmt, int flags,
                                void *out, int ofmt) {
    return kzg_msm_g1(ctx, srs, 0, coeffs, n, sfmt, flags, out, ofmt);
}

extern "C" int kzg_commit_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, int sfmt, int flags,
                               void *out, int ofmt) {
    if (!ctx || !lagrange) return KZG_ERR_SHAPE;
    if (d != lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d) (src/eval_form.rs:115)");
    return kzg_msm_g1(ctx, lagrange, 0, evals, d, sfmt, flags, out, ofmt);
}

// ---- the batched pipeline shared by kzg_msm_g1_batch and kzg_witness_coeff_many -------------------------------------------
// Item b runs on lane b % nl; every bucket-accumulation kernel goes to one of the dedicated FIFO streams (the plan:
// plan_pipeline in runtime.hip).
struct BatchPipe {
    int nl = 1, nas = 0;
    uint8_t *d_out = nullptr;
    bool out_dev = false;
};

static int batch_begin(kzg_ctx *ctx, size_t batch, size_t out_bytes, void *out, int flags, BatchPipe *bp) {
    bp->out_dev = (flags & KZG_OUT_DEVICE) != 0;
    if (bp->out_dev) {
        bp->d_out = (uint8_t *)out;
    } else {
        // grow-only device staging for the results: a hipMalloc / hipFree pair per call costs a device-wide sync
        if (ctx->batch_out_bytes < out_bytes + 256) {
            if (ctx->batch_out) hipFree(ctx->batch_out);
            ctx->batch_out = nullptr;
            ctx->batch_out_bytes = 0;
            KZG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->batch_out, out_bytes + 256));
            ctx->batch_out_bytes = out_bytes + 256;
        }
        bp->d_out = (uint8_t *)ctx->batch_out;
    }
    KZG_TRY(plan_pipeline(ctx, (int)std::min<size_t>(batch, (size_t)ctx->opt_streams), &bp->nl, &bp->nas));
    // at least two MSMs per lane: the lanes never run dry, so the tail is organised for lane-time instead of depth
    for (int l = 0; l < bp->nl; l++) set_lane_mode(ctx, l, bp->nl > 1, batch >= 2 * (size_t)bp->nl);
    return KZG_OK;
}

static int batch_msm(kzg_ctx *ctx, const BatchPipe &bp, size_t b, int lane, const kzg_srs *srs, size_t offset, const void *d_sc,
                     size_t n, int sfmt, MsmPoint **res, MsmPending *defer = nullptr) {
    // (Staggering the first round -- lane b starting its sort when lane b - 2 has sorted, so that the first accumulation kernel
    // does not wait for sixteen contending sorts -- measured 460 against 472 commitments/s same-box, profiles/r03_ab_kernel.txt:
    // the up-front burst of sorts is the better start.)
    if (bp.nas) {
        // a lane's two MSMs in flight (deferred tails) use different events
        const int ev = defer ? lane + (int)((b / (size_t)bp.nl) & 1) * bp.nl : lane;
        return msm_run(ctx, lane, srs, offset, d_sc, n, sfmt, res, ctx->accum_streams[b % (size_t)accum_streams_for(ctx, bp.nas, srs, n)],
                       ctx->sorted_events[ev], ctx->accum_events[ev], defer);
    }
    return msm_run(ctx, lane, srs, offset, d_sc, n, sfmt, res);
}

static int batch_end(kzg_ctx *ctx, const BatchPipe &bp, int rc, void *out, size_t out_bytes) {
    for (int l = 0; l < bp.nl; l++) hipStreamSynchronize(ctx->lanes[l].stream);
    for (int l = 0; l < bp.nl; l++) set_lane_mode(ctx, l, false, false);
    if (rc == KZG_OK && !bp.out_dev) {
        hipError_t e = hipMemcpy(out, bp.d_out, out_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, hipGetErrorString(e));
    }
#if !defined(KZG_TIMING_NO_PICKUP)
    if (rc == KZG_OK) {  // the lanes' last sort plans (common.h heavy_last)
        uint32_t hv[KZG_MAX_LANES];
        if (hipMemcpy(hv, ctx->d_lane_heavy, sizeof hv, hipMemcpyDeviceToHost) == hipSuccess)
            for (int l = 0; l < bp.nl; l++) {
                Lane &ln = ctx->lanes[l];
                if (ln.heavy_seq == ln.heavy_seen) continue;
                ln.heavy_seen = ln.heavy_seq;
                if (hv[l] == ln.heavy_seq) ctx->heavy_last.store(ctx->msm_count.load(std::memory_order_relaxed), std::memory_order_relaxed);
            }
    }
#endif
    if (ctx->prof) prof_collect(ctx);
    return rc;
}

// ---- the grouped shape of the batched pipeline (four streams whatever the process' hardware-queue pool: plan_pipeline) ----
// A lane is a stream and a stream is in order, so 3 lanes hold 3 MSMs in their latency-bound sort and tail kernels -- too few to
// keep the accumulation queue fed.  Here the MSMs travel in groups of G (option group_msms): every sort kernel and every tail
// kernel is launched ONCE per group (grid.y = the MSM's slot, msm.hip / msm_wide.hip / msm_tail.hip k_*_g), k_accum_affine stays
// one launch per MSM, and four streams carry the whole pipeline:
//     sort stream:  sort(g)  ->  ev sorted     two accumulation FIFO streams (MSMs alternate):  accum(g, i)  ->  ev accumulated
//     tail stream:  tail(g) + results  ->  ev done;     sort(g + 2) waits for it: group g + 2 re-uses group g's half of the arena.
// Two groups are in flight.  Ordering is by events only.  Oversized sort bins: a group is sorted with one block per bin (never in
// slices); a slot that meets one says so in its word of d_lane_heavy, the pick-up at the end of the call notes it in heavy_last, and
// the following calls keep the per-lane path, slices included, for as long as that note holds (common.h, KZG_HEAVY_WINDOW).
static bool batch_wants_group(kzg_ctx *ctx, const kzg_srs *srs, size_t n, size_t batch) {
    if (ctx->plan_group <= 0 || batch < 2 || !msm_group_covers(ctx, srs, n)) return false;
    // (2^17 points with three or more accumulation streams planned are small MSMs, common.h msm_small: as lanes they take a 160-block
    // accumulation grid on four streams.  Grouped, with the batch grid on two, they measured 3043 against 2801 commitments/s on 24
    // queues, profiles/grouped_pipeline_ab.txt (h): no exception for them.)
    if (ctx->opt_heavy_bins == 1) return false;
    const uint64_t now = ctx->msm_count.load(std::memory_order_relaxed) + 1, last = ctx->heavy_last.load(std::memory_order_relaxed);
    return !(ctx->opt_heavy_bins == 0 && last != 0 && now - last <= (uint64_t)KZG_HEAVY_WINDOW);
}

static int msm_batch_grouped(kzg_ctx *ctx, const BatchPipe &bp, const kzg_srs *srs, size_t offset, const void *scalars, size_t n,
                             size_t batch, size_t stride_bytes, int sfmt, int flags, size_t psz, int ofmt) {
    const size_t G = (size_t)ctx->plan_group, ngroups = (batch + G - 1) / G;
    const size_t ws = align_up(msm_workspace_bytes(srs, n), 256);
    const size_t per = align_up(ws + stage_bytes(n * 32, flags) + 8192, 4096);
    const size_t D = KZG_GROUP_DEPTH, nslots = std::min(batch, D * G);  // groups in flight = parts of the group arena
    hipStream_t s_sort = ctx->lanes[0].stream, s_tail = ctx->lanes[1].stream;
    hipStream_t s_acc[2] = {ctx->accum_streams[0], bp.nas >= 2 ? ctx->accum_streams[1] : ctx->lanes[2].stream};
    while (ctx->group_events.size() < 4 * D) {
        hipEvent_t e = nullptr;
        KZG_HIP_CHECK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->group_events.push_back(e);
    }
    // per arena half h: [4 h] sorted, [4 h + 1 + a] accumulated on FIFO stream a, [4 h + 3] tail done
    hipEvent_t *ev = ctx->group_events.data();
    if (ctx->group_tab_count < batch) {
        if (ctx->group_tab) hipFree(ctx->group_tab);
        ctx->group_tab = nullptr;
        ctx->group_tab_count = 0;
        KZG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->group_tab, batch * sizeof(GroupSlot)));
        ctx->group_tab_count = batch;
    }
    KZG_TRY(lane_reserve(ctx, 0, nslots * per + 4096));
    ctx->lanes[0].arena_limit = 0;
    char *arena = (char *)lane_alloc(ctx, 0, nslots * per);
    if (!arena) return fail(ctx, KZG_ERR_ALLOC, "group arena not reserved");
    // the slots' table: MSM b is slot b % G of group b / G, in arena half (b / G) % D
    std::vector<GroupSlot> tab(batch);
    for (size_t b = 0; b < batch; b++) {
        const size_t slot = ((b / G) % D) * G + b % G;
        GroupSlot &t = tab[b];
        t.base = arena + slot * per;
        t.scalars = (flags & KZG_IN_DEVICE) ? (const void *)((const uint8_t *)scalars + b * stride_bytes) : (const void *)(t.base + ws);
        t.out = bp.d_out + b * psz;
        t.heavy = ctx->d_lane_heavy + KZG_MAX_LANES + slot;
    }
    KZG_HIP_CHECK(ctx, hipMemcpy(ctx->group_tab, tab.data(), batch * sizeof(GroupSlot), hipMemcpyHostToDevice));  // (nothing of the call is in flight yet)
    const uint32_t seq = ++ctx->group_heavy_seq;
    ctx->msm_count.fetch_add(batch, std::memory_order_relaxed);
    auto enqueue = [&]() -> int {
    for (size_t g = 0; g < ngroups; g++) {
        const size_t b0 = g * G, cnt = std::min(G, batch - b0), h = g % D;
        const GroupSlot *d_tab = ctx->group_tab + b0;
        if (g >= D) KZG_HIP_CHECK(ctx, hipStreamWaitEvent(s_sort, ev[4 * h + 3], 0));  // the half's previous group has left it
        if (!(flags & KZG_IN_DEVICE))
            for (size_t i = 0; i < cnt; i++)
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(tab[b0 + i].base + ws, (const uint8_t *)scalars + (b0 + i) * stride_bytes, n * 32,
                                                  hipMemcpyHostToDevice, s_sort));
        KZG_TRY(msm_group_sort(ctx, s_sort, srs, offset, n, sfmt, d_tab, (int)cnt, seq));
        KZG_HIP_CHECK(ctx, hipEventRecord(ev[4 * h], s_sort));
        const int na = cnt > 1 ? 2 : 1;
        for (int a = 0; a < na; a++) KZG_HIP_CHECK(ctx, hipStreamWaitEvent(s_acc[a], ev[4 * h], 0));
        for (size_t i = 0; i < cnt; i++) KZG_TRY(msm_group_accum(ctx, s_acc[i & 1], srs, n, tab[b0 + i].base));
        for (int a = 0; a < na; a++) {
            KZG_HIP_CHECK(ctx, hipEventRecord(ev[4 * h + 1 + a], s_acc[a]));
            KZG_HIP_CHECK(ctx, hipStreamWaitEvent(s_tail, ev[4 * h + 1 + a], 0));
        }
        KZG_TRY(msm_group_tail(ctx, s_tail, srs, n, d_tab, (int)cnt, ofmt));
        KZG_HIP_CHECK(ctx, hipEventRecord(ev[4 * h + 3], s_tail));
    }
    return KZG_OK;
    };
    const int rc = enqueue();
    if (rc != KZG_OK) {  // nothing of a failed call stays queued: batch_end waits for the lanes' streams only
        for (hipStream_t st : {s_sort, s_acc[0], s_acc[1], s_tail}) hipStreamSynchronize(st);
        return rc;
    }
#if !defined(KZG_TIMING_NO_PICKUP)
    // the slots' last sorts (common.h heavy_last), as batch_end does for the lanes'.  The tail stream has waited for everything else.
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(s_tail));
    uint32_t hv[KZG_GROUP_DEPTH * KZG_MAX_GROUP];
    KZG_HIP_CHECK(ctx, hipMemcpy(hv, ctx->d_lane_heavy + KZG_MAX_LANES, sizeof hv, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nslots; k++)
        if (hv[k] == seq) ctx->heavy_last.store(ctx->msm_count.load(std::memory_order_relaxed), std::memory_order_relaxed);
#endif
    return KZG_OK;
}

namespace kzg {
// kzg_msm_g1_batch with an explicit distance between consecutive scalar vectors (the sharded commit hands every device the
// slice [lo, hi) of each polynomial: stride = whole-polynomial bytes, n = hi - lo)
int msm_batch_strided(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n, size_t batch,
                      size_t stride_bytes, int sfmt, int flags, void *out, int ofmt, bool may_group) {
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (n > srs->n || offset > srs->n - n) return fail(ctx, KZG_ERR_SHAPE, "MSM range exceeds the SRS");
    if (batch == 0) return KZG_OK;
    BatchPipe bp;
    KZG_TRY(batch_begin(ctx, batch, batch * psz, out, flags, &bp));
    if (may_group && batch_wants_group(ctx, srs, n, batch))
        return batch_end(ctx, bp, msm_batch_grouped(ctx, bp, srs, offset, scalars, n, batch, stride_bytes, sfmt, flags, psz, ofmt), out, batch * psz);
    size_t per = align_up(msm_workspace_bytes(srs, n) + stage_bytes(n * 32, flags) + 8192, 4096);
    int rc = KZG_OK;
    // Software pipelining inside a lane (deep batches on FIFO accumulation streams): MSM b's tail is enqueued AFTER the sort of the
    // lane's next MSM (b + nl), so the accumulation queue gets its next kernel before the lane spends milliseconds in latency-bound
    // tail kernels.  Two MSMs of a lane are in flight then: two workspaces (the arena's halves) and two event pairs per lane.
    const bool defer = bp.nas > 0 && batch > (size_t)bp.nl && !ctx->opt_no_defer_tail;
    std::vector<MsmPending> pend(defer ? 2 * (size_t)bp.nl : 0);
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, defer ? 2 * per : per);
    auto finish = [&](size_t b) {
        const int l = (int)(b % bp.nl);
        MsmPoint *res = nullptr;
        int r = msm_finish(ctx, pend[(size_t)l + ((b / (size_t)bp.nl) & 1) * (size_t)bp.nl], &res);
        if (r == KZG_OK) r = emit_point(ctx, l, res, bp.d_out + b * psz, ofmt);
        return r;
    };
    for (size_t b = 0; b < batch && rc == KZG_OK; b++) {
        int l = (int)(b % bp.nl);
        const size_t half = defer ? ((b / (size_t)bp.nl) & 1) : 0;
        ctx->lanes[l].arena_used = half * per;  // stream order makes re-use of the lane arena (of this half) safe
        ctx->lanes[l].arena_limit = defer ? (half + 1) * per : 0;  // an under-estimated workspace fails (KZG_ERR_ALLOC) instead of running
                                                                   // into the other half, which belongs to the lane's other MSM in flight
        const void *d_sc = nullptr;
        rc = stage_in(ctx, l, (const uint8_t *)scalars + b * stride_bytes, n * 32, flags, &d_sc);
        MsmPoint *res = nullptr;
        if (defer) {
            MsmPending &pd = pend[(size_t)l + half * (size_t)bp.nl];
            if (rc == KZG_OK) rc = batch_msm(ctx, bp, b, l, srs, offset, d_sc, n, sfmt, &res, &pd);
            if (rc == KZG_OK && !pd.active) pd.result = res;  // (not deferred: multi-pass / wide path) finish() emits it
            if (rc == KZG_OK && b >= (size_t)bp.nl) rc = finish(b - bp.nl);
            continue;
        }
        if (rc == KZG_OK) rc = batch_msm(ctx, bp, b, l, srs, offset, d_sc, n, sfmt, &res);
        if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + b * psz, ofmt);
    }
    if (defer)
        for (size_t b = batch > (size_t)bp.nl ? batch - bp.nl : 0; b < batch && rc == KZG_OK; b++) rc = finish(b);
    for (int l = 0; l < bp.nl; l++) ctx->lanes[l].arena_limit = 0;
    return batch_end(ctx, bp, rc, out, batch * psz);
}
}  // namespace kzg

extern "C" int kzg_msm_g1_batch(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n,
                                size_t batch, int sfmt, int flags, void *out, int ofmt) {
    if (!ctx || !srs || !out || (!scalars && n && batch)) return KZG_ERR_SHAPE;
    if (n > SIZE_MAX / 32) return KZG_ERR_SHAPE;
    return msm_batch_strided(ctx, srs, offset, scalars, n, batch, n * 32, sfmt, flags, out, ofmt, true);
}

extern "C" int kzg_witness_coeff_many(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, const void *xs,
                                      const void *ys, size_t count, int sfmt, int flags, void *out, int ofmt, int *status) {
    // `count` calls of KZGProver::create_witness (src/coeff_form.rs:66-81) on ONE polynomial, pipelined: opening j computes its
    // quotient (Horner scan) and its MSM on lane j % streams.  status[j] = 0 or KZG_ERR_POINT_NOT_ON_POLY (p(x_j) != y_j).
    if (!ctx || !srs || !coeffs || !out || n == 0 || ((!xs || !ys) && count)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (n - 1 > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (count == 0) return KZG_OK;
    std::vector<Fr> xm(count);
    for (size_t j = 0; j < count; j++) KZG_TRY(host_scalar(ctx, (const uint8_t *)xs + 32 * j, sfmt, &xm[j]));
    for (size_t j = 0; j < count; j++) {  // the ys are only compared with p(x_j) below; host scalars all the same: < r
        Fr ym;
        KZG_TRY(host_scalar(ctx, (const uint8_t *)ys + 32 * j, sfmt, &ym));
    }
    BatchPipe bp;
    KZG_TRY(batch_begin(ctx, count, count * psz, out, flags, &bp));
    int rc = KZG_OK;
    // shared inputs / outputs live in the arena of one extra lane: the coefficients (when they come from the host) and p(x_j)
    const int sl = bp.nl;
    rc = ensure_lanes(ctx, sl + 1);
    if (rc == KZG_OK) rc = lane_reserve(ctx, sl, stage_bytes(n * 32, flags) + count * 32 + 4096);
    const void *d_coeffs = nullptr;
    Fr *d_px = nullptr;
    if (rc == KZG_OK) rc = stage_in(ctx, sl, coeffs, n * 32, flags, &d_coeffs);
    if (rc == KZG_OK && !(d_px = (Fr *)lane_alloc(ctx, sl, count * 32))) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
    if (rc == KZG_OK && hipStreamSynchronize(ctx->lanes[sl].stream) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "stage-in of the coefficients");
    size_t per = msm_workspace_bytes(srs, n - 1) + n * 32 + (n / 2048 + 4) * 64 + 65536;
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, per);
    for (size_t j = 0; j < count && rc == KZG_OK; j++) {
        int l = (int)(j % bp.nl);
        ctx->lanes[l].arena_used = 0;
        Fr *dq = (Fr *)lane_alloc(ctx, l, n * 32);
        if (!dq) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
        if (rc == KZG_OK) rc = quotient_linear_run(ctx, l, (const Fr *)d_coeffs, n, xm[j], dq, d_px + j);
        MsmPoint *res = nullptr;
        if (rc == KZG_OK) rc = batch_msm(ctx, bp, j, l, srs, 0, dq, n - 1, sfmt, &res);
        if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + j * psz, ofmt);
    }
    rc = batch_end(ctx, bp, rc, out, count * psz);
    if (rc != KZG_OK) return rc;
    std::vector<uint8_t> px(count * 32);
    KZG_HIP_CHECK(ctx, hipMemcpy(px.data(), d_px, count * 32, hipMemcpyDeviceToHost));
    int worst = KZG_OK;
    for (size_t j = 0; j < count; j++) {
        // remainder of (p - y)/(X - x) is p(x) - y: Some(_) => Err(PointNotOnPolynomial)
        int sj = memcmp(px.data() + 32 * j, (const uint8_t *)ys + 32 * j, 32) != 0 ? KZG_ERR_POINT_NOT_ON_POLY : KZG_OK;
        if (status) status[j] = sj;
        if (sj) worst = sj;
    }
    if (worst && !status) return fail(ctx, KZG_ERR_POINT_NOT_ON_POLY, "point not on polynomial!");
    return KZG_OK;
}

extern "C" int kzg_witness_eval_many(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, const size_t *indices,
                                     size_t count, int sfmt, int flags, void *out, int ofmt) {
    // `count` calls of KZGProverEvalForm::create_witness (src/eval_form.rs:124-140) on ONE evaluation vector, pipelined
    if (!ctx || !lagrange || !evals || !out || (!indices && count)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    for (size_t j = 0; j < count; j++)
        if (indices[j] >= d) return fail(ctx, KZG_ERR_SHAPE, "evaluation index out of range (reference: index panic)");
    if (d > lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "evaluations longer than the Lagrange SRS (reference: slice panic)");
    uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    if (count == 0) return KZG_OK;
    BatchPipe bp;
    KZG_TRY(batch_begin(ctx, count, count * psz, out, flags, &bp));
    const int sl = bp.nl;  // shared arena: the evaluations when they come from the host
    int rc = ensure_lanes(ctx, sl + 1);
    if (rc == KZG_OK) rc = lane_reserve(ctx, sl, stage_bytes(d * 32, flags) + 4096);
    const void *de = nullptr;
    if (rc == KZG_OK) rc = stage_in(ctx, sl, evals, d * 32, flags, &de);
    if (rc == KZG_OK) rc = eval_tables_ready(ctx, sl, log_d);  // also waits for the stage-in
    size_t per = msm_workspace_bytes(lagrange, d) + d * 32 + (d / 256 + 4) * 32 + 65536;
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, per);
    for (size_t j = 0; j < count && rc == KZG_OK; j++) {
        int l = (int)(j % bp.nl);
        ctx->lanes[l].arena_used = 0;
        Fr *dq = (Fr *)lane_alloc(ctx, l, d * 32);
        if (!dq) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
        if (rc == KZG_OK) rc = quotient_eval_run(ctx, l, (const Fr *)de, log_d, indices[j], sfmt, dq);
        MsmPoint *res = nullptr;
        if (rc == KZG_OK) rc = batch_msm(ctx, bp, j, l, lagrange, 0, dq, d, sfmt, &res);
        if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + j * psz, ofmt);
    }
    return batch_end(ctx, bp, rc, out, count * psz);
}

extern "C" int kzg_g1_sum(kzg_ctx *ctx, const void *points, size_t count, int pfmt, int flags, void *out, int ofmt) {
    if (!ctx || !out || (!points && count)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    size_t psz = point_format_bytes(pfmt);
    if (!psz || !point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 point format");
    size_t cnt = count ? count : 1;
    size_t need = stage_bytes(cnt * psz, flags) + cnt * sizeof(G1Xyzz) + (cnt + 2 * sum_points_scratch_count(cnt) + 4) * sizeof(MsmPoint) + 8192;
    KZG_TRY(lane_reserve(ctx, 0, need));
    hipStream_t st = ctx->lanes[0].stream;
    G1Xyzz *dec = (G1Xyzz *)lane_alloc(ctx, 0, cnt * sizeof(G1Xyzz));
    MsmPoint *pts = (MsmPoint *)lane_alloc(ctx, 0, cnt * sizeof(MsmPoint));
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, 0, 2 * sum_points_scratch_count(cnt) * sizeof(MsmPoint));
    int *bad = (int *)lane_alloc(ctx, 0, 256);
    if (!dec || !pts || !scratch || !bad) return fail(ctx, KZG_ERR_ALLOC, "sum workspace not reserved");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    MsmPoint *res = pts;
    if (count == 0) {
        KZG_TRY(point_set_infinity(ctx, st, pts));
    } else {
        const void *d_raw = nullptr;
        KZG_TRY(stage_in(ctx, 0, points, count * psz, flags, &d_raw));
        KZG_TRY(decode_points(ctx, st, d_raw, count, pfmt, dec, bad, POINTS_ON_CURVE));
        KZG_TRY(points_to30(ctx, st, dec, pts, count));
        KZG_TRY(sum_points_run(ctx, 0, pts, count, scratch, &res));
    }
    int hbad = 0;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    KZG_TRY(finish_point(ctx, 0, res, out, ofmt, flags));
    if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, "a G1 point failed to decode or is not on the curve");
    return KZG_OK;
}

namespace kzg {
int g1_sum_batch_strided(kzg_ctx *ctx, const void *points, size_t count, size_t groups, size_t gstride, size_t istride, int pfmt,
                         int flags, void *out, int ofmt, int level) {
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    size_t psz = point_format_bytes(pfmt), osz = point_format_bytes(ofmt);
    if (!psz || !osz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 point format");
    if (count > (1u << 20) || groups > (1u << 24)) return fail(ctx, KZG_ERR_SHAPE, "kzg_g1_sum_batch: count <= 2^20, groups <= 2^24");
    // every source slot the strides reach: count * groups of them for dense groups, more when the records carry other slots
    // between the points -- the gathered [world][batch + 1] records of a device group (mgpu.hip) hold a status slot after each
    // rank's batch partials, so rank r's partial of polynomial b sits at r (batch + 1) + b
    size_t total = count && groups ? (groups - 1) * gstride + (count - 1) * istride + 1 : 0;
    KZG_TRY(lane_reserve(ctx, 0, stage_bytes(total * psz, flags) + total * sizeof(G1Xyzz) + (total + groups + 4) * sizeof(MsmPoint) + groups * 144 + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    G1Xyzz *dec = (G1Xyzz *)lane_alloc(ctx, 0, total * sizeof(G1Xyzz));
    MsmPoint *pts = (MsmPoint *)lane_alloc(ctx, 0, total * sizeof(MsmPoint));
    MsmPoint *tmp = (MsmPoint *)lane_alloc(ctx, 0, groups * sizeof(MsmPoint));
    int *bad = (int *)lane_alloc(ctx, 0, 256);
    void *d_out = (flags & KZG_OUT_DEVICE) ? out : lane_alloc(ctx, 0, groups * osz);
    if (!dec || !pts || !tmp || !bad || !d_out) return fail(ctx, KZG_ERR_ALLOC, "sum workspace not reserved");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    const void *d_raw = nullptr;
    KZG_TRY(stage_in(ctx, 0, points, total * psz, flags, &d_raw));
    KZG_TRY(decode_points(ctx, st, d_raw, total, pfmt, dec, bad, level));
    KZG_TRY(points_to30(ctx, st, dec, pts, total));
    // up to four host-bound sums (the combine step of a sharded commit has one): converted on the calling thread, as in finish_point
    const bool on_host = !(flags & KZG_OUT_DEVICE) && ctx->opt_host_affine && groups <= 4;
    KZG_TRY(sum_groups_emit(ctx, 0, pts, count, groups, gstride, istride, tmp, on_host ? nullptr : d_out, ofmt));
    int hbad = 0;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    MsmPoint hsum[4];
    if (on_host) KZG_HIP_CHECK(ctx, hipMemcpyAsync(hsum, tmp, groups * sizeof(MsmPoint), hipMemcpyDeviceToHost, st));
    else if (!(flags & KZG_OUT_DEVICE)) KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, groups * osz, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (on_host)
        for (size_t gi = 0; gi < groups; gi++) {
            alignas(16) uint8_t buf[144];
            emit_one(hsum[gi], buf, ofmt);
            memcpy((uint8_t *)out + gi * osz, buf, osz);
        }
    if (ctx->prof) prof_collect(ctx);
    if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, "a G1 point failed to decode or is not on the curve");
    return KZG_OK;
}
}  // namespace kzg

extern "C" int kzg_g1_sum_batch(kzg_ctx *ctx, const void *points, size_t count, size_t groups, int pfmt, int flags,
                                void *out, int ofmt) {
    if (!ctx || !out || !points || count == 0 || groups == 0) return KZG_ERR_SHAPE;
    return g1_sum_batch_strided(ctx, points, count, groups, count, 1, pfmt, flags, out, ofmt);
}

// ---------------------------------------------------------------------------------------------
// NTT
// ---------------------------------------------------------------------------------------------
extern "C" int kzg_compute_omega(size_t d, size_t *m_out, uint32_t *exp_out, void *omega, int sfmt) {
    // EvaluationDomain::compute_omega (src/ft.rs:55-76)
    size_t m = 1;
    uint32_t exp = 0;
    while (m < d) {
        m *= 2;
        exp += 1;
        if (exp >= FR_TWO_ADICITY) return KZG_ERR_DEGREE_TOO_LARGE;
    }
    if (m_out) *m_out = m;
    if (exp_out) *exp_out = exp;
    if (omega) scalar_out(host_omega(exp), sfmt, omega);
    return KZG_OK;
}

extern "C" int kzg_ntt_fr(kzg_ctx *ctx, void *data, uint32_t log_n, int inverse, int flags) {
    if (!ctx || !data) return KZG_ERR_SHAPE;
    Lease ls;  // EvaluationDomain::fft is a `&mut self` method of the caller's own vector: many threads, one context
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (log_n >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "polynomial degree too large");
    if (log_n > 28) return fail(ctx, KZG_ERR_SHAPE, "NTT sizes above 2^28 are not supported (2^24-point two-pass transforms under one 16-point outer level)");
    size_t n = (size_t)1 << log_n;
    // above 2^24: the transposed copy of the whole vector + the inner transform's 2^24-element scratch + the outer twiddle tables
    KZG_TRY(lane_reserve(ctx, lane, ntt_workspace_bytes(log_n) + stage_bytes(n * 32, flags) + 8192));
    hipStream_t st = ctx->lanes[lane].stream;
    const void *d = nullptr;
    KZG_TRY(stage_in(ctx, lane, data, n * 32, flags, &d));
    KZG_TRY(ntt_run(ctx, lane, (Fr *)d, log_n, inverse));
    if (!(flags & KZG_IN_DEVICE)) KZG_HIP_CHECK(ctx, hipMemcpyAsync(data, d, n * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

// kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch.  Device data is transformed where it lies.  Host data goes through the lane in pieces of
// max(1, 2^21 / n) vectors (64 MiB, or one vector above that), packed back to back on the device: the words between the caller's
// vectors never leave the host.
static int ntt_batch_entry(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int flags, bool coset) {
    if (!ctx || !data) return KZG_ERR_SHAPE;
    if (log_n >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "polynomial degree too large");
    if (log_n > 28) return fail(ctx, KZG_ERR_SHAPE, "NTT sizes above 2^28 are not supported (as kzg_ntt_fr)");
    const size_t n = (size_t)1 << log_n;
    if (stride && stride < n) return fail(ctx, KZG_ERR_SHAPE, "batched NTT: stride must be 0 (contiguous) or at least 2^log_n elements");
    if (!stride) stride = n;
    if (batch == 0) return KZG_OK;
    size_t span, span_bytes;
    if (__builtin_mul_overflow(batch - 1, stride, &span) || __builtin_add_overflow(span, n, &span) || __builtin_mul_overflow(span, (size_t)32, &span_bytes))
        return fail(ctx, KZG_ERR_SHAPE, "batched NTT: (batch - 1) * stride + 2^log_n elements do not fit the address space");
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const bool on_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t piece = on_dev ? batch : std::min(batch, log_n >= 21 ? (size_t)1 : (size_t)1 << (21 - log_n));
    KZG_TRY(lane_reserve(ctx, lane, (on_dev ? 0 : align_up(piece * n * 32 + 256, 256)) + ntt_batch_workspace_bytes(ctx, log_n, piece) + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    const Fr g7 = from_u64<FrParams>(FR_MULT_GENERATOR);
    Fr *stage = on_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, piece * n * 32);
    if (!on_dev && !stage) return fail(ctx, KZG_ERR_ALLOC, "input staging not reserved");
    const size_t mark = ctx->lanes[lane].arena_used;
    for (size_t b0 = 0; b0 < batch; b0 += piece) {
        const size_t cnt = std::min(piece, batch - b0);
        Fr *d = on_dev ? (Fr *)data : stage;
        uint8_t *host = (uint8_t *)data + b0 * stride * 32;
        if (!on_dev) KZG_HIP_CHECK(ctx, hipMemcpy2DAsync(d, n * 32, host, stride * 32, n * 32, cnt, hipMemcpyHostToDevice, st));
        ctx->lanes[lane].arena_used = mark;
        if (coset) KZG_TRY(coset_ntt_batch_run(ctx, lane, d, log_n, cnt, on_dev ? stride : n, inverse, g7));
        else KZG_TRY(ntt_batch_run(ctx, lane, d, log_n, cnt, on_dev ? stride : n, inverse));
        if (!on_dev) KZG_HIP_CHECK(ctx, hipMemcpy2DAsync(host, stride * 32, d, n * 32, n * 32, cnt, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int flags) {
    return ntt_batch_entry(ctx, data, log_n, batch, stride, inverse, flags, false);
}

extern "C" int kzg_coset_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int sfmt, int flags) {
    (void)sfmt;  // linear map with Montgomery constants: the data's form is preserved (as kzg_coset_ntt_fr)
    return ntt_batch_entry(ctx, data, log_n, batch, stride, inverse, flags, true);
}

// ---------------------------------------------------------------------------------------------
// Fr polynomial helpers
// ---------------------------------------------------------------------------------------------
extern "C" int kzg_poly_eval(kzg_ctx *ctx, const void *coeffs, size_t n, const void *x, int sfmt, int flags, void *y_out) {
    if (!ctx || !coeffs || !x || !y_out || n == 0 || !count_ok(n)) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    Fr xm;
    KZG_TRY(host_scalar(ctx, x, sfmt, &xm));
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(n * 32, flags) + (n / 2048 + 4) * 64 + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    const void *d = nullptr;
    KZG_TRY(stage_in(ctx, lane, coeffs, n * 32, flags, &d));
    Fr *dy = (Fr *)lane_alloc(ctx, lane, 256);
    if (!dy) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_TRY(poly_eval_run(ctx, lane, (const Fr *)d, n, xm, dy));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(y_out, dy, 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_quotient_linear(kzg_ctx *ctx, const void *coeffs, size_t n, const void *x, const void *y, int sfmt,
                                   int flags, void *q_out) {
    if (!ctx || !coeffs || !x || !y || n == 0 || (!q_out && n > 1) || !count_ok(n)) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    Fr xm, ym;
    KZG_TRY(host_scalar(ctx, x, sfmt, &xm));
    KZG_TRY(host_scalar(ctx, y, sfmt, &ym));  // only compared with p(x) below; a host scalar all the same: < r, before q_out is written
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(n * 32, flags) * 2 + (n / 2048 + 4) * 64 + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    const void *d = nullptr;
    KZG_TRY(stage_in(ctx, lane, coeffs, n * 32, flags, &d));
    bool out_dev = (flags & KZG_OUT_DEVICE) != 0;
    Fr *dq = out_dev ? (Fr *)q_out : (Fr *)lane_alloc(ctx, lane, n * 32);
    Fr *dpx = (Fr *)lane_alloc(ctx, lane, 256);
    if (!dq || !dpx) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_TRY(quotient_linear_run(ctx, lane, (const Fr *)d, n, xm, dq, dpx));
    Fr px;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(px.v, dpx, 32, hipMemcpyDeviceToHost, st));
    if (!out_dev && n > 1) KZG_HIP_CHECK(ctx, hipMemcpyAsync(q_out, dq, (n - 1) * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    if (memcmp(px.v, y, 32) != 0) return fail(ctx, KZG_ERR_POINT_NOT_ON_POLY, "point not on polynomial!");
    return KZG_OK;
}

extern "C" int kzg_quotient_eval(kzg_ctx *ctx, const void *evals, size_t d, size_t i, int sfmt, int flags, void *q_out) {
    if (!ctx || !evals || !q_out) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    if (i >= d) return fail(ctx, KZG_ERR_SHAPE, "evaluation index out of range (reference: index panic)");
    uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(d * 32, flags) * 2 + (d / 256 + 4) * 32 + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    const void *de = nullptr;
    KZG_TRY(stage_in(ctx, lane, evals, d * 32, flags, &de));
    bool out_dev = (flags & KZG_OUT_DEVICE) != 0;
    Fr *dq = out_dev ? (Fr *)q_out : (Fr *)lane_alloc(ctx, lane, d * 32);
    if (!dq) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_TRY(quotient_eval_run(ctx, lane, (const Fr *)de, log_d, i, sfmt, dq));
    if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(q_out, dq, d * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

// ---------------------------------------------------------------------------------------------
// evaluation form at any point of Fr (open_eval.hip): y = p(z), the quotient's values on the domain, the witness
// ---------------------------------------------------------------------------------------------
// what the three entry points check alike, before memory is touched: the domain, the scalar format, and every z (host scalars: < r)
static int open_args(kzg_ctx *ctx, size_t d, size_t batch, const void *zs, int sfmt, uint32_t *log_d, std::vector<OpenPoint> *pts) {
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    *log_d = (uint32_t)ilog2_ceil(d);
    if (*log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    if (batch > SIZE_MAX / (d * 32)) return fail(ctx, KZG_ERR_SHAPE, "batch too large");
    try {  // (no exception may leave through the C ABI)
        pts->resize(batch);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the opening points");
    }
    for (size_t b = 0; b < batch; b++) {
        Fr zm;
        KZG_TRY(host_scalar(ctx, (const uint8_t *)zs + 32 * b, sfmt, &zm));
        if (open_point_classify(*log_d, zm, &(*pts)[b]) != KZG_OK) return fail(ctx, KZG_ERR_INTERNAL, "z^d == 1 but z is no power of omega");
    }
    return KZG_OK;
}

// the Fr stage alone on one lane: ys_out (optional, host) and, for ONE polynomial, its quotient at q_out (optional; host or device)
static int open_fr_only(kzg_ctx *ctx, int lane, const void *evals, uint32_t log_d, size_t batch, const OpenPoint *pts, int sfmt, int flags,
                        void *ys_out, void *q_out) {
    const size_t d = (size_t)1 << log_d;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>({(size_t)OE_MAX_CHUNK, batch, ((size_t)1 << 22) / d}));
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, q_dev = q_out && (flags & KZG_OUT_DEVICE);
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(chunk * d * 32, flags) + align_up(batch * 32, 256) + ((q_out && !q_dev) ? align_up(d * 32, 256) : 0) +
                                        open_eval_fr_workspace_bytes(d, chunk) + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, chunk * d * 32);
    Fr *d_y = (Fr *)lane_alloc(ctx, lane, batch * 32);
    Fr *d_q = !q_out ? nullptr : (q_dev ? (Fr *)q_out : (Fr *)lane_alloc(ctx, lane, d * 32));
    if ((!in_dev && !d_in) || !d_y || (q_out && !d_q)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    int rc = KZG_OK;
    for (size_t b0 = 0; b0 < batch && rc == KZG_OK; b0 += chunk) {
        const size_t B = std::min(chunk, batch - b0);
        const Fr *src = (const Fr *)evals + b0 * d;
        if (!in_dev) {
            if (hipMemcpyAsync(d_in, src, B * d * 32, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "stage-in of the evaluations");
            src = d_in;
        }
        if (rc == KZG_OK) rc = open_eval_fr_run(ctx, lane, src, log_d, B, pts + b0, sfmt, d_y + b0, d_q);
    }
    if (rc == KZG_OK && ys_out && hipMemcpyAsync(ys_out, d_y, batch * 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "copy of the values");
    if (rc == KZG_OK && q_out && !q_dev && hipMemcpyAsync(q_out, d_q, d * 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "copy of the quotient");
    if (hipStreamSynchronize(st) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "evaluation-form opening");
    if (ctx->prof) prof_collect(ctx);
    return rc;
}

extern "C" int kzg_eval_form_eval(kzg_ctx *ctx, const void *evals, size_t d, size_t batch, const void *zs, int sfmt, int flags, void *ys_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!evals || !zs || !ys_out) return fail(ctx, KZG_ERR_SHAPE, "kzg_eval_form_eval: NULL evals, zs or ys_out");
    uint32_t log_d = 0;
    std::vector<OpenPoint> pts;
    KZG_TRY(open_args(ctx, d, batch, zs, sfmt, &log_d, &pts));
    if (batch == 0) return KZG_OK;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return open_fr_only(ctx, ls.lane, evals, log_d, batch, pts.data(), sfmt, flags, ys_out, nullptr);
}

extern "C" int kzg_quotient_eval_at(kzg_ctx *ctx, const void *evals, size_t d, const void *z, int sfmt, int flags, void *y_out, void *q_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!evals || !z || !q_out) return fail(ctx, KZG_ERR_SHAPE, "kzg_quotient_eval_at: NULL evals, z or q_out");
    uint32_t log_d = 0;
    std::vector<OpenPoint> pts;
    KZG_TRY(open_args(ctx, d, 1, z, sfmt, &log_d, &pts));
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return open_fr_only(ctx, ls.lane, evals, log_d, 1, pts.data(), sfmt, flags, y_out, q_out);
}

extern "C" int kzg_open_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t batch, const void *zs, int sfmt,
                             int flags, void *ys_out, void *out_w, int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!lagrange || !evals || !zs) return fail(ctx, KZG_ERR_SHAPE, "kzg_open_eval: NULL lagrange, evals or zs");
    if (!ys_out && !out_w) return fail(ctx, KZG_ERR_SHAPE, "kzg_open_eval: no output");
    const size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (d != lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d) (src/eval_form.rs:115)");
    if (lagrange->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the Lagrange SRS is resident on another GPU than this context's");
    uint32_t log_d = 0;
    std::vector<OpenPoint> pts;
    KZG_TRY(open_args(ctx, d, batch, zs, sfmt, &log_d, &pts));
    if (batch == 0) return KZG_OK;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!out_w) return open_fr_only(ctx, 0, evals, log_d, batch, pts.data(), sfmt, flags & ~KZG_OUT_DEVICE, ys_out, nullptr);
    BatchPipe bp;
    KZG_TRY(batch_begin(ctx, batch, batch * psz, out_w, flags, &bp));
    // Chunks of one polynomial per lane.  The Fr stage of a chunk runs on the stream of one extra lane (its arena holds what the
    // chunks share: staged evaluations, the values, two sets of quotients); the MSMs of chunk c read set c & 1 on their lanes while
    // that stream already works on chunk c + 1, and chunk c + 2 waits for them before it overwrites the set.
    const size_t chunk = (size_t)bp.nl;
    const int sl = bp.nl;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t qset = align_up(chunk * d * 32, 256);
    int rc = ensure_lanes(ctx, sl + 1);
    if (rc == KZG_OK) rc = lane_reserve(ctx, sl, stage_bytes(chunk * d * 32, flags) + 2 * qset + align_up(batch * 32, 256) + open_eval_fr_workspace_bytes(d, chunk) + 65536);
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, msm_workspace_bytes(lagrange, d) + 65536);
    hipStream_t fst = rc == KZG_OK ? ctx->lanes[sl].stream : nullptr;
    Fr *d_in = nullptr, *d_y = nullptr, *d_q[2] = {nullptr, nullptr};
    if (rc == KZG_OK) {
        d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, sl, chunk * d * 32);
        d_y = (Fr *)lane_alloc(ctx, sl, batch * 32);
        d_q[0] = (Fr *)lane_alloc(ctx, sl, qset);
        d_q[1] = (Fr *)lane_alloc(ctx, sl, qset);
        if ((!in_dev && !d_in) || !d_y || !d_q[0] || !d_q[1]) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    // events: the Fr stage of a chunk is done (per set); lane l is done with its MSM of a chunk (per set and lane)
    std::vector<hipEvent_t> evs;
    try {
        evs.assign(2 + 2 * chunk, nullptr);
    } catch (const std::bad_alloc &) {
        if (rc == KZG_OK) rc = fail(ctx, KZG_ERR_ALLOC, "host memory");
    }
    for (size_t i = 0; i < evs.size() && rc == KZG_OK; i++)
        if (hipEventCreateWithFlags(&evs[i], hipEventDisableTiming) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventCreate");
    for (size_t b0 = 0, c = 0; b0 < batch && rc == KZG_OK; b0 += chunk, c++) {
        const size_t B = std::min(chunk, batch - b0), p = c & 1;
        hipEvent_t fr_done = evs[p], *lane_done = &evs[2 + p * chunk];
        if (c >= 2)  // (every chunk but the last is full: all lanes recorded in chunk c - 2)
            for (size_t l = 0; l < chunk && rc == KZG_OK; l++)
                if (hipStreamWaitEvent(fst, lane_done[l], 0) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipStreamWaitEvent");
        const Fr *src = (const Fr *)evals + b0 * d;
        if (!in_dev && rc == KZG_OK) {
            if (hipMemcpyAsync(d_in, src, B * d * 32, hipMemcpyHostToDevice, fst) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "stage-in of the evaluations");
            src = d_in;
        }
        if (rc == KZG_OK) rc = open_eval_fr_run(ctx, sl, src, log_d, B, pts.data() + b0, sfmt, d_y + b0, d_q[p]);
        if (rc == KZG_OK && hipEventRecord(fr_done, fst) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventRecord");
        for (size_t b = 0; b < B && rc == KZG_OK; b++) {
            const int l = (int)b;
            hipStream_t st = ctx->lanes[l].stream;
            ctx->lanes[l].arena_used = 0;  // stream order makes re-use of the lane arena safe
            if (hipStreamWaitEvent(st, fr_done, 0) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipStreamWaitEvent");
            MsmPoint *res = nullptr;
            if (rc == KZG_OK) rc = batch_msm(ctx, bp, b0 + b, l, lagrange, 0, d_q[p] + b * d, d, sfmt, &res);
            if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + (b0 + b) * psz, ofmt);
            if (rc == KZG_OK && hipEventRecord(lane_done[l], st) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventRecord");
        }
    }
    if (fst && hipStreamSynchronize(fst) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "evaluation-form opening");
    rc = batch_end(ctx, bp, rc, out_w, batch * psz);
    for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
    if (rc == KZG_OK && ys_out) KZG_HIP_CHECK(ctx, hipMemcpy(ys_out, d_y, batch * 32, hipMemcpyDeviceToHost));
    return rc;
}

// ---------------------------------------------------------------------------------------------
// many polynomials at one point, one folded witness (fold.hip): F = sum_i gamma^i p_i, the witness of F
// ---------------------------------------------------------------------------------------------
constexpr size_t FOLD_STAGE_BYTES = (size_t)64 << 20;  // host vectors of kzg_fr_fold are staged in pieces of at most this (one vector at least)

// what the three calls check alike: t, the sizes, the challenges (host scalars in [1, r)) -> Montgomery
static int fold_args(kzg_ctx *ctx, const char *who, size_t d, size_t t, size_t groups, const void *gammas, int sfmt, std::vector<Fr> *gm) {
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (t == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t == 0");
    if (d == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (!count_ok(d) || !count_ok(t) || !count_ok(groups) || t > (SIZE_MAX >> 6) / d || groups > (SIZE_MAX >> 6) / (t * d))
        return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": groups x t x d too large");
    if (groups && !gammas) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL gammas");
    try {  // (no exception may leave through the C ABI)
        gm->resize(groups);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the challenges");
    }
    for (size_t g = 0; g < groups; g++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)gammas + 32 * g, 32);
        if (!is_canonical(x) || x.is_zero()) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a challenge gamma must be in [1, modulus)");
        (*gm)[g] = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
    }
    return KZG_OK;
}

// the opening points of the folded calls: host scalars below r in either format
static int fold_points_ok(kzg_ctx *ctx, const char *who, const void *zs, size_t groups) {
    for (size_t g = 0; g < groups; g++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)zs + 32 * g, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a point z >= modulus");
    }
    return KZG_OK;
}

// One group's t vectors of d scalars at src (host unless in_dev) folded into d_F on the lane's stream, in pieces of at most P vectors
// from the last one down (the running sum stays at d_F); d_in: P x d scalars of staging (host input).  each(piece, i0, B), if given,
// runs on every piece while it is on the device.
template <typename Each>
static int fold_group(kzg_ctx *ctx, int lane, const Fr *src, size_t d, size_t t, size_t P, bool in_dev, Fr *d_in, const Fr *d_gamma, Fr *d_F,
                      Each each) {
    hipStream_t st = ctx->lanes[lane].stream;
    for (size_t i1 = t; i1 > 0;) {
        const size_t i0 = i1 > P ? i1 - P : 0, B = i1 - i0;
        const Fr *piece = src + i0 * d;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, piece, B * d * 32, hipMemcpyHostToDevice, st));
            piece = d_in;
        }
        KZG_TRY(each(piece, i0, B));
        if (d_F) KZG_TRY(fold_run(ctx, st, piece, d, B, 0, 1, d_gamma, i1 != t, d_F));
        i1 = i0;
    }
    return KZG_OK;
}

extern "C" int kzg_fr_fold(kzg_ctx *ctx, const void *vecs, size_t d, size_t t, size_t groups, const void *gammas, int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    std::vector<Fr> gm;
    KZG_TRY(fold_args(ctx, "kzg_fr_fold", d, t, groups, gammas, sfmt, &gm));
    if (groups == 0) return KZG_OK;
    if (!vecs || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_fr_fold: NULL vecs or out");
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t P = std::max<size_t>(1, std::min(t, FOLD_STAGE_BYTES / (d * 32)));      // vectors per staged piece
    const size_t GC = out_dev ? groups : std::max<size_t>(1, std::min(groups, FOLD_STAGE_BYTES / (d * 32)));  // groups per chunk of host output
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(P * d * 32, flags) + (out_dev ? 0 : align_up(GC * d * 32, 256)) + align_up(groups * 32, 256) + 65536));
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, P * d * 32);
    Fr *d_o = out_dev ? (Fr *)out : (Fr *)lane_alloc(ctx, lane, GC * d * 32);
    Fr *d_gam = (Fr *)lane_alloc(ctx, lane, groups * 32);
    if ((!in_dev && !d_in) || !d_o || !d_gam) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_gam, gm.data(), groups * 32, hipMemcpyHostToDevice, st));
    for (size_t g0 = 0; g0 < groups; g0 += GC) {
        const size_t G = std::min(GC, groups - g0);
        Fr *o = out_dev ? d_o + g0 * d : d_o;
        if (in_dev) {
            KZG_TRY(fold_run(ctx, st, (const Fr *)vecs + g0 * t * d, d, t, t * d, G, d_gam + g0, false, o));
        } else {
            for (size_t g = 0; g < G; g++)
                KZG_TRY(fold_group(ctx, lane, (const Fr *)vecs + (g0 + g) * t * d, d, t, P, false, d_in, d_gam + g0 + g, o + g * d,
                                   [](const Fr *, size_t, size_t) { return (int)KZG_OK; }));
        }
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out + g0 * d * 32, o, G * d * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_open_fold_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t t, size_t groups, const void *zs,
                                  const void *gammas, int sfmt, int flags, void *ys_out, void *out_w, int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_open_fold_eval";
    if (!lagrange || (groups && (!evals || !zs))) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL lagrange, evals or zs");
    if (!ys_out && !out_w) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    const size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (d != lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d) (src/eval_form.rs:115)");
    if (lagrange->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the Lagrange SRS is resident on another GPU than this context's");
    std::vector<Fr> gm;
    KZG_TRY(fold_args(ctx, who, d, t, groups, gammas, sfmt, &gm));
    KZG_TRY(fold_points_ok(ctx, who, zs, groups));
    uint32_t log_d = 0;
    std::vector<OpenPoint> pts, rep;  // one per group | a group's point once per polynomial of a piece
    KZG_TRY(open_args(ctx, d, groups, zs, sfmt, &log_d, &pts));
    if (groups == 0) return KZG_OK;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0;
    // vectors per piece: a chunk of the evaluation stage; host input is staged piece by piece (the bound of kzg_eval_form_eval)
    const size_t P = std::max<size_t>(1, std::min<size_t>({(size_t)OE_MAX_CHUNK, t, in_dev ? t : ((size_t)1 << 22) / d}));
    try {
        rep.resize(P);
        if (!out_w) pts.resize(groups * t);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the opening points");
    }
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (!out_w) {  // the values alone: kzg_eval_form_eval with every group's point once per polynomial
        for (size_t k = groups * t; k-- > 0;) pts[k] = pts[k / t];
        return open_fr_only(ctx, 0, evals, log_d, groups * t, pts.data(), sfmt, flags & ~KZG_OUT_DEVICE, ys_out, nullptr);
    }
    BatchPipe bp;
    KZG_TRY(batch_begin(ctx, groups, groups * psz, out_w, flags, &bp));
    // Chunks of one GROUP per lane, on the plan of kzg_open_eval: the Fr stage of a chunk (values and fold of every group, then the
    // quotients of the folded vectors) on the stream of one extra lane, the MSMs of chunk c on their lanes beside the Fr stage of c + 1.
    const size_t chunk = (size_t)bp.nl;
    const int sl = bp.nl;
    const size_t qset = align_up(chunk * d * 32, 256);
    int rc = ensure_lanes(ctx, sl + 1);
    if (rc == KZG_OK)
        rc = lane_reserve(ctx, sl, stage_bytes(P * d * 32, flags) + 3 * qset + align_up(groups * t * 32, 256) + 2 * align_up(groups * 32, 256) +
                                       std::max(open_eval_fr_workspace_bytes(d, P, 1), open_eval_fr_workspace_bytes(d, chunk)) + 65536);
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, msm_workspace_bytes(lagrange, d) + 65536);
    hipStream_t fst = rc == KZG_OK ? ctx->lanes[sl].stream : nullptr;
    Fr *d_in = nullptr, *d_y = nullptr, *d_yF = nullptr, *d_gam = nullptr, *d_F = nullptr, *d_q[2] = {nullptr, nullptr};
    if (rc == KZG_OK) {
        d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, sl, P * d * 32);
        d_y = (Fr *)lane_alloc(ctx, sl, groups * t * 32);
        d_yF = (Fr *)lane_alloc(ctx, sl, groups * 32);
        d_gam = (Fr *)lane_alloc(ctx, sl, groups * 32);
        d_F = (Fr *)lane_alloc(ctx, sl, qset);
        d_q[0] = (Fr *)lane_alloc(ctx, sl, qset);
        d_q[1] = (Fr *)lane_alloc(ctx, sl, qset);
        if ((!in_dev && !d_in) || !d_y || !d_yF || !d_gam || !d_F || !d_q[0] || !d_q[1]) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    if (rc == KZG_OK && hipMemcpyAsync(d_gam, gm.data(), groups * 32, hipMemcpyHostToDevice, fst) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "copy of the challenges");
    std::vector<hipEvent_t> evs;
    try {
        evs.assign(2 + 2 * chunk, nullptr);
    } catch (const std::bad_alloc &) {
        if (rc == KZG_OK) rc = fail(ctx, KZG_ERR_ALLOC, "host memory");
    }
    for (size_t i = 0; i < evs.size() && rc == KZG_OK; i++)
        if (hipEventCreateWithFlags(&evs[i], hipEventDisableTiming) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventCreate");
    for (size_t b0 = 0, c = 0; b0 < groups && rc == KZG_OK; b0 += chunk, c++) {
        const size_t B = std::min(chunk, groups - b0), p = c & 1;
        hipEvent_t fr_done = evs[p], *lane_done = &evs[2 + p * chunk];
        if (c >= 2)  // (every chunk but the last is full: all lanes recorded in chunk c - 2)
            for (size_t l = 0; l < chunk && rc == KZG_OK; l++)
                if (hipStreamWaitEvent(fst, lane_done[l], 0) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipStreamWaitEvent");
        for (size_t b = 0; b < B && rc == KZG_OK; b++) {
            const size_t gi = b0 + b;
            for (size_t k = 0; k < P; k++) rep[k] = pts[gi];
            rc = fold_group(ctx, sl, (const Fr *)evals + gi * t * d, d, t, P, in_dev, d_in, d_gam + gi, d_F + b * d,
                            [&](const Fr *piece, size_t i0, size_t n) {
                                return ys_out ? open_eval_fr_run(ctx, sl, piece, log_d, n, rep.data(), sfmt, d_y + gi * t + i0, nullptr) : (int)KZG_OK;
                            });
        }
        if (rc == KZG_OK) rc = open_eval_fr_run(ctx, sl, d_F, log_d, B, pts.data() + b0, sfmt, d_yF + b0, d_q[p]);
        if (rc == KZG_OK && hipEventRecord(fr_done, fst) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventRecord");
        for (size_t b = 0; b < B && rc == KZG_OK; b++) {
            const int l = (int)b;
            hipStream_t st = ctx->lanes[l].stream;
            ctx->lanes[l].arena_used = 0;  // stream order makes re-use of the lane arena safe
            if (hipStreamWaitEvent(st, fr_done, 0) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipStreamWaitEvent");
            MsmPoint *res = nullptr;
            if (rc == KZG_OK) rc = batch_msm(ctx, bp, b0 + b, l, lagrange, 0, d_q[p] + b * d, d, sfmt, &res);
            if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + (b0 + b) * psz, ofmt);
            if (rc == KZG_OK && hipEventRecord(lane_done[l], st) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "hipEventRecord");
        }
    }
    if (fst && hipStreamSynchronize(fst) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "folded evaluation-form opening");
    rc = batch_end(ctx, bp, rc, out_w, groups * psz);
    for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
    if (rc == KZG_OK && ys_out) KZG_HIP_CHECK(ctx, hipMemcpy(ys_out, d_y, groups * t * 32, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int kzg_open_fold_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t t, size_t groups, const void *zs,
                                   const void *gammas, int sfmt, int flags, void *ys_out, void *out_w, int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_open_fold_coeff";
    if (!srs || (groups && (!coeffs || !zs))) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL srs, coeffs or zs");
    if (!ys_out && !out_w) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    const size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    std::vector<Fr> gm, zm;
    KZG_TRY(fold_args(ctx, who, n, t, groups, gammas, sfmt, &gm));
    KZG_TRY(fold_points_ok(ctx, who, zs, groups));
    if (n - 1 > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    try {
        zm.resize(groups);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the opening points");
    }
    for (size_t g = 0; g < groups; g++) KZG_TRY(host_scalar(ctx, (const uint8_t *)zs + 32 * g, sfmt, &zm[g]));
    if (groups == 0) return KZG_OK;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t P = std::max<size_t>(1, std::min<size_t>({(size_t)OE_MAX_CHUNK, t, in_dev ? t : ((size_t)1 << 22) / n}));
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    BatchPipe bp;
    if (out_w) {
        KZG_TRY(batch_begin(ctx, groups, groups * psz, out_w, flags, &bp));
    } else {
        bp.nl = 1;  // the values alone: lane 0, no MSM
    }
    // what the lanes share lives in the arena of one extra lane: the values and the challenges
    const int sl = bp.nl;
    int rc = ensure_lanes(ctx, sl + 1);
    if (rc == KZG_OK) rc = lane_reserve(ctx, sl, align_up(groups * t * 32, 256) + align_up(groups * 32, 256) + 4096);
    Fr *d_y = nullptr, *d_gam = nullptr;
    if (rc == KZG_OK) {
        d_y = (Fr *)lane_alloc(ctx, sl, groups * t * 32);
        d_gam = (Fr *)lane_alloc(ctx, sl, groups * 32);
        if (!d_y || !d_gam) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    if (rc == KZG_OK && hipMemcpy(d_gam, gm.data(), groups * 32, hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "copy of the challenges");
    const size_t horner = (n / 2048 + 4) * 64 + 65536;  // one poly_eval_run / quotient_linear_run
    const size_t per = (out_w ? msm_workspace_bytes(srs, n - 1) + 2 * align_up(n * 32, 256) : 0) + stage_bytes(P * n * 32, flags) + horner + 65536;
    for (int l = 0; l < bp.nl && rc == KZG_OK; l++) rc = lane_reserve(ctx, l, per);
    for (size_t gi = 0; gi < groups && rc == KZG_OK; gi++) {
        const int l = (int)(gi % (size_t)bp.nl);
        ctx->lanes[l].arena_used = 0;  // stream order makes re-use of the lane arena safe
        Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, l, P * n * 32);
        Fr *d_F = out_w ? (Fr *)lane_alloc(ctx, l, n * 32) : nullptr, *dq = out_w ? (Fr *)lane_alloc(ctx, l, n * 32) : nullptr;
        Fr *dpx = (Fr *)lane_alloc(ctx, l, 256);
        if ((!in_dev && !d_in) || (out_w && (!d_F || !dq)) || !dpx) rc = fail(ctx, KZG_ERR_ALLOC, "workspace");
        if (rc == KZG_OK)
            rc = fold_group(ctx, l, (const Fr *)coeffs + gi * t * n, n, t, P, in_dev, d_in, d_gam + gi, d_F, [&](const Fr *piece, size_t i0, size_t B) {
                const size_t mark = ctx->lanes[l].arena_used;
                for (size_t k = 0; k < B && ys_out; k++) {
                    KZG_TRY(poly_eval_run(ctx, l, piece + k * n, n, zm[gi], d_y + gi * t + i0 + k));
                    ctx->lanes[l].arena_used = mark;  // (stream order)
                }
                return (int)KZG_OK;
            });
        if (!out_w) continue;
        if (rc == KZG_OK) rc = quotient_linear_run(ctx, l, d_F, n, zm[gi], dq, dpx);
        MsmPoint *res = nullptr;
        if (rc == KZG_OK) rc = batch_msm(ctx, bp, gi, l, srs, 0, dq, n - 1, sfmt, &res);
        if (rc == KZG_OK) rc = emit_point(ctx, l, res, bp.d_out + gi * psz, ofmt);
    }
    if (out_w) {
        rc = batch_end(ctx, bp, rc, out_w, groups * psz);
    } else {
        if (hipStreamSynchronize(ctx->lanes[0].stream) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "folded coefficient-form opening");
        if (ctx->prof) prof_collect(ctx);
    }
    if (rc == KZG_OK && ys_out) KZG_HIP_CHECK(ctx, hipMemcpy(ys_out, d_y, groups * t * 32, hipMemcpyDeviceToHost));
    return rc;
}

// ---------------------------------------------------------------------------------------------
// many polynomials at many points, one two-element proof (multiopen.hip, multiopen_plan.h): D = [g]_1 and pi, DESIGN.md section 3.4d
// ---------------------------------------------------------------------------------------------
namespace {
struct MoArgs {            // what the calls check alike, before memory is touched
    std::vector<Fr> z;     // the claims' points, Montgomery
    Fr r, t;               // the challenges, Montgomery
};

// sizes, formats, pointers, indices, every z and the challenges; t_in null: a first phase
int mo_args(kzg_ctx *ctx, const char *who, size_t len, size_t n_polys, const uint32_t *poly_idx, const void *zs, size_t count, const void *r,
            const void *t_in, int sfmt, MoArgs *a) {
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!count_ok(len) || !count_ok(n_polys) || count > ((size_t)1 << 31) || n_polys > ((size_t)1 << 31) || (n_polys && len > (SIZE_MAX >> 6) / n_polys))
        return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n_polys x length or count too large");
    if (!poly_idx && count != n_polys) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": without indices there is one claim per polynomial");
    if (count && (!zs || !r || !n_polys)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL zs or r, or no polynomial");
    if (poly_idx)
        for (size_t k = 0; k < count; k++)
            if (poly_idx[k] >= n_polys) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": polynomial index >= n_polys");
    try {  // (no exception may leave through the C ABI)
        a->z.resize(count);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the opening points");
    }
    auto challenge = [&](const void *src, bool nonzero, const char *what, Fr *out) {
        Fr x;
        memcpy(x.v, src, 32);
        if (!is_canonical(x) || (nonzero && x.is_zero())) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": " + what);
        *out = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
        return (int)KZG_OK;
    };
    a->r = a->t = Fr::one();
    if (r) KZG_TRY(challenge(r, true, "the challenge r must be in [1, modulus)", &a->r));
    if (t_in) KZG_TRY(challenge(t_in, false, "the challenge t >= modulus", &a->t));
    for (size_t k = 0; k < count; k++) {
        KZG_TRY(challenge((const uint8_t *)zs + 32 * k, false, "a point z >= modulus", &a->z[k]));
        if (t_in && a->z[k] == a->t) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t equals a point z_k (draw another t)");
    }
    return KZG_OK;
}

struct MoBlob {  // host tables that go to the device in one copy
    std::vector<uint8_t> h;
    size_t add(const void *src, size_t bytes) {
        const size_t off = align_up(h.size(), 256);
        h.resize(off + std::max<size_t>(bytes, 16));
        if (src && bytes) memcpy(h.data() + off, src, bytes);
        return off;
    }
};

// the end of the four calls: g (len scalars on the device, sfmt) against the SRS -> the point at `out`; len == 0: the identity
int mo_commit_point(kzg_ctx *ctx, const kzg_srs *srs, const Fr *d_g, size_t len, int sfmt, int flags, void *out, int ofmt) {
    MsmPoint *res = nullptr;
    if (len) {
        KZG_TRY(msm_run(ctx, 0, srs, 0, d_g, len, sfmt, &res));
    } else {
        if (!(res = (MsmPoint *)lane_alloc(ctx, 0, sizeof(MsmPoint)))) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        KZG_TRY(point_set_infinity(ctx, ctx->lanes[0].stream, res));
    }
    return finish_point(ctx, 0, res, out, ofmt, flags);
}

// the weights of the second phase on the host: W_m = sum_{m(k) = m} r^k / (t - z_k), the one batch inversion of the call
int mo_poly_weights_host(kzg_ctx *ctx, const MoArgs &a, const uint32_t *poly_idx, size_t n_polys, std::vector<Fr> *W) {
    try {
        std::vector<Fr> w(a.z.size());
        W->assign(n_polys, Fr::zero());
        Fr rk = Fr::one();
        if (!mo_weights(a.z.data(), a.z.size(), a.r, a.t, &rk, w.data())) return fail(ctx, KZG_ERR_SHAPE, "t equals a point z_k");
        mo_poly_weights(w.data(), poly_idx, 0, a.z.size(), W->data());
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the weights");
    }
    return KZG_OK;
}

// v = sum_m W_m p_m - g on lane 0: g (glen <= len scalars) enters at weight -1, then the n_polys vectors; consts: W | -1 | the indices 0 .. n_polys - 1 | 0
int mo_second_phase_vector(kzg_ctx *ctx, const Fr *d_polys, size_t len, size_t n_polys, const Fr *d_g, size_t glen, const std::vector<Fr> &W, MoBlob *blob,
                           Fr *d_v) {
    hipStream_t st = ctx->lanes[0].stream;
    const Fr minus_one = neg(Fr::one());
    std::vector<uint32_t> ident(n_polys + 1);
    for (size_t m = 0; m < n_polys; m++) ident[m] = (uint32_t)m;
    ident[n_polys] = 0;
    const size_t o_w = blob->add(W.data(), n_polys * 32), o_m1 = blob->add(minus_one.v, 32), o_id = blob->add(ident.data(), (n_polys + 1) * 4);
    uint8_t *d_tab = (uint8_t *)lane_alloc(ctx, 0, blob->h.size());
    if (!d_tab) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_tab, blob->h.data(), blob->h.size(), hipMemcpyHostToDevice, st));
    if (glen < len) KZG_HIP_CHECK(ctx, hipMemsetAsync(d_v, 0, len * 32, st));
    KZG_TRY(lincomb_run(ctx, st, d_g, glen, (const uint32_t *)(d_tab + o_id) + n_polys, (const Fr *)(d_tab + o_m1), 1, false, d_v));
    return lincomb_run(ctx, st, d_polys, len, (const uint32_t *)(d_tab + o_id), (const Fr *)(d_tab + o_w), n_polys, true, d_v);
}
}  // namespace

extern "C" int kzg_fr_lincomb(kzg_ctx *ctx, const void *vecs, size_t d, size_t n_vecs, const uint32_t *idx, const void *weights, size_t count,
                              int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_fr_lincomb";
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (d == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (!count_ok(d) || !count_ok(n_vecs) || !count_ok(count) || n_vecs > ((size_t)1 << 31) || (n_vecs && d > (SIZE_MAX >> 6) / n_vecs))
        return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n_vecs x d or count too large");
    if (!out || (count && (!vecs || !idx || !weights))) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL vecs, idx, weights or out");
    for (size_t k = 0; k < count; k++)
        if (idx[k] >= n_vecs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": index >= n_vecs");
    std::vector<Fr> wm;
    try {
        wm.resize(count);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the weights");
    }
    for (size_t k = 0; k < count; k++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)weights + 32 * k, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a weight >= modulus");
        wm[k] = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
    }
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    // host vectors are staged one piece of named vectors at a time, with the running sum on the device (carry)
    const size_t P = in_dev ? count : std::max<size_t>(1, std::min(std::max<size_t>(count, 1), FOLD_STAGE_BYTES / (d * 32)));
    KZG_TRY(lane_reserve(ctx, lane, stage_bytes(P * d * 32, flags) + (out_dev ? 0 : align_up(d * 32, 256)) + align_up(count * 32 + 32, 256) +
                                        align_up(std::max(count, P) * 4 + 4, 256) + 65536));
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, P * d * 32);
    Fr *d_o = out_dev ? (Fr *)out : (Fr *)lane_alloc(ctx, lane, d * 32);
    Fr *d_w = (Fr *)lane_alloc(ctx, lane, count * 32 + 32);
    uint32_t *d_idx = (uint32_t *)lane_alloc(ctx, lane, std::max(count, P) * 4 + 4);
    if ((!in_dev && !d_in) || !d_o || !d_w || !d_idx) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    std::vector<uint32_t> local;
    StreamDrain drain{st};
    if (count) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_w, wm.data(), count * 32, hipMemcpyHostToDevice, st));
    if (in_dev) {
        if (count) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_idx, idx, count * 4, hipMemcpyHostToDevice, st));
        KZG_TRY(lincomb_run(ctx, st, (const Fr *)vecs, d, d_idx, d_w, count, false, d_o));
    } else {
        try {
            local.resize(P);
        } catch (const std::bad_alloc &) {
            return fail(ctx, KZG_ERR_ALLOC, "host memory for the indices");
        }
        for (size_t k = 0; k < P; k++) local[k] = (uint32_t)k;
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_idx, local.data(), P * 4, hipMemcpyHostToDevice, st));
        if (!count) KZG_TRY(lincomb_run(ctx, st, d_in, d, d_idx, d_w, 0, false, d_o));
        for (size_t k0 = 0; k0 < count; k0 += P) {
            const size_t B = std::min(P, count - k0);
            for (size_t k = 0; k < B; k++)
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in + k * d, (const Fr *)vecs + (size_t)idx[k0 + k] * d, d * 32, hipMemcpyHostToDevice, st));
            KZG_TRY(lincomb_run(ctx, st, d_in, d, d_idx, d_w + k0, B, k0 != 0, d_o));
        }
    }
    if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, d_o, d * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_multiopen_eval_commit(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t n_polys, const uint32_t *poly_idx,
                                         const void *zs, size_t count, const void *r, int sfmt, int flags, void *ys_out, void *g_out, void *out_d,
                                         int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_multiopen_eval_commit";
    if (!lagrange) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL lagrange");
    if (!point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    if (d != lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d) (src/eval_form.rs:115)");
    if (lagrange->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the Lagrange SRS is resident on another GPU than this context's");
    const uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    MoArgs a;
    KZG_TRY(mo_args(ctx, who, d, n_polys, poly_idx, zs, count, r, nullptr, sfmt, &a));
    if (count && !evals) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL evals");
    if (!ys_out && !g_out && !out_d) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    // ---- the plan: claims sorted by point, the distinct points classified, the off-domain ones first ----
    MoPlan plan;
    std::vector<OpenPoint> pts;
    std::vector<uint32_t> vidx, pu, src;
    std::vector<Fr> cw, cs;
    size_t n_off = 0, max_claims = 1;
    const size_t cap = mo_chunk_points(d, ctx->opt_multiopen_points_chunk);
    MoBlob blob;
    size_t o_vidx = 0, o_pu = 0, o_cw = 0, o_ps = 0, o_z = 0, o_c = 0, o_one = 0, o_zero = 0;
    try {
        mo_plan(a.z.data(), count, a.r, &plan);
        const size_t U = plan.points();
        std::vector<OpenPoint> cls(U);
        std::vector<uint8_t> on(U);
        for (size_t u = 0; u < U; u++) {
            if (open_point_classify(log_d, plan.z[u], &cls[u]) != KZG_OK) return fail(ctx, KZG_ERR_INTERNAL, "z^d == 1 but z is no power of omega");
            on[u] = cls[u].on_domain ? 1 : 0;
        }
        n_off = mo_off_domain_first(&plan, on.data(), &src);
        pts.resize(U);
        cs.resize(U);
        for (size_t u = 0; u < U; u++) {
            pts[u] = cls[src[u]];
            cs[u] = pts[u].c;
        }
        vidx.resize(count);
        pu.resize(count);
        cw.resize(count);
        for (size_t u = 0; u < U; u++)
            for (uint32_t s = plan.pstart[u]; s < plan.pstart[u + 1]; s++) {
                const uint32_t k = plan.order[s];
                vidx[s] = poly_idx ? poly_idx[k] : k;
                pu[s] = u < n_off ? (uint32_t)(u % cap) : (uint32_t)pts[u].m;  // its point of the chunk | its place on the domain
                cw[s] = plan.rk[k];
            }
        for (size_t u0 = 0; u0 < n_off; u0 += cap)
            max_claims = std::max<size_t>(max_claims, plan.pstart[std::min(u0 + cap, n_off)] - plan.pstart[u0]);
        const Fr one = Fr::one();
        const uint32_t zero = 0;
        o_vidx = blob.add(vidx.data(), count * 4);
        o_pu = blob.add(pu.data(), count * 4);
        o_cw = blob.add(cw.data(), count * 32);
        o_ps = blob.add(plan.pstart.data(), (U + 1) * 4);
        o_z = blob.add(plan.z.data(), U * 32);
        o_c = blob.add(cs.data(), U * 32);
        o_one = blob.add(one.v, 32);
        o_zero = blob.add(&zero, 4);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    }
    const size_t U = plan.points(), n_on = U - n_off;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, g_dev = in_dev && g_out;
    const bool want_g = g_out || out_d;  // the values alone: no quotient work (as the coefficient form)
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    const size_t vec = align_up(d * 32, 256), nblk = (d + 255) / 256, ncap = std::min(cap, std::max<size_t>(n_off, 1));
    KZG_TRY(lane_reserve(ctx, 0, stage_bytes(n_polys * d * 32, flags) + (g_dev ? 0 : vec) + align_up(blob.h.size(), 256) + align_up(count * 32 + 32, 256) +
                                     align_up(U * 32 + 32, 256) +
                                     (n_off ? align_up(open_powtab_bytes(d), 256) + 2 * align_up(ncap * d * 32, 256) + align_up(std::min<size_t>(max_claims, 65535) * nblk * 32, 256) : 0) +
                                     (n_on ? 2 * vec + align_up(nblk * 32, 256) : 0) + msm_workspace_bytes(lagrange, d) + 65536));
    std::vector<uint8_t> ys_sorted;  // (outlives the drain of the stream that fills it)
    StreamDrain drain{st};
    const void *d_polys = nullptr;
    if (count) KZG_TRY(stage_in(ctx, 0, evals, n_polys * d * 32, flags, &d_polys));  // host polynomials: once, whole
    Fr *d_g = g_dev ? (Fr *)g_out : (Fr *)lane_alloc(ctx, 0, d * 32);
    uint8_t *d_tab = (uint8_t *)lane_alloc(ctx, 0, blob.h.size());
    Fr *d_y = (Fr *)lane_alloc(ctx, 0, count * 32 + 32), *d_Y = (Fr *)lane_alloc(ctx, 0, U * 32 + 32);
    if (!d_g || !d_tab || !d_y || !d_Y) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_tab, blob.h.data(), blob.h.size(), hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_g, 0, d * 32, st));
    const uint32_t *t_vidx = (const uint32_t *)(d_tab + o_vidx), *t_pu = (const uint32_t *)(d_tab + o_pu), *t_ps = (const uint32_t *)(d_tab + o_ps);
    const Fr *t_cw = (const Fr *)(d_tab + o_cw), *t_z = (const Fr *)(d_tab + o_z), *t_c = (const Fr *)(d_tab + o_c);
    if (n_off) {  // chunks of at most `cap` distinct points: inverses, the values of the chunk's claims, one accumulation pass
        Fr *tab = (Fr *)lane_alloc(ctx, 0, open_powtab_bytes(d));
        Fr *den = (Fr *)lane_alloc(ctx, 0, ncap * d * 32), *iv = (Fr *)lane_alloc(ctx, 0, ncap * d * 32);
        Fr *partial = (Fr *)lane_alloc(ctx, 0, std::min<size_t>(max_claims, 65535) * nblk * 32);
        if (!tab || !den || !iv || !partial) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        KZG_TRY(open_powtab_run(ctx, st, log_d, tab));
        for (size_t u0 = 0; u0 < n_off; u0 += cap) {
            const int nz = (int)std::min(cap, n_off - u0);
            const size_t s0 = plan.pstart[u0], s1 = plan.pstart[u0 + nz];
            KZG_TRY(open_inverses_run(ctx, st, log_d, tab, plan.z.data() + u0, nz, den, iv));
            KZG_TRY(open_eval_values_idx_run(ctx, st, (const Fr *)d_polys, log_d, iv, t_vidx + s0, t_pu + s0, t_z + u0, t_c + u0, s1 - s0, partial, d_y + s0));
            if (want_g) KZG_TRY(multiopen_accum_run(ctx, st, (const Fr *)d_polys, d, t_vidx, t_cw, t_ps + u0, nz, d_y, d_Y + u0, iv, d_g));
        }
    }
    if (n_on) {  // points of the domain: the values as they are stored; F_u materialised, the unchanged quotient, added into g
        const size_t s0 = plan.pstart[n_off];
        KZG_TRY(multiopen_gather_run(ctx, st, (const Fr *)d_polys, d, t_vidx + s0, t_pu + s0, count - s0, d_y + s0));
        Fr *d_F = (Fr *)lane_alloc(ctx, 0, d * 32), *d_q = (Fr *)lane_alloc(ctx, 0, d * 32);
        if (!d_F || !d_q) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        const size_t mark = ctx->lanes[0].arena_used;
        for (size_t u = n_off; u < U && want_g; u++) {
            const size_t a0 = plan.pstart[u], a1 = plan.pstart[u + 1];
            KZG_TRY(lincomb_run(ctx, st, (const Fr *)d_polys, d, t_vidx + a0, t_cw + a0, a1 - a0, false, d_F));
            KZG_TRY(quotient_eval_run(ctx, 0, d_F, log_d, pts[u].m, sfmt, d_q));
            ctx->lanes[0].arena_used = mark;  // (stream order)
            KZG_TRY(lincomb_run(ctx, st, d_q, d, (const uint32_t *)(d_tab + o_zero), (const Fr *)(d_tab + o_one), 1, true, d_g));
        }
    }
    if (ys_out && count) {
        try {
            ys_sorted.resize(count * 32);
        } catch (const std::bad_alloc &) {
            return fail(ctx, KZG_ERR_ALLOC, "host memory for the values");
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(ys_sorted.data(), d_y, count * 32, hipMemcpyDeviceToHost, st));
    }
    if (g_out && !g_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(g_out, d_g, d * 32, hipMemcpyDeviceToHost, st));
    if (out_d) {
        KZG_TRY(mo_commit_point(ctx, lagrange, d_g, count ? d : 0, sfmt, flags, out_d, ofmt));  // the ONE MSM of the call
    } else {
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
        if (ctx->prof) prof_collect(ctx);
    }
    for (size_t s = 0; s < ys_sorted.size() / 32; s++) memcpy((uint8_t *)ys_out + 32 * (size_t)plan.order[s], ys_sorted.data() + 32 * s, 32);
    return KZG_OK;
}

extern "C" int kzg_multiopen_eval_finish(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t n_polys, const uint32_t *poly_idx,
                                         const void *zs, size_t count, const void *r, const void *t, const void *g_in, int sfmt, int flags, void *y_out,
                                         void *out_pi, int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_multiopen_eval_finish";
    if (!lagrange || !t) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL lagrange or t");
    if (!point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    if (d != lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d) (src/eval_form.rs:115)");
    if (lagrange->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the Lagrange SRS is resident on another GPU than this context's");
    const uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    MoArgs a;
    KZG_TRY(mo_args(ctx, who, d, n_polys, poly_idx, zs, count, r, t, sfmt, &a));
    if (count && (!evals || !g_in)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL evals or g");
    if (!y_out && !out_pi) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    OpenPoint pt;
    if (open_point_classify(log_d, a.t, &pt) != KZG_OK) return fail(ctx, KZG_ERR_INTERNAL, "t^d == 1 but t is no power of omega");
    std::vector<Fr> W;
    KZG_TRY(mo_poly_weights_host(ctx, a, poly_idx, n_polys, &W));
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    const size_t vec = align_up(d * 32, 256);
    KZG_TRY(lane_reserve(ctx, 0, stage_bytes(n_polys * d * 32, flags) + stage_bytes(d * 32, flags) + 2 * vec + align_up(n_polys * 36 + 1024, 256) + 1024 +
                                     open_eval_fr_workspace_bytes(d, 1) + msm_workspace_bytes(lagrange, d) + 65536));
    MoBlob blob;  // (outlives the drain of the stream that reads it)
    StreamDrain drain{st};
    if (!count) {  // no claim: v = 0
        if (y_out) memset(y_out, 0, 32);
        if (out_pi) return mo_commit_point(ctx, lagrange, nullptr, 0, sfmt, flags, out_pi, ofmt);
        return KZG_OK;
    }
    const void *d_polys = nullptr, *d_g = nullptr;
    KZG_TRY(stage_in(ctx, 0, evals, n_polys * d * 32, flags, &d_polys));  // host polynomials: once, whole
    KZG_TRY(stage_in(ctx, 0, g_in, d * 32, flags, &d_g));
    Fr *d_v = (Fr *)lane_alloc(ctx, 0, d * 32), *d_q = (Fr *)lane_alloc(ctx, 0, d * 32), *d_y = (Fr *)lane_alloc(ctx, 0, 256);
    if (!d_v || !d_q || !d_y) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    try {
        KZG_TRY(mo_second_phase_vector(ctx, (const Fr *)d_polys, d, n_polys, (const Fr *)d_g, d, W, &blob, d_v));
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the tables");
    }
    KZG_TRY(open_eval_fr_run(ctx, 0, d_v, log_d, 1, &pt, sfmt, d_y, out_pi ? d_q : nullptr));  // v(t) and the values of (v - v(t)) / (X - t)
    if (y_out) KZG_HIP_CHECK(ctx, hipMemcpyAsync(y_out, d_y, 32, hipMemcpyDeviceToHost, st));
    if (out_pi) return mo_commit_point(ctx, lagrange, d_q, d, sfmt, flags, out_pi, ofmt);  // the ONE MSM of the call
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_multiopen_coeff_commit(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t n_polys, const uint32_t *poly_idx,
                                          const void *zs, size_t count, const void *r, int sfmt, int flags, void *ys_out, void *g_out, void *out_d,
                                          int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_multiopen_coeff_commit";
    if (!srs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL srs");
    if (!point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty polynomials");
    if (n - 1 > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    MoArgs a;
    KZG_TRY(mo_args(ctx, who, n, n_polys, poly_idx, zs, count, r, nullptr, sfmt, &a));
    if (count && !coeffs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL coeffs");
    if (!ys_out && !g_out && !out_d) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    MoPlan plan;
    std::vector<uint32_t> vidx;
    std::vector<Fr> cw;
    MoBlob blob;
    size_t o_vidx = 0, o_cw = 0, o_one = 0, o_zero = 0;
    try {
        mo_plan(a.z.data(), count, a.r, &plan);
        vidx.resize(count);
        cw.resize(count);
        for (size_t s = 0; s < count; s++) {
            vidx[s] = poly_idx ? poly_idx[plan.order[s]] : plan.order[s];
            cw[s] = plan.rk[plan.order[s]];
        }
        const Fr one = Fr::one();
        const uint32_t zero = 0;
        o_vidx = blob.add(vidx.data(), count * 4);
        o_cw = blob.add(cw.data(), count * 32);
        o_one = blob.add(one.v, 32);
        o_zero = blob.add(&zero, 4);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    }
    const size_t U = plan.points(), glen = n - 1;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, g_dev = in_dev && g_out;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    const size_t vec = align_up(n * 32, 256), horner = (n / 2048 + 4) * 64 + 65536;  // one poly_eval_run / quotient_linear_run
    KZG_TRY(lane_reserve(ctx, 0, stage_bytes(n_polys * n * 32, flags) + 3 * vec + align_up(blob.h.size(), 256) + align_up(count * 32 + 32, 256) + 1024 + horner +
                                     msm_workspace_bytes(srs, glen) + 65536));
    std::vector<uint8_t> ys_sorted;  // (outlives the drain of the stream that fills it)
    StreamDrain drain{st};
    const void *d_polys = nullptr;
    if (count) KZG_TRY(stage_in(ctx, 0, coeffs, n_polys * n * 32, flags, &d_polys));  // host polynomials: once, whole
    Fr *d_g = g_dev ? (Fr *)g_out : (Fr *)lane_alloc(ctx, 0, glen * 32 + 32);
    uint8_t *d_tab = (uint8_t *)lane_alloc(ctx, 0, blob.h.size());
    Fr *d_y = (Fr *)lane_alloc(ctx, 0, count * 32 + 32), *d_F = (Fr *)lane_alloc(ctx, 0, n * 32), *d_q = (Fr *)lane_alloc(ctx, 0, n * 32);
    Fr *d_px = (Fr *)lane_alloc(ctx, 0, 256);
    if (!d_g || !d_tab || !d_y || !d_F || !d_q || !d_px) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_tab, blob.h.data(), blob.h.size(), hipMemcpyHostToDevice, st));
    if (glen) KZG_HIP_CHECK(ctx, hipMemsetAsync(d_g, 0, glen * 32, st));
    const uint32_t *t_vidx = (const uint32_t *)(d_tab + o_vidx);
    const Fr *t_cw = (const Fr *)(d_tab + o_cw);
    const size_t mark = ctx->lanes[0].arena_used;
    for (size_t u = 0; u < U; u++) {
        const size_t a0 = plan.pstart[u], a1 = plan.pstart[u + 1];
        for (size_t s = a0; s < a1 && ys_out; s++) {  // the values: Polynomial::eval per claim
            KZG_TRY(poly_eval_run(ctx, 0, (const Fr *)d_polys + (size_t)vidx[s] * n, n, plan.z[u], d_y + s));
            ctx->lanes[0].arena_used = mark;  // (stream order)
        }
        if (!glen || (!g_out && !out_d)) continue;
        KZG_TRY(lincomb_run(ctx, st, (const Fr *)d_polys, n, t_vidx + a0, t_cw + a0, a1 - a0, false, d_F));
        KZG_TRY(quotient_linear_run(ctx, 0, d_F, n, plan.z[u], d_q, d_px));  // (F_u - F_u(z_u)) / (X - z_u): n - 1 coefficients
        ctx->lanes[0].arena_used = mark;
        KZG_TRY(lincomb_run(ctx, st, d_q, glen, (const uint32_t *)(d_tab + o_zero), (const Fr *)(d_tab + o_one), 1, true, d_g));
    }
    if (ys_out && count) {
        try {
            ys_sorted.resize(count * 32);
        } catch (const std::bad_alloc &) {
            return fail(ctx, KZG_ERR_ALLOC, "host memory for the values");
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(ys_sorted.data(), d_y, count * 32, hipMemcpyDeviceToHost, st));
    }
    if (g_out && !g_dev && glen) KZG_HIP_CHECK(ctx, hipMemcpyAsync(g_out, d_g, glen * 32, hipMemcpyDeviceToHost, st));
    if (out_d) {
        KZG_TRY(mo_commit_point(ctx, srs, d_g, count ? glen : 0, sfmt, flags, out_d, ofmt));  // the ONE MSM of the call
    } else {
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
        if (ctx->prof) prof_collect(ctx);
    }
    for (size_t s = 0; s < ys_sorted.size() / 32; s++) memcpy((uint8_t *)ys_out + 32 * (size_t)plan.order[s], ys_sorted.data() + 32 * s, 32);
    return KZG_OK;
}

extern "C" int kzg_multiopen_coeff_finish(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t n_polys, const uint32_t *poly_idx,
                                          const void *zs, size_t count, const void *r, const void *t, const void *g_in, int sfmt, int flags, void *y_out,
                                          void *out_pi, int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_multiopen_coeff_finish";
    if (!srs || !t) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL srs or t");
    if (!point_format_bytes(ofmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty polynomials");
    if (n - 1 > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    MoArgs a;
    KZG_TRY(mo_args(ctx, who, n, n_polys, poly_idx, zs, count, r, t, sfmt, &a));
    const size_t glen = n - 1;
    if (count && (!coeffs || (!g_in && glen))) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL coeffs or g");
    if (!y_out && !out_pi) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no output");
    std::vector<Fr> W;
    KZG_TRY(mo_poly_weights_host(ctx, a, poly_idx, n_polys, &W));
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    const size_t vec = align_up(n * 32, 256), horner = (n / 2048 + 4) * 64 + 65536;
    KZG_TRY(lane_reserve(ctx, 0, stage_bytes(n_polys * n * 32, flags) + stage_bytes(n * 32, flags) + 2 * vec + align_up(n_polys * 36 + 1024, 256) + 1024 + horner +
                                     msm_workspace_bytes(srs, glen) + 65536));
    MoBlob blob;  // (outlives the drain of the stream that reads it)
    StreamDrain drain{st};
    if (!count) {
        if (y_out) memset(y_out, 0, 32);
        if (out_pi) return mo_commit_point(ctx, srs, nullptr, 0, sfmt, flags, out_pi, ofmt);
        return KZG_OK;
    }
    const void *d_polys = nullptr, *d_g = nullptr;
    KZG_TRY(stage_in(ctx, 0, coeffs, n_polys * n * 32, flags, &d_polys));  // host polynomials: once, whole
    KZG_TRY(stage_in(ctx, 0, g_in, glen * 32, flags, &d_g));
    Fr *d_v = (Fr *)lane_alloc(ctx, 0, n * 32), *d_q = (Fr *)lane_alloc(ctx, 0, n * 32), *d_y = (Fr *)lane_alloc(ctx, 0, 256);
    if (!d_v || !d_q || !d_y) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    try {
        KZG_TRY(mo_second_phase_vector(ctx, (const Fr *)d_polys, n, n_polys, (const Fr *)d_g, glen, W, &blob, d_v));
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the tables");
    }
    KZG_TRY(quotient_linear_run(ctx, 0, d_v, n, a.t, d_q, d_y));  // (v - v(t)) / (X - t) and v(t)
    if (y_out) KZG_HIP_CHECK(ctx, hipMemcpyAsync(y_out, d_y, 32, hipMemcpyDeviceToHost, st));
    if (out_pi) return mo_commit_point(ctx, srs, d_q, glen, sfmt, flags, out_pi, ofmt);  // the ONE MSM of the call
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

// ---------------------------------------------------------------------------------------------
// witnesses
// ---------------------------------------------------------------------------------------------
extern "C" int kzg_witness_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, const void *x,
                                 const void *y, int sfmt, int flags, void *out, int ofmt) {
    // KZGProver::create_witness (src/coeff_form.rs:66-81)
    if (!ctx || !srs || !coeffs || !x || !y || !out || n == 0) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (n - 1 > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    Fr xm, ym;
    KZG_TRY(host_scalar(ctx, x, sfmt, &xm));
    KZG_TRY(host_scalar(ctx, y, sfmt, &ym));  // y is only compared with p(x) below, but the rule for host scalars holds for it too: < r
    size_t need = msm_workspace_bytes(srs, n - 1) + stage_bytes(n * 32, flags) + n * 32 + (n / 2048 + 4) * 64 + 65536;
    KZG_TRY(lane_reserve(ctx, lane, need));
    hipStream_t st = ctx->lanes[lane].stream;
    const void *d = nullptr;
    KZG_TRY(stage_in(ctx, lane, coeffs, n * 32, flags, &d));
    Fr *dq = (Fr *)lane_alloc(ctx, lane, n * 32);
    Fr *dpx = (Fr *)lane_alloc(ctx, lane, 256);
    if (!dq || !dpx) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_TRY(quotient_linear_run(ctx, lane, (const Fr *)d, n, xm, dq, dpx));
    // p(x) goes to the lane's PINNED staging buffer (behind the 144 bytes finish_point uses): a device-to-host copy into pageable
    // memory -- the stack variable this used to be -- makes hipMemcpyAsync wait for the stream, so the host sat out the three quotient
    // kernels before it could enqueue the MSM's fourteen, and the GPU then idled between those short kernels (0.4-0.5 ms of a lone
    // create_witness; profiles/r06_prof_witness_coeff.txt)
    KZG_TRY(lane_pinned(ctx, lane, 4096));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(ctx->lanes[lane].pinned + 1024, dpx, 32, hipMemcpyDeviceToHost, st));
    MsmPoint *res = nullptr;
    KZG_TRY(lease_msm(ctx, ls, srs, 0, dq, n - 1, sfmt, &res));
    KZG_TRY(finish_point(ctx, lane, res, out, ofmt, flags));  // synchronises the stream
    Fr px;
    memcpy(px.v, ctx->lanes[lane].pinned + 1024, 32);
    // remainder of (p - y)/(X - x) is p(x) - y: Some(_) => Err(PointNotOnPolynomial)
    if (memcmp(px.v, y, 32) != 0) return fail(ctx, KZG_ERR_POINT_NOT_ON_POLY, "point not on polynomial!");
    return KZG_OK;
}

extern "C" int kzg_witness_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t i, int sfmt,
                                int flags, void *out, int ofmt) {
    // KZGProverEvalForm::create_witness (src/eval_form.rs:124-140)
    if (!ctx || !lagrange || !evals || !out) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    if (i >= d) return fail(ctx, KZG_ERR_SHAPE, "evaluation index out of range (reference: index panic)");
    if (d > lagrange->n) return fail(ctx, KZG_ERR_SHAPE, "evaluations longer than the Lagrange SRS (reference: slice panic)");
    uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    size_t need = msm_workspace_bytes(lagrange, d) + stage_bytes(d * 32, flags) + d * 32 + (d / 256 + 4) * 32 + 65536;
    KZG_TRY(lane_reserve(ctx, lane, need));
    const void *de = nullptr;
    KZG_TRY(stage_in(ctx, lane, evals, d * 32, flags, &de));
    Fr *dq = (Fr *)lane_alloc(ctx, lane, d * 32);
    if (!dq) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_TRY(quotient_eval_run(ctx, lane, (const Fr *)de, log_d, i, sfmt, dq));
    MsmPoint *res = nullptr;
    KZG_TRY(lease_msm(ctx, ls, lagrange, 0, dq, d, sfmt, &res));
    return finish_point(ctx, lane, res, out, ofmt, flags);
}

static int verify_against(kzg_ctx *ctx, int lane, const MsmPoint *res, const void *commitment, int pfmt, int *ok) {
    size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144)
        return fail(ctx, KZG_ERR_SHAPE, "verify_poly takes the commitment in an affine format (KZGCommitment = G1Affine)");
    uint8_t mine[96];
    KZG_TRY(finish_point(ctx, lane, res, mine, pfmt, 0));
    *ok = memcmp(mine, commitment, psz) == 0;
    return KZG_OK;
}

extern "C" int kzg_verify_poly_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *commitment, int pfmt,
                                     const void *coeffs, size_t n, int sfmt, int flags, int *ok) {
    // KZGVerifier::verify_poly (src/coeff_form.rs:119-124)
    if (!ctx || !srs || !commitment || !ok || (!coeffs && n)) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (n > srs->n) return fail(ctx, KZG_ERR_SHAPE, "polynomial longer than the SRS (reference: slice index panic)");
    KZG_TRY(lane_reserve(ctx, lane, msm_workspace_bytes(srs, n) + stage_bytes(n * 32, flags) + 8192));
    const void *d = nullptr;
    KZG_TRY(stage_in(ctx, lane, coeffs, n * 32, flags, &d));
    MsmPoint *res = nullptr;
    KZG_TRY(lease_msm(ctx, ls, srs, 0, d, n, sfmt, &res));
    return verify_against(ctx, lane, res, commitment, pfmt, ok);
}

extern "C" int kzg_verify_poly_eval(kzg_ctx *ctx, const kzg_srs *monomial, const void *commitment, int pfmt,
                                    const void *evals, size_t d, int sfmt, int flags, int *ok) {
    // KZGVerifierEvalForm::verify_poly (src/eval_form.rs:162-171): ifft, then the monomial-basis MSM
    if (!ctx || !monomial || !commitment || !ok || !evals) return KZG_ERR_SHAPE;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(check_sfmt(ctx, sfmt));
    if (!is_pow2(d)) return fail(ctx, KZG_ERR_SHAPE, "evaluation domain size must be a power of two");
    if (d > monomial->n) return fail(ctx, KZG_ERR_SHAPE, "polynomial longer than the SRS (reference: slice index panic)");
    uint32_t log_d = (uint32_t)ilog2_ceil(d);
    if (log_d >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    KZG_TRY(lane_reserve(ctx, lane, msm_workspace_bytes(monomial, d) + d * 32 + ntt_workspace_bytes(log_d) + 65536));
    hipStream_t st = ctx->lanes[lane].stream;
    Fr *work = (Fr *)lane_alloc(ctx, lane, d * 32);
    if (!work) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(work, evals, d * 32, (flags & KZG_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    KZG_TRY(ntt_run(ctx, lane, work, log_d, 1));
    MsmPoint *res = nullptr;
    KZG_TRY(lease_msm(ctx, ls, monomial, 0, work, d, sfmt, &res));
    return verify_against(ctx, lane, res, commitment, pfmt, ok);
}

#ifdef KZG_TEST_HOOKS
#include "../../include/kzg_mi355x_test.h"
// ---------------------------------------------------------------------------------------------
// test hooks
// ---------------------------------------------------------------------------------------------
template <class K, class... Args>
static int run_test_kernel(kzg_ctx *ctx, const char *name, K kern, size_t n, size_t in_elem, int n_in, const void *a,
                           const void *b, size_t in_elem_b, void *out, size_t out_elem) {
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(lane_reserve(ctx, 0, n * (in_elem + in_elem_b + out_elem) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *da = lane_alloc(ctx, 0, n * in_elem + 16), *db = lane_alloc(ctx, 0, n * in_elem_b + 16),
         *dout = lane_alloc(ctx, 0, n * out_elem + 16);
    if (!da || !db || !dout) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(da, a, n * in_elem, hipMemcpyHostToDevice, st));
    if (n_in > 1) KZG_HIP_CHECK(ctx, hipMemcpyAsync(db, b, n * in_elem_b, hipMemcpyHostToDevice, st));
    kern(st, da, db, dout);
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, n * out_elem, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    return KZG_OK;
}

extern "C" int kzg_test_fr_mul(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out) {
    if (!ctx || !n) return KZG_ERR_SHAPE;
    unsigned grid = (unsigned)((n + 255) / 256);
    return run_test_kernel(ctx, "k_test_fr_mul", [&](hipStream_t st, void *da, void *db, void *dout) {
        hipLaunchKernelGGL(k_test_fr_mul, dim3(grid), dim3(256), 0, st, (const Fr *)da, (const Fr *)db, n, (Fr *)dout);
    }, n, 32, 2, a, b, 32, out, 32);
}
extern "C" int kzg_test_fq_mul(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out) {
    if (!ctx || !n) return KZG_ERR_SHAPE;
    unsigned grid = (unsigned)((n + 255) / 256);
    return run_test_kernel(ctx, "k_test_fq_mul", [&](hipStream_t st, void *da, void *db, void *dout) {
        hipLaunchKernelGGL(k_test_fq_mul, dim3(grid), dim3(256), 0, st, (const Fq *)da, (const Fq *)db, n, (Fq *)dout);
    }, n, 48, 2, a, b, 48, out, 48);
}
extern "C" int kzg_test_fr_inv(kzg_ctx *ctx, const void *a, size_t n, void *out) {
    if (!ctx || !n) return KZG_ERR_SHAPE;
    unsigned grid = (unsigned)((n + 255) / 256);
    return run_test_kernel(ctx, "k_test_fr_inv", [&](hipStream_t st, void *da, void *, void *dout) {
        hipLaunchKernelGGL(k_test_fr_inv, dim3(grid), dim3(256), 0, st, (const Fr *)da, n, (Fr *)dout);
    }, n, 32, 1, a, nullptr, 0, out, 32);
}
extern "C" int kzg_test_g1_add(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out) {
    if (!ctx || !n) return KZG_ERR_SHAPE;
    unsigned grid = (unsigned)((n + 255) / 256);
    return run_test_kernel(ctx, "k_test_g1_add", [&](hipStream_t st, void *da, void *db, void *dout) {
        hipLaunchKernelGGL(k_test_g1_add, dim3(grid), dim3(256), 0, st, (const G1Affine *)da, (const G1Affine *)db, n,
                           (G1Affine *)dout);
    }, n, 96, 2, a, b, 96, out, 96);
}
// pretend an SRS lives on another GPU (one-GPU test boxes): the device check of msm_run
extern "C" int kzg_test_srs_set_device(kzg_srs *srs, int device) {
    if (!srs) return KZG_ERR_SHAPE;
    srs->device = device;
    return KZG_OK;
}
extern "C" int kzg_test_g1_mul(kzg_ctx *ctx, const void *p, const void *k, size_t n, void *out) {
    if (!ctx || !n) return KZG_ERR_SHAPE;
    unsigned grid = (unsigned)((n + 255) / 256);
    return run_test_kernel(ctx, "k_test_g1_mul", [&](hipStream_t st, void *da, void *db, void *dout) {
        hipLaunchKernelGGL(k_test_g1_mul, dim3(grid), dim3(256), 0, st, (const G1Affine *)da, (const Fr *)db, n,
                           (G1Affine *)dout);
    }, n, 96, 2, p, k, 32, out, 96);
}
#endif  // KZG_TEST_HOOKS

