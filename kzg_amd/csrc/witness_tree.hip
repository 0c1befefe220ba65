// witness_tree.hip -- batched openings on a point tree (kzg_point_tree): the verifier of KZGVerifier::verify_eval_batched
// (src/coeff_form.rs:144-182) for callers who hold a plan, without that call's bound of 16,384 points.
//
// kzg_verify_eval_tree checks `count` openings at ONE point set:  e(w_c, hz) == e(C_c - gr_c, hs[0])  with
//   hz   = [M(tau)]_2 = MSM(hs[0 .. k], M): the plan's product M never leaves the device, its k + 1 coefficients go through the bucket
//          method of g2_msm.hip ONCE per call;
//   gr_c = MSM(gs[0 .. k), r_c): the G1 pipeline of a lone MSM, one after the other on lane 0;
// and one GPU thread per check (k_vet_check), as kzg_verify_eval: hz takes its Miller lines on the fly, hs[0] its stored ones.
//
// kzg_witness_coeff_tree is the prover of KZGProver::create_witness_batched (:83-111) on a plan: with M the plan's product (resident,
// Montgomery) and p_b = q_b M + r_b, the division stages of poly_divide.hip (PolyDivisor: the series inverse of rev(M) ONCE per call)
// give q_b and r_b per polynomial on the device, a chunk of polynomials at a time in a workspace of the call's own; the chunk's
// quotients go to the batched MSM pipeline (msm_batch_strided) without leaving HBM; a claim ys_b holds iff r_b equals the tree
// interpolation of ys_b (point_tree_interpolate_run), compared on the device (k_wt_compare).
// DESIGN.md section 3.6b.
#include <algorithm>

#include "vcb_shared.h"

namespace kzg {

// ok[c] = e(w_c, hz) e(-(C_c - gr_c), h0) == 1
__global__ __launch_bounds__(64) void k_vet_check(const G1Xyzz *C, const G1Affine *gr, const G1Xyzz *w, const G2Affine *hz, const G2Affine *h0,
                                                  const Fq2 *lines_h0, size_t count, uint8_t *ok) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    G1Affine P[2];
    G2Affine Q[2], T[2];
    const Fq2 *tabs[2] = {nullptr, lines_h0};
    G1Xyzz ngr = G1Xyzz::from_affine(g1_neg(gr[c]));
    P[0] = g1_to_affine(w[c]);
    P[1] = g1_neg(g1_to_affine(g1_add(C[c], ngr)));
    Q[0] = *hz;
    Q[1] = *h0;
    ok[c] = pairing_product_is_one(P, Q, T, 2, tabs) ? 1 : 0;
}

// status[b] = KZG_ERR_POINT_NOT_ON_POLY unless r_b == the interpolant of the claim, coefficient by coefficient (both in one form)
__global__ __launch_bounds__(256) void k_wt_compare(const Fr *r, const Fr *want, size_t k, size_t total, int *status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    Fr a = r[i], b = want[i];
    reduce_once(a);
    reduce_once(a);
    reduce_once(b);
    reduce_once(b);
    if (!(a == b)) status[i / k] = KZG_ERR_POINT_NOT_ON_POLY;
}

constexpr size_t WT_CHUNK_COEFFS = (size_t)1 << 24, WT_CHUNK_MAX = 16;  // polynomials per chunk: clamp(2^24 / max(n, K), 1, 16): 16 up to n = 2^20

}  // namespace kzg

using namespace kzg;

namespace {
struct DevBlock {  // the workspace of one call
    char *p = nullptr;
    size_t used = 0, bytes = 0;
    ~DevBlock() {
        if (p) hipFree(p);
    }
    Fr *take(size_t elems) {
        Fr *r = (Fr *)(p + used);
        used += align_up(elems * 32 + 32, 256);
        return r;
    }
};
}  // namespace

extern "C" int kzg_witness_coeff_tree(kzg_ctx *ctx, const kzg_srs *srs, const kzg_point_tree *plan, const void *coeffs, size_t n, size_t batch,
                                      const void *ys, int sfmt, int flags, void *out_w, int ofmt, void *out_r, int *status) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!srs || !plan || !coeffs || !out_w) return fail(ctx, KZG_ERR_SHAPE, "kzg_witness_coeff_tree: NULL srs, plan, coeffs or out_w");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    PointTreeView pv;
    point_tree_view(plan, &pv);
    const size_t k = pv.k, K = pv.K;
    if (pv.device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "kzg_witness_coeff_tree: the point tree is resident on another GPU");
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    if (!pv.distinct) return fail(ctx, KZG_ERR_SHAPE, "kzg_witness_coeff_tree: two points of the plan coincide (the reference panics in invert().unwrap())");
    if (n == 0 || n > ((size_t)1 << 27)) return fail(ctx, KZG_ERR_SHAPE, "kzg_witness_coeff_tree: polynomials of 1 .. 2^27 coefficients");
    if (n > k && n - k > srs->n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (batch > ((size_t)1 << 50) / std::max(n, k)) return fail(ctx, KZG_ERR_SHAPE, "kzg_witness_coeff_tree: batch x n too large");
    if (batch == 0) return KZG_OK;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    PolyDivisor dv;
    poly_divisor_shape(n, k + 1, &dv);
    const size_t m = dv.m;  // quotient coefficients: n - k, or 0
    const size_t C = std::min(batch, std::min(WT_CHUNK_MAX, std::max<size_t>(1, WT_CHUNK_COEFFS / std::max(n, K))));
    const size_t arena_need = ntt_workspace_bytes(std::max(dv.log_tq, dv.log_N)) + 65536;

    DevBlock ws;
    {  // sizes first (take() only counts while p is null), then one allocation
        for (int pass = 0; pass < 2; pass++) {
            ws.used = 0;
            if (m) {
                dv.f = ws.take(dv.fl_all), dv.g = ws.take(m), dv.G = ws.take(dv.Tq), dv.A = ws.take(dv.Tq), dv.B = ws.take(dv.N);
                dv.af = ws.take(dv.N), dv.qf = ws.take(dv.N), dv.tmp0 = ws.take(dv.t0), dv.tmp1 = ws.take(dv.t1);
            }
            if (pass == 0) {
                ws.bytes = ws.used + 2 * align_up(C * n * 32 + 32, 256) + 4 * align_up(C * k * 32 + 32, 256) + align_up(C * 2 * K * 32 + 32, 256) +
                           align_up(C * K * 32 + 32, 256) + align_up(C * 32 + 32, 256) + align_up(psz + 512, 256) + 4096;
                KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
                if (hipMalloc((void **)&ws.p, ws.bytes) != hipSuccess) {
                    ws.p = nullptr;
                    return fail(ctx, KZG_ERR_ALLOC, "hipMalloc(kzg_witness_coeff_tree workspace)");
                }
            }
        }
    }
    Fr *d_in = in_dev ? nullptr : ws.take(C * n), *d_q = ws.take(C * std::max<size_t>(m, 1)), *d_r = ws.take(C * k);
    Fr *d_ys = (ys && !in_dev) ? ws.take(C * k) : nullptr, *d_want = ys ? ws.take(C * k) : nullptr;
    Fr *d_R = ys ? ws.take(C * 2 * K) : nullptr, *d_A2 = ys ? ws.take(C * K) : nullptr;
    int *d_status = (int *)ws.take(C);
    uint8_t *d_id = (uint8_t *)ws.take(psz / 32 + 16);
    if (ws.used > ws.bytes) return fail(ctx, KZG_ERR_INTERNAL, "kzg_witness_coeff_tree: workspace accounting");

    bool any_fail = false;
    std::vector<int> h_status(C);
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const size_t B = std::min(C, batch - b0);
        {  // the Fr stage of the chunk, on lane 0
            Guard g(ctx);
            KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
            KZG_TRY(lane_reserve(ctx, 0, arena_need));
            hipStream_t st = ctx->lanes[0].stream;
            if (b0 == 0) {
                if (m) {
                    KZG_TRY(poly_divisor_run(ctx, 0, pv.product, 0, true, dv));  // M is Montgomery already
                } else {  // n <= k: every witness is the identity
                    MsmPoint *inf = (MsmPoint *)lane_alloc(ctx, 0, sizeof(MsmPoint));
                    if (!inf) return fail(ctx, KZG_ERR_ALLOC, "workspace");
                    KZG_TRY(point_set_infinity(ctx, st, inf));
                    KZG_TRY(emit_point(ctx, 0, inf, d_id, ofmt));
                }
            }
            const Fr *src = (const Fr *)coeffs + b0 * n;
            if (!in_dev) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * n * 32, hipMemcpyHostToDevice, st));
                src = d_in;
            }
            KZG_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, C * sizeof(int), st));
            for (size_t bi = 0; bi < B; bi++) {
                if (m) {
                    KZG_TRY(poly_dividend_run(ctx, 0, dv, src + bi * n, d_q + bi * m, true, d_r + bi * k, d_status + C));  // (the `exact` word behind the C status words is not read)
                } else {
                    KZG_TRY(poly_pad_run(ctx, st, src + bi * n, n, d_r + bi * k, k));
                    if (out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out_w + (b0 + bi) * psz, d_id, psz, hipMemcpyDeviceToDevice, st));
                }
            }
            if (!m && !out_dev) {
                KZG_TRY(lane_pinned(ctx, 0, 4096));
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(ctx->lanes[0].pinned, d_id, psz, hipMemcpyDeviceToHost, st));
            }
            if (ys) {
                const Fr *yv = (const Fr *)ys + b0 * k;
                if (!in_dev) {
                    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_ys, yv, B * k * 32, hipMemcpyHostToDevice, st));
                    yv = d_ys;
                }
                KZG_TRY(point_tree_interpolate_run(ctx, st, plan, yv, B, d_R, d_A2, d_want));
                KZG_LAUNCH(ctx, st, "k_wt_compare", k_wt_compare, (unsigned)((B * k + 255) / 256), 256, 0, (const Fr *)d_r, (const Fr *)d_want, k, B * k, d_status);
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(h_status.data(), d_status, B * sizeof(int), hipMemcpyDeviceToHost, st));
            }
            if (out_r) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)out_r + b0 * k, d_r, B * k * 32, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
            KZG_HIP_CHECK(ctx, hipGetLastError());
            if (!m && !out_dev)
                for (size_t bi = 0; bi < B; bi++) memcpy((uint8_t *)out_w + (b0 + bi) * psz, ctx->lanes[0].pinned, psz);
            if (ctx->prof) prof_collect(ctx);
        }
        if (ys)
            for (size_t bi = 0; bi < B; bi++) {
                if (h_status[bi]) any_fail = true;
                if (status) status[b0 + bi] = h_status[bi];
            }
        // the chunk's quotients, resident, through the batched MSM pipeline (it takes the context itself)
        if (m) KZG_TRY(msm_batch_strided(ctx, srs, 0, d_q, m, B, m * 32, sfmt, KZG_IN_DEVICE | (flags & KZG_OUT_DEVICE), (uint8_t *)out_w + b0 * psz, ofmt, true));
    }
    if (ys && !status && any_fail) return fail(ctx, KZG_ERR_POINT_NOT_ON_POLY, "point not on polynomial!");
    return KZG_OK;
}

extern "C" int kzg_verify_eval_tree(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const kzg_point_tree *plan, const void *r_coeffs,
                                    int sfmt, const void *commitments, const void *witnesses, int pfmt, size_t count, uint8_t *ok) {
    if (!ctx || !gs || !hs || !plan || !r_coeffs || !commitments || !witnesses || !ok) return KZG_ERR_SHAPE;  // (also at count == 0)
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / witnesses are affine (G1Affine)");
    PointTreeView pv;
    point_tree_view(plan, &pv);
    const size_t k = pv.k;
    if (pv.device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_eval_tree: the point tree is resident on another GPU");
    if (gs->device != ctx->device || hs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    if (!pv.distinct) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_eval_tree: two points of the plan coincide");
    if (k >= hs->n) return fail(ctx, KZG_ERR_SHAPE, "z longer than hs (reference: slice index panic)");
    if (k > gs->n) return fail(ctx, KZG_ERR_SHAPE, "witness.r longer than gs (reference: slice index panic)");
    if (count > ((size_t)1 << 40) / k) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_eval_tree: count x k too large");
    if (!count) return KZG_OK;
    KZG_TRY(lane_reserve(ctx, 0, align_up((k + 2) * 32, 256) + g2_msm_bucket_workspace_bytes(ctx) + msm_workspace_bytes(gs, k) + align_up(k * 32 + 32, 256) +
                                     count * (2 * psz + 2 * sizeof(G1Xyzz) + sizeof(G1Affine) + 1 + 1024) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    int *bad = (int *)lane_alloc(ctx, 0, 256);
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, 0, count);
    G1Affine *gr = (G1Affine *)lane_alloc(ctx, 0, count * sizeof(G1Affine));
    G2Affine *hz = (G2Affine *)lane_alloc(ctx, 0, sizeof(G2Affine));
    Fr *dr = (Fr *)lane_alloc(ctx, 0, k * 32 + 32);
    if (!bad || !d_ok || !gr || !hz || !dr) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    G1Xyzz *C = nullptr, *W = nullptr;
    KZG_TRY(g1_inputs(ctx, 0, commitments, count, pfmt, &C, bad));
    KZG_TRY(g1_inputs(ctx, 0, witnesses, count, pfmt, &W, bad));
    const size_t mark = ctx->lanes[0].arena_used;
    {  // hz, once: the scratch of the G2 sum goes back to the arena (the kernels of the call follow one another on the stream)
        Fr *zc = (Fr *)lane_alloc(ctx, 0, (k + 2) * 32);
        if (!zc) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        KZG_TRY(vcb_canon(ctx, st, pv.product, k + 1, 1, zc));
        KZG_TRY(g2_msm_bucket_device(ctx, hs, 0, zc, k + 1, hz));
        ctx->lanes[0].arena_used = mark;
    }
    for (size_t c = 0; c < count; c++) {
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(dr, (const uint8_t *)r_coeffs + c * k * 32, k * 32, hipMemcpyHostToDevice, st));
        MsmPoint *res = nullptr;
        KZG_TRY(msm_run(ctx, 0, gs, 0, dr, k, sfmt, &res));
        KZG_TRY(emit_point(ctx, 0, res, gr + c, KZG_G1_AFFINE_MONT_96));
        ctx->lanes[0].arena_used = mark;
    }
    KZG_LAUNCH(ctx, st, "k_vet_check", k_vet_check, (unsigned)((count + 63) / 64), 64, 0, (const G1Xyzz *)C, (const G1Affine *)gr, (const G1Xyzz *)W,
               (const G2Affine *)hz, (const G2Affine *)hs->pts, (const Fq2 *)hs->lines, count, d_ok);
    return fetch_ok(ctx, 0, d_ok, bad, count, ok);
}
