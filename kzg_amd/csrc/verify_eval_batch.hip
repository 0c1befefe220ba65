// verify_eval_batch.hip -- kzg_verify_eval_batch: ONE verdict for any number of single-point openings, by a random linear combination
// of the per-opening equations of k_verify_eval (pairing.hip).  Not a reference method.
//
// Opening k: commitment index m_k, point x_k, value y_k, witness pi_k; weights rho_k = r^k over the whole call.
//   P1 = sum_k rho_k pi_k            P2 = sum_k (rho_k x_k) pi_k
//   c_m = sum_{k: m_k = m} rho_k     Cagg = sum_m c_m C_m            yagg = sum_k rho_k y_k
//   ok = [ e(P1, hs[1]) e(-(P2 + Cagg - [yagg] gs[0]), hs[0]) == 1 ]
// This is kzg_verify_cosets_batch at l = 1 with x_k read from the caller instead of taken from the domain, and every stage but one is
// that call's (vcb_shared.h).  Per chunk of B openings: the witnesses are decoded, rho = r^(k0 + k) (k_powers), then
//   k_veb_scalars   rho_k and rho_k x_k as canonical scalars (the one kernel of this file on the path)
//   k_vcb_fold / k_vcb_fold2 at l = 1   yagg += sum_k rho_k y_k, in a fixed order
//   k_vcb_bucket    bucket (slice-slot, window, |digit|) += +-pi_k for both scalar sets
// and the third bucket set: with one commitment per opening (commitment_idx == NULL) the chunk's commitments against rho in the same
// loop; with indices k_vcb_cweights per chunk and the commitments against c after the last chunk.  (gs[0], -yagg) rides as one more
// pair of the third set, so the set's total is Cagg - [yagg] gs[0] and the Ragg slot of the finish stays the identity.  Then
// k_vcb_reduce and the finish of vcb_finish.h, on the calling thread or in k_vcb_finish.  DESIGN.md section 3.5g.
//
// kzg_verify_fold (vf_run) and kzg_verify_multiopen (vm_run) are the same equation with other weights, and live here for that.  All
// three stand on the driver core of vcb_shared.h (workspace, points into buckets, commitment weights, the Cagg loop) and on what only
// they share, below: veb_front / veb_chunks (the shape checks and the chunk rule), veb_work, veb_witnesses, veb_weighted, veb_finish.
// What is left in a driver is its own mathematics: which points meet which scalars, in which pass.
#include <algorithm>
#include <vector>

#include "multiopen_plan.h"
#include "vcb_shared.h"

namespace kzg {

constexpr size_t VEB_CHUNK = (size_t)VCB_G * VCB_S;  // openings per chunk: what the slice slots of one bucket set hold

// s1[k] = rho_k, s2[k] = rho_k x_k, canonical and reduced; rho Montgomery, x in the caller's scalar format (any 256-bit value: the
// Montgomery product reduces it)
__global__ __launch_bounds__(256) void k_veb_scalars(const Fr *rho, const Fr *xs, size_t count, int is_mont, Fr *s1, Fr *s2) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const Fr p = rho[k], px = mul(p, xs[k]);  // Montgomery x canonical = canonical
    s1[k] = from_mont(p);
    s2[k] = is_mont ? from_mont(px) : px;
}

// one thread: yagg (the fold's sum, in the caller's scalar format) canonical, and -yagg canonical: the scalar of gs[0] in the third set
__global__ void k_veb_yagg(const Fr *y, int is_mont, Fr *yc, Fr *yn) {
    if (blockIdx.x || threadIdx.x) return;
    const Fr c = is_mont ? from_mont(y[0]) : mul(y[0], Fr::one());
    yc[0] = c;
    yn[0] = neg(c);
}

namespace {
// ---- what the three calls of this file share beyond the core of vcb_shared.h ----
// The first shape checks, in the name of `who`; `points` is what the call's encoded points are.  Nothing is touched.
int veb_front(kzg_ctx *ctx, const char *who, const char *points, const kzg_srs *gs, const kzg_srs_g2 *hs, int sfmt, int pfmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!gs || !hs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL SRS");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (!point_format_bytes(pfmt) || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, std::string(points) + " are affine (G1Affine)");
    if (gs->n < 1 || hs->n < 2) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + " needs gs[0], hs[0], hs[1]");
    if (gs->device != ctx->device || hs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    return KZG_OK;
}

struct VebChunks {
    bool indexed;
    size_t chunk, B0, BP;  // openings per chunk | of the largest chunk | points the largest step decodes at once
};
// one commitment per `word` unless the call has indices, then the chunk rule (option verify_eval_batch_chunk lowers VEB_CHUNK)
int veb_chunks(kzg_ctx *ctx, const char *who, const char *word, size_t count, size_t n_commitments, const uint32_t *commitment_idx, VebChunks *c) {
    c->indexed = commitment_idx != nullptr;
    if (!c->indexed && n_commitments != count) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": without indices there is one commitment per " + word);
    c->chunk = VEB_CHUNK;
    if (ctx->opt_verify_eval_batch_chunk > 0) c->chunk = std::min(c->chunk, (size_t)ctx->opt_verify_eval_batch_chunk);
    c->B0 = std::min(c->chunk, count);
    c->BP = c->indexed ? std::min(c->chunk, std::max(count, n_commitments)) : c->B0;
    return KZG_OK;
}
int veb_indices(kzg_ctx *ctx, const char *who, const uint32_t *commitment_idx, size_t count, size_t n_commitments) {
    for (size_t k = 0; k < count; k++)
        if (commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
    return KZG_OK;
}

struct VebWork : VcbWork {
    int is_mont;
    Fr *d_x, *d_y;  // a chunk's points and values, in the caller's scalar format
    Fr *d_yagg;     // yagg (sfmt), yagg, -yagg (canonical)
    Fr *d_part;     // the fold's scratch
};
int veb_work(kzg_ctx *ctx, int lane, int sfmt, int pfmt, const VebChunks &c, size_t n_commitments, VebWork *w) {
    const size_t fold_blocks = (c.B0 + VCB_FOLD_CELLS - 1) / VCB_FOLD_CELLS;
    // gs[0] takes slice slot 0 in the end (and so do the single points of kzg_verify_multiopen)
    KZG_TRY(vcb_work(ctx, lane, pfmt, c.B0, c.BP, c.indexed ? std::max<size_t>(n_commitments, 1) : 1, c.B0 * 2 * 32 + (fold_blocks + 4) * 32, 1, w));
    w->is_mont = sfmt == KZG_FR_MONT_LE_32 ? 1 : 0;
    w->d_yagg = (Fr *)lane_alloc(ctx, lane, 3 * 32);
    w->d_part = (Fr *)lane_alloc(ctx, lane, fold_blocks * 32);
    w->d_x = (Fr *)lane_alloc(ctx, lane, c.B0 * 32);
    w->d_y = (Fr *)lane_alloc(ctx, lane, c.B0 * 32);
    if (!w->d_yagg || !w->d_part || !w->d_x || !w->d_y) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(w->sums, 0, sizeof(VcbSums), w->st));  // the Ragg slot stays the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(w->d_yagg, 0, 3 * 32, w->st));
    return KZG_OK;
}

// Witnesses k0 .. k0 + B of the call against r^k and r^k x_k: P1 and P2.  Leaves rho in w->d_rho and rho canonical in w->d_s1.
int veb_witnesses(VebWork *w, const Fr &rm, const void *xs, const void *witnesses, size_t k0, size_t B) {
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_x, (const uint8_t *)xs + k0 * 32, B * 32, hipMemcpyHostToDevice, w->st));
    KZG_TRY(powers_run(w->ctx, w->st, rm, k0, B, w->d_rho));
    KZG_LAUNCH(w->ctx, w->st, "k_veb_scalars", k_veb_scalars, vcb_grid(B), 256, 0, (const Fr *)w->d_rho, (const Fr *)w->d_x, B, w->is_mont, w->d_s1, w->d_s2);
    return vcb_points(w, (const uint8_t *)witnesses + k0 * w->psz, B, w->d_s1, w->d_s2, w->bk[0], w->bk[1], 2);
}

// Values k0 .. k0 + B of the call and their commitments against the chunk's weights rho, formed on the host (Montgomery): yagg +=
// sum_k rho_k y_k, and c += the weights per commitment or, one commitment per value (commitment_idx null: c_k = rho_k), the chunk's
// commitments into the third set at once
int veb_weighted(VebWork *w, VcbLists *lists, const Fr *rho, const void *ys, const uint32_t *commitment_idx, const void *commitments, size_t k0,
                 size_t B) {
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_rho, rho, B * 32, hipMemcpyHostToDevice, w->st));
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_y, (const uint8_t *)ys + k0 * 32, B * 32, hipMemcpyHostToDevice, w->st));
    KZG_TRY(vcb_fold(w->ctx, w->st, w->d_y, w->d_rho, B, 0, w->d_part, w->d_yagg));
    if (commitment_idx) return vcb_commit_weights(w, lists, commitment_idx + k0, B);
    KZG_TRY(vcb_canon(w->ctx, w->st, w->d_rho, B, 1, w->d_s1));
    return vcb_points(w, (const uint8_t *)commitments + k0 * w->psz, B, w->d_s1, w->d_s1, w->bk[2], w->bk[2], 1);
}

// The end: - [yagg] gs[0] as one more pair of the third set (row 0 of the SRS table is gs itself), the reduction, the pairing check.
// out_yagg, out_points (may be null): the outputs of kzg_test_verify_eval_batch_parts.
int veb_finish(VebWork *w, const kzg_srs *gs, const kzg_srs_g2 *hs, void *out_yagg, void *out_points, int *ok) {
    KZG_LAUNCH(w->ctx, w->st, "k_veb_yagg", k_veb_yagg, 1, 1, 0, (const Fr *)w->d_yagg, w->is_mont, w->d_yagg + 1, w->d_yagg + 2);
    KZG_TRY(vb_accumulate(w->ctx, w->st, (const G1Affine *)gs->table, w->d_yagg + 2, w->d_yagg + 2, 1, w->bk[2], w->bk[2], 1));
    KZG_TRY(vb_reduce(w->ctx, w->st, w->bk[0], (uint32_t)w->slots, w->sums));
    if (out_yagg) KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(out_yagg, w->d_yagg + 1, 32, hipMemcpyDeviceToHost, w->st));
    return vcb_conclude(w->ctx, w->lane, w->sums, hs->pts, hs->lines, hs->h_pts, hs->h_lines, w->bad, w->d_ok, w->d_parts, out_points, ok);
}

struct EvalParts {  // the extra outputs of kzg_test_verify_eval_batch_parts (host)
    void *yagg = nullptr, *cw = nullptr, *points = nullptr;
};

int veb_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt, const void *commitments,
            size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt, size_t count, const void *r, int *ok,
            const EvalParts *parts) {
    const char *who = "kzg_verify_eval_batch";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    KZG_TRY(veb_front(ctx, who, "commitments / witnesses", gs, hs, sfmt, pfmt));
    if (!count) {
        if (ok) *ok = 1;
        return KZG_OK;
    }
    if (!xs || !ys || !commitments || !witnesses || !r || !ok) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL argument");
    Fr rm;
    KZG_TRY(load_challenge(ctx, who, r, sfmt, &rm));
    if (count > (SIZE_MAX >> 9) || n_commitments > (SIZE_MAX >> 9)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": count too large");
    VebChunks c;
    KZG_TRY(veb_chunks(ctx, who, "opening", count, n_commitments, commitment_idx, &c));
    VcbLists lists;
    if (c.indexed) {
        KZG_TRY(veb_indices(ctx, who, commitment_idx, count, n_commitments));
        if (!lists.reserve(n_commitments, c.B0)) return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the indices");
    }

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[ls.lane].stream;
    StreamDrain drain{st};
    VebWork w;
    KZG_TRY(veb_work(ctx, ls.lane, sfmt, pfmt, c, n_commitments, &w));
    for (size_t k0 = 0; k0 < count; k0 += c.chunk) {
        const size_t B = std::min(c.chunk, count - k0);
        KZG_TRY(veb_witnesses(&w, rm, xs, witnesses, k0, B));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(w.d_y, (const uint8_t *)ys + k0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_TRY(vcb_fold(ctx, st, w.d_y, w.d_rho, B, 0, w.d_part, w.d_yagg));
        if (c.indexed) {
            KZG_TRY(vcb_commit_weights(&w, &lists, commitment_idx + k0, B));
        } else {  // c_k = rho_k: the chunk's commitments into the third set at once
            KZG_TRY(vcb_points(&w, (const uint8_t *)commitments + k0 * w.psz, B, w.d_s1, w.d_s1, w.bk[2], w.bk[2], 1));
            if (parts) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)parts->cw + k0 * 32, w.d_s1, B * 32, hipMemcpyDeviceToHost, st));
        }
        // the host lists and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (c.indexed) {
        KZG_TRY(vcb_cagg(&w, commitments, n_commitments));
        if (parts) KZG_HIP_CHECK(ctx, hipMemcpyAsync(parts->cw, w.d_c, n_commitments * 32, hipMemcpyDeviceToHost, st));
    }
    return veb_finish(&w, gs, hs, parts ? parts->yagg : nullptr, parts ? parts->points : nullptr, ok);
}

// kzg_verify_fold: `groups` folded openings (kzg_open_fold_eval / kzg_open_fold_coeff), one verdict.  The equation of veb_run with two
// kinds of weights: the witness of group g carries r^g (and r^g z_g), value and commitment (g, i) carry rho_{g,i} = r^g gamma_g^i.  So
// the call runs in two passes over its own chunks: the witnesses against r^g (veb_witnesses), then the values and commitments against
// rho, formed on the host (fold_weights of vcb_host.h, one product per value) and uploaded per chunk (veb_weighted).  DESIGN.md
// section 3.4c.
int vf_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt, const void *commitments,
           size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt, size_t t, size_t groups, const void *gammas,
           const void *r, int *ok) {
    const char *who = "kzg_verify_fold";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    KZG_TRY(veb_front(ctx, who, "commitments / witnesses", gs, hs, sfmt, pfmt));
    if (t == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t == 0");
    if (!groups) {
        if (ok) *ok = 1;
        return KZG_OK;
    }
    if (!zs || !ys || !commitments || !witnesses || !gammas || !ok || (!r && groups > 1)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL argument");
    if (groups > (SIZE_MAX >> 9) || t > (SIZE_MAX >> 9) / groups || n_commitments > (SIZE_MAX >> 9))
        return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": groups x t too large");
    const size_t count = groups * t;
    Fr rm = Fr::one();
    if (r) {
        KZG_TRY(load_challenge(ctx, who, r, sfmt, &rm));
    }
    std::vector<Fr> gm;
    try {  // (no exception may leave through the C ABI)
        gm.resize(groups);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the challenges");
    }
    for (size_t g = 0; g < groups; g++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)gammas + 32 * g, 32);
        if (!is_canonical(x) || x.is_zero()) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a challenge gamma must be in [1, modulus)");
        gm[g] = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
        memcpy(x.v, (const uint8_t *)zs + 32 * g, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a point z >= modulus");
    }
    VebChunks c;
    KZG_TRY(veb_chunks(ctx, who, "value", count, n_commitments, commitment_idx, &c));
    if (c.indexed) KZG_TRY(veb_indices(ctx, who, commitment_idx, count, n_commitments));
    VcbLists lists;
    std::vector<Fr> rho;  // a chunk's weights
    bool room = !c.indexed || lists.reserve(n_commitments, c.B0);
    try {
        rho.resize(c.B0);
    } catch (const std::bad_alloc &) {
        room = false;
    }
    if (!room) return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the weights and indices");

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[ls.lane].stream;
    StreamDrain drain{st};
    VebWork w;
    KZG_TRY(veb_work(ctx, ls.lane, sfmt, pfmt, c, n_commitments, &w));
    // ---- the witnesses: P1 and P2 against r^g and r^g z_g ----
    for (size_t g0 = 0; g0 < groups; g0 += c.chunk) {
        const size_t B = std::min(c.chunk, groups - g0);
        KZG_TRY(veb_witnesses(&w, rm, zs, witnesses, g0, B));
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    // ---- values and commitments against rho_{g,i} = r^g gamma_g^i; the weights walk (g, i) across the chunk boundaries ----
    FoldWalk walk;
    for (size_t k0 = 0; k0 < count; k0 += c.chunk) {
        const size_t B = std::min(c.chunk, count - k0);
        fold_weights(&walk, t, rm, gm.data(), B, rho.data());
        KZG_TRY(veb_weighted(&w, &lists, rho.data(), ys, commitment_idx, commitments, k0, B));
        // the host lists and weights and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (c.indexed) KZG_TRY(vcb_cagg(&w, commitments, n_commitments));
    return veb_finish(&w, gs, hs, nullptr, nullptr, ok);
}

// kzg_verify_multiopen: N claims at any points answered by the two elements D and pi (kzg_multiopen_*_commit / _finish; DESIGN.md section
// 3.4d).  With w_k = r^k / (t - z_k): E = sum_m W_m C_m, W_m = sum_{m(k) = m} w_k, g2 = sum_k w_k y_k, and the proof is a plain opening of
// E - D at (t, g2) with the witness pi.  So: the ONE witness against 1 and t (k_veb_scalars), D as one more pair of the third set
// against -1, then the values and commitments against w_k, formed on the host per chunk (one inversion each, multiopen_plan.h) and
// uploaded (veb_weighted): the fold gives g2, k_vcb_cweights or the third set gives E.
int vm_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt, const void *commitments,
           size_t n_commitments, const uint32_t *commitment_idx, size_t count, const void *r, const void *t, const void *d_point, const void *pi,
           int pfmt, int *ok) {
    const char *who = "kzg_verify_multiopen";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    KZG_TRY(veb_front(ctx, who, "commitments / D / pi", gs, hs, sfmt, pfmt));
    if (!count) {
        if (ok) *ok = 1;
        return KZG_OK;
    }
    if (!zs || !ys || !commitments || !r || !t || !d_point || !pi || !ok) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL argument");
    if (count > (SIZE_MAX >> 9) || n_commitments > (SIZE_MAX >> 9)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": count too large");
    Fr rm, tm;
    KZG_TRY(load_challenge(ctx, who, r, sfmt, &rm));
    memcpy(tm.v, t, 32);
    if (!is_canonical(tm)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": the challenge t >= modulus");
    if (sfmt != KZG_FR_MONT_LE_32) tm = to_mont(tm);
    VebChunks c;
    KZG_TRY(veb_chunks(ctx, who, "claim", count, n_commitments, commitment_idx, &c));
    VcbLists lists;
    std::vector<Fr> zm, wt;  // the points (Montgomery) | a chunk's weights
    bool room = !c.indexed || lists.reserve(n_commitments, c.B0);
    try {  // (no exception may leave through the C ABI)
        zm.resize(count);
        wt.resize(c.B0);
    } catch (const std::bad_alloc &) {
        room = false;
    }
    if (!room) return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the weights and indices");
    for (size_t k = 0; k < count; k++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)zs + 32 * k, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a point z >= modulus");
        zm[k] = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
        if (zm[k] == tm) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t equals a point z_k (draw another t)");
        if (c.indexed && commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
    }
    const Fr one = Fr::one(), minus_one = from_mont(neg(Fr::one()));  // the witness's weight (Montgomery) | D's scalar (canonical)

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[ls.lane].stream;
    StreamDrain drain{st};
    VebWork w;
    KZG_TRY(veb_work(ctx, ls.lane, sfmt, pfmt, c, n_commitments, &w));
    // ---- the witness: P1 = pi, P2 = t pi ----
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(w.d_rho, one.v, 32, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(w.d_x, t, 32, hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_veb_scalars", k_veb_scalars, 1, 256, 0, (const Fr *)w.d_rho, (const Fr *)w.d_x, (size_t)1, w.is_mont, w.d_s1, w.d_s2);
    KZG_TRY(vcb_points(&w, pi, 1, w.d_s1, w.d_s2, w.bk[0], w.bk[1], 2));
    // ---- D: one more commitment, of weight -1 ----
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(w.d_s1, minus_one.v, 32, hipMemcpyHostToDevice, st));
    KZG_TRY(vcb_points(&w, d_point, 1, w.d_s1, w.d_s1, w.bk[2], w.bk[2], 1));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    // ---- values and commitments against w_k = r^k / (t - z_k); r^k walks across the chunk boundaries ----
    Fr rk = Fr::one();
    for (size_t k0 = 0; k0 < count; k0 += c.chunk) {
        const size_t B = std::min(c.chunk, count - k0);
        if (!mo_weights(zm.data() + k0, B, rm, tm, &rk, wt.data())) return fail(ctx, KZG_ERR_INTERNAL, std::string(who) + ": t equals a point");
        KZG_TRY(veb_weighted(&w, &lists, wt.data(), ys, commitment_idx, commitments, k0, B));
        // the host lists and weights and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (c.indexed) KZG_TRY(vcb_cagg(&w, commitments, n_commitments));
    return veb_finish(&w, gs, hs, nullptr, nullptr, ok);
}
}  // namespace

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_verify_multiopen(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt,
                                    const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, size_t count, const void *r,
                                    const void *t, const void *d_point, const void *pi, int pfmt, int *ok) {
    return vm_run(ctx, gs, hs, zs, ys, sfmt, commitments, n_commitments, commitment_idx, count, r, t, d_point, pi, pfmt, ok);
}

extern "C" int kzg_verify_fold(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt,
                               const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt,
                               size_t t, size_t groups, const void *gammas, const void *r, int *ok) {
    return vf_run(ctx, gs, hs, zs, ys, sfmt, commitments, n_commitments, commitment_idx, witnesses, pfmt, t, groups, gammas, r, ok);
}

extern "C" int kzg_verify_eval_batch(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt,
                                     const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses,
                                     int pfmt, size_t count, const void *r, int *ok) {
    return veb_run(ctx, gs, hs, xs, ys, sfmt, commitments, n_commitments, commitment_idx, witnesses, pfmt, count, r, ok, nullptr);
}

#ifdef KZG_TEST_HOOKS
#include "../../include/kzg_mi355x_test.h"
extern "C" int kzg_test_verify_eval_batch_parts(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt,
                                                const void *commitments, size_t n_commitments, const uint32_t *commitment_idx,
                                                const void *witnesses, int pfmt, size_t count, const void *r, int *ok, void *out_yagg,
                                                void *out_cw, void *out_points) {
    if (!out_yagg || !out_cw || !out_points || !count) return KZG_ERR_SHAPE;
    EvalParts parts;
    parts.yagg = out_yagg;
    parts.cw = out_cw;
    parts.points = out_points;
    return veb_run(ctx, gs, hs, xs, ys, sfmt, commitments, n_commitments, commitment_idx, witnesses, pfmt, count, r, ok, &parts);
}
#endif
