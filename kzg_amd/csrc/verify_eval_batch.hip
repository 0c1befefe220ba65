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
struct EvalParts {  // the extra outputs of kzg_test_verify_eval_batch_parts (host)
    void *yagg = nullptr, *cw = nullptr, *points = nullptr;
};

int veb_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt, const void *commitments,
            size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt, size_t count, const void *r, int *ok,
            const EvalParts *parts) {
    const char *who = "kzg_verify_eval_batch";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (!gs || !hs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL SRS");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / witnesses are affine (G1Affine)");
    if (gs->n < 1 || hs->n < 2) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + " needs gs[0], hs[0], hs[1]");
    if (gs->device != ctx->device || hs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
    if (!count) {
        if (ok) *ok = 1;
        return KZG_OK;
    }
    if (!xs || !ys || !commitments || !witnesses || !r || !ok) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL argument");
    Fr rm;
    KZG_TRY(load_challenge(ctx, who, r, sfmt, &rm));
    if (count > (SIZE_MAX >> 9) || n_commitments > (SIZE_MAX >> 9)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": count too large");
    const bool indexed = commitment_idx != nullptr;
    if (!indexed && n_commitments != count) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": without indices there is one commitment per opening");
    size_t chunk = VEB_CHUNK;
    if (ctx->opt_verify_eval_batch_chunk > 0) chunk = std::min(chunk, (size_t)ctx->opt_verify_eval_batch_chunk);
    const size_t B0 = std::min(chunk, count), BP = indexed ? std::min(chunk, std::max(count, n_commitments)) : B0;
    std::vector<uint32_t> cnt, which, start, order;  // the counting sort of a chunk's openings by commitment
    if (indexed) {
        for (size_t k = 0; k < count; k++)
            if (commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
        try {  // (no exception may leave through the C ABI)
            cnt.assign(n_commitments, 0);
            which.resize(B0);
            start.resize(B0 + 1);
            order.resize(B0);
        } catch (const std::bad_alloc &) {
            return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the indices");
        }
    }

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const int is_mont = sfmt == KZG_FR_MONT_LE_32 ? 1 : 0;
    const size_t fold_blocks = (B0 + VCB_FOLD_CELLS - 1) / VCB_FOLD_CELLS, bucket_bytes = 3 * (size_t)VCB_G * VCB_SET * sizeof(G1Xyzz);
    const size_t c_bytes = indexed ? std::max<size_t>(n_commitments, 1) * 32 : 32;
    KZG_TRY(lane_reserve(ctx, lane, bucket_bytes + sizeof(VcbSums) + c_bytes + (BP + (indexed ? 0 : B0)) * (psz + sizeof(G1Xyzz)) +
                                        B0 * (3 * 4 + 5 * 32) + (fold_blocks + 4) * 32 + 65536));
    struct Drain {  // nothing of the call is in flight once its host-side buffers go out of scope
        hipStream_t st;
        ~Drain() { hipStreamSynchronize(st); }
    } drain{st};
    int *bad = (int *)lane_alloc(ctx, lane, 256);
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, lane, 256);
    G1Affine *d_parts = (G1Affine *)lane_alloc(ctx, lane, 4 * sizeof(G1Affine));
    G1Xyzz *bk = (G1Xyzz *)lane_alloc(ctx, lane, bucket_bytes);
    VcbSums *sums = (VcbSums *)lane_alloc(ctx, lane, sizeof(VcbSums));
    Fr *d_yagg = (Fr *)lane_alloc(ctx, lane, 3 * 32), *d_part = (Fr *)lane_alloc(ctx, lane, fold_blocks * 32);  // yagg (sfmt), yagg, -yagg
    Fr *d_c = (Fr *)lane_alloc(ctx, lane, c_bytes);
    uint32_t *d_which = (uint32_t *)lane_alloc(ctx, lane, B0 * 4), *d_start = (uint32_t *)lane_alloc(ctx, lane, (B0 + 1) * 4);
    uint32_t *d_order = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    Fr *d_rho = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s1 = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s2 = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    Fr *d_x = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_y = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    uint8_t *raw = (uint8_t *)lane_alloc(ctx, lane, BP * psz);
    G1Xyzz *W = (G1Xyzz *)lane_alloc(ctx, lane, BP * sizeof(G1Xyzz));
    uint8_t *raw_c = indexed ? raw : (uint8_t *)lane_alloc(ctx, lane, B0 * psz);  // a chunk's commitments next to its witnesses
    G1Xyzz *Cm = indexed ? W : (G1Xyzz *)lane_alloc(ctx, lane, B0 * sizeof(G1Xyzz));
    if (!bad || !d_ok || !d_parts || !bk || !sums || !d_yagg || !d_part || !d_c || !d_which || !d_start || !d_order || !d_rho || !d_s1 || !d_s2 ||
        !d_x || !d_y || !raw || !W || !raw_c || !Cm)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    G1Xyzz *bk1 = bk, *bk2 = bk + (size_t)VCB_G * VCB_SET, *bk3 = bk + 2 * (size_t)VCB_G * VCB_SET;
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, bucket_bytes, st));         // zz = 0: the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, sizeof(VcbSums), st));    // the Ragg slot stays the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_yagg, 0, 3 * 32, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_c, 0, c_bytes, st));
    size_t slots = 1;  // slice slots any chunk has used (gs[0] takes slot 0)
    for (size_t k0 = 0; k0 < count; k0 += chunk) {
        const size_t B = std::min(chunk, count - k0);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_x, (const uint8_t *)xs + k0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_y, (const uint8_t *)ys + k0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)witnesses + k0 * psz, B * psz, hipMemcpyHostToDevice, st));
        KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
        KZG_TRY(powers_run(ctx, st, rm, k0, B, d_rho));
        KZG_LAUNCH(ctx, st, "k_veb_scalars", k_veb_scalars, vcb_grid(B), 256, 0, (const Fr *)d_rho, (const Fr *)d_x, B, is_mont, d_s1, d_s2);
        KZG_TRY(vcb_fold(ctx, st, d_y, d_rho, B, 0, d_part, d_yagg));
        KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s2, B, bk1, bk2, 2));
        if (indexed) {  // the chunk's openings listed per commitment, commitments in the order of their first opening
            size_t lists = 0;
            const uint32_t *cm = commitment_idx + k0;
            for (size_t k = 0; k < B; k++)
                if (!cnt[cm[k]]++) which[lists++] = cm[k];
            uint32_t at = 0;
            for (size_t g = 0; g < lists; g++) {
                start[g] = at;
                at += cnt[which[g]];
                cnt[which[g]] = start[g];
            }
            start[lists] = at;
            for (size_t k = 0; k < B; k++) order[cnt[cm[k]]++] = (uint32_t)k;
            for (size_t g = 0; g < lists; g++) cnt[which[g]] = 0;
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_which, which.data(), lists * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_start, start.data(), (lists + 1) * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_order, order.data(), B * 4, hipMemcpyHostToDevice, st));
            KZG_TRY(vcb_cweights(ctx, st, d_rho, d_which, d_start, d_order, lists, d_c));
        } else {  // c_k = rho_k: the chunk's commitments into the third set at once
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw_c, (const uint8_t *)commitments + k0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw_c, B, pfmt, Cm, bad, untrusted_level(ctx)));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)Cm, d_s1, d_s1, B, bk3, bk3, 1));
            if (parts) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)parts->cw + k0 * 32, d_s1, B * 32, hipMemcpyDeviceToHost, st));
        }
        slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        // the host lists and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (indexed) {  // Cagg: the commitments against the canonical c, in chunks like the openings
        for (size_t m0 = 0; m0 < n_commitments; m0 += BP) {
            const size_t B = std::min(BP, n_commitments - m0);
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)commitments + m0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
            KZG_TRY(vcb_canon(ctx, st, d_c + m0, B, 1, d_c + m0));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_c + m0, d_c + m0, B, bk3, bk3, 1));
            slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        }
        if (parts) KZG_HIP_CHECK(ctx, hipMemcpyAsync(parts->cw, d_c, n_commitments * 32, hipMemcpyDeviceToHost, st));
    }
    // - [yagg] gs[0]: one more pair of the third set (row 0 of the SRS table is gs itself)
    KZG_LAUNCH(ctx, st, "k_veb_yagg", k_veb_yagg, 1, 1, 0, (const Fr *)d_yagg, is_mont, d_yagg + 1, d_yagg + 2);
    KZG_TRY(vb_accumulate(ctx, st, (const G1Affine *)gs->table, d_yagg + 2, d_yagg + 2, 1, bk3, bk3, 1));
    KZG_TRY(vb_reduce(ctx, st, bk, (uint32_t)slots, sums));
    if (parts) KZG_HIP_CHECK(ctx, hipMemcpyAsync(parts->yagg, d_yagg + 1, 32, hipMemcpyDeviceToHost, st));
    return vcb_conclude(ctx, lane, sums, hs->pts, hs->lines, hs->h_pts, hs->h_lines, bad, d_ok, d_parts, parts ? parts->points : nullptr, ok);
}
// kzg_verify_fold: `groups` folded openings (kzg_open_fold_eval / kzg_open_fold_coeff), one verdict.  The equation of veb_run with two
// kinds of weights: the witness of group g carries r^g (and r^g z_g), value and commitment (g, i) carry rho_{g,i} = r^g gamma_g^i.  So
// the call runs veb_run's stages in two passes over its own chunks: the witnesses against r^g (k_powers, k_veb_scalars, the first two
// bucket sets), then the values and commitments against rho (formed on the host, one product per opening, and uploaded per chunk: the
// fold of yagg, and k_vcb_cweights or the third bucket set).  The end is veb_run's.  DESIGN.md section 3.4c.
int vf_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt, const void *commitments,
           size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt, size_t t, size_t groups, const void *gammas,
           const void *r, int *ok) {
    const char *who = "kzg_verify_fold";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (!gs || !hs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL SRS");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / witnesses are affine (G1Affine)");
    if (gs->n < 1 || hs->n < 2) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + " needs gs[0], hs[0], hs[1]");
    if (gs->device != ctx->device || hs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
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
    const bool indexed = commitment_idx != nullptr;
    if (!indexed && n_commitments != count) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": without indices there is one commitment per value");
    size_t chunk = VEB_CHUNK;
    if (ctx->opt_verify_eval_batch_chunk > 0) chunk = std::min(chunk, (size_t)ctx->opt_verify_eval_batch_chunk);
    const size_t B0 = std::min(chunk, count), BP = indexed ? std::min(chunk, std::max(count, n_commitments)) : B0;
    std::vector<uint32_t> cnt, which, start, order;  // the counting sort of a chunk's values by commitment
    std::vector<Fr> rho;                             // a chunk's weights
    if (indexed)
        for (size_t k = 0; k < count; k++)
            if (commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
    try {
        rho.resize(B0);
        if (indexed) {
            cnt.assign(n_commitments, 0);
            which.resize(B0);
            start.resize(B0 + 1);
            order.resize(B0);
        }
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the weights and indices");
    }

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const int is_mont = sfmt == KZG_FR_MONT_LE_32 ? 1 : 0;
    const size_t fold_blocks = (B0 + VCB_FOLD_CELLS - 1) / VCB_FOLD_CELLS, bucket_bytes = 3 * (size_t)VCB_G * VCB_SET * sizeof(G1Xyzz);
    const size_t c_bytes = indexed ? std::max<size_t>(n_commitments, 1) * 32 : 32;
    KZG_TRY(lane_reserve(ctx, lane, bucket_bytes + sizeof(VcbSums) + c_bytes + BP * (psz + sizeof(G1Xyzz)) + B0 * (3 * 4 + 5 * 32) + (fold_blocks + 4) * 32 + 65536));
    struct Drain {  // nothing of the call is in flight once its host-side buffers go out of scope
        hipStream_t st;
        ~Drain() { hipStreamSynchronize(st); }
    } drain{st};
    int *bad = (int *)lane_alloc(ctx, lane, 256);
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, lane, 256);
    G1Affine *d_parts = (G1Affine *)lane_alloc(ctx, lane, 4 * sizeof(G1Affine));
    G1Xyzz *bk = (G1Xyzz *)lane_alloc(ctx, lane, bucket_bytes);
    VcbSums *sums = (VcbSums *)lane_alloc(ctx, lane, sizeof(VcbSums));
    Fr *d_yagg = (Fr *)lane_alloc(ctx, lane, 3 * 32), *d_part = (Fr *)lane_alloc(ctx, lane, fold_blocks * 32);  // yagg (sfmt), yagg, -yagg
    Fr *d_c = (Fr *)lane_alloc(ctx, lane, c_bytes);
    uint32_t *d_which = (uint32_t *)lane_alloc(ctx, lane, B0 * 4), *d_start = (uint32_t *)lane_alloc(ctx, lane, (B0 + 1) * 4);
    uint32_t *d_order = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    Fr *d_rho = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s1 = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s2 = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    Fr *d_x = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_y = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    uint8_t *raw = (uint8_t *)lane_alloc(ctx, lane, BP * psz);
    G1Xyzz *W = (G1Xyzz *)lane_alloc(ctx, lane, BP * sizeof(G1Xyzz));
    if (!bad || !d_ok || !d_parts || !bk || !sums || !d_yagg || !d_part || !d_c || !d_which || !d_start || !d_order || !d_rho || !d_s1 || !d_s2 ||
        !d_x || !d_y || !raw || !W)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    G1Xyzz *bk1 = bk, *bk2 = bk + (size_t)VCB_G * VCB_SET, *bk3 = bk + 2 * (size_t)VCB_G * VCB_SET;
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, bucket_bytes, st));         // zz = 0: the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, sizeof(VcbSums), st));    // the Ragg slot stays the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_yagg, 0, 3 * 32, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_c, 0, c_bytes, st));
    size_t slots = 1;  // slice slots any chunk has used (gs[0] takes slot 0)
    // ---- the witnesses: P1 and P2 against r^g and r^g z_g ----
    for (size_t g0 = 0; g0 < groups; g0 += chunk) {
        const size_t B = std::min(chunk, groups - g0);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_x, (const uint8_t *)zs + g0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)witnesses + g0 * psz, B * psz, hipMemcpyHostToDevice, st));
        KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
        KZG_TRY(powers_run(ctx, st, rm, g0, B, d_rho));
        KZG_LAUNCH(ctx, st, "k_veb_scalars", k_veb_scalars, vcb_grid(B), 256, 0, (const Fr *)d_rho, (const Fr *)d_x, B, is_mont, d_s1, d_s2);
        KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s2, B, bk1, bk2, 2));
        slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    // ---- values and commitments against rho_{g,i} = r^g gamma_g^i; the weights walk (g, i) across the chunk boundaries ----
    size_t wg = 0, wi = 0;
    Fr rg = Fr::one(), w = Fr::one();  // r^wg, r^wg gamma_wg^wi
    for (size_t k0 = 0; k0 < count; k0 += chunk) {
        const size_t B = std::min(chunk, count - k0);
        for (size_t k = 0; k < B; k++) {
            rho[k] = w;
            if (++wi == t) {
                wi = 0;
                wg++;
                rg = mul(rg, rm);
                w = rg;
            } else {
                w = mul(w, gm[wg]);
            }
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_rho, rho.data(), B * 32, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_y, (const uint8_t *)ys + k0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_TRY(vcb_fold(ctx, st, d_y, d_rho, B, 0, d_part, d_yagg));
        if (indexed) {  // the chunk's values listed per commitment, commitments in the order of their first value
            size_t lists = 0;
            const uint32_t *cm = commitment_idx + k0;
            for (size_t k = 0; k < B; k++)
                if (!cnt[cm[k]]++) which[lists++] = cm[k];
            uint32_t at = 0;
            for (size_t g = 0; g < lists; g++) {
                start[g] = at;
                at += cnt[which[g]];
                cnt[which[g]] = start[g];
            }
            start[lists] = at;
            for (size_t k = 0; k < B; k++) order[cnt[cm[k]]++] = (uint32_t)k;
            for (size_t g = 0; g < lists; g++) cnt[which[g]] = 0;
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_which, which.data(), lists * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_start, start.data(), (lists + 1) * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_order, order.data(), B * 4, hipMemcpyHostToDevice, st));
            KZG_TRY(vcb_cweights(ctx, st, d_rho, d_which, d_start, d_order, lists, d_c));
        } else {  // c_k = rho_k: the chunk's commitments into the third set at once
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)commitments + k0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
            KZG_TRY(vcb_canon(ctx, st, d_rho, B, 1, d_s1));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s1, B, bk3, bk3, 1));
        }
        slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        // the host lists and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (indexed) {  // Cagg: the commitments against the canonical c, in chunks like the values
        for (size_t m0 = 0; m0 < n_commitments; m0 += BP) {
            const size_t B = std::min(BP, n_commitments - m0);
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)commitments + m0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
            KZG_TRY(vcb_canon(ctx, st, d_c + m0, B, 1, d_c + m0));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_c + m0, d_c + m0, B, bk3, bk3, 1));
            slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        }
    }
    // - [yagg] gs[0]: one more pair of the third set (row 0 of the SRS table is gs itself)
    KZG_LAUNCH(ctx, st, "k_veb_yagg", k_veb_yagg, 1, 1, 0, (const Fr *)d_yagg, is_mont, d_yagg + 1, d_yagg + 2);
    KZG_TRY(vb_accumulate(ctx, st, (const G1Affine *)gs->table, d_yagg + 2, d_yagg + 2, 1, bk3, bk3, 1));
    KZG_TRY(vb_reduce(ctx, st, bk, (uint32_t)slots, sums));
    return vcb_conclude(ctx, lane, sums, hs->pts, hs->lines, hs->h_pts, hs->h_lines, bad, d_ok, d_parts, nullptr, ok);
}
// kzg_verify_multiopen: N claims at any points answered by the two elements D and pi (kzg_multiopen_*_commit / _finish; DESIGN.md section
// 3.4d).  With w_k = r^k / (t - z_k): E = sum_m W_m C_m, W_m = sum_{m(k) = m} w_k, g2 = sum_k w_k y_k, and the proof is a plain opening of
// E - D at (t, g2) with the witness pi.  So this is vf_run with other weights: the ONE witness against 1 and t (k_veb_scalars), D as
// one more pair of the third set against -1, then the values and commitments against w_k, formed on the host per chunk (one inversion
// each, multiopen_plan.h): the fold gives g2, k_vcb_cweights or the third set gives E.  The end is veb_run's.
int vm_run(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt, const void *commitments,
           size_t n_commitments, const uint32_t *commitment_idx, size_t count, const void *r, const void *t, const void *d_point, const void *pi,
           int pfmt, int *ok) {
    const char *who = "kzg_verify_multiopen";
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (!gs || !hs) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL SRS");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / D / pi are affine (G1Affine)");
    if (gs->n < 1 || hs->n < 2) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + " needs gs[0], hs[0], hs[1]");
    if (gs->device != ctx->device || hs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the SRS is resident on another GPU than this context's");
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
    const bool indexed = commitment_idx != nullptr;
    if (!indexed && n_commitments != count) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": without indices there is one commitment per claim");
    size_t chunk = VEB_CHUNK;
    if (ctx->opt_verify_eval_batch_chunk > 0) chunk = std::min(chunk, (size_t)ctx->opt_verify_eval_batch_chunk);
    const size_t B0 = std::min(chunk, count), BP = indexed ? std::min(chunk, std::max(count, n_commitments)) : B0;
    std::vector<uint32_t> cnt, which, start, order;  // the counting sort of a chunk's claims by commitment
    std::vector<Fr> zm, w;                           // the points (Montgomery) | a chunk's weights
    try {  // (no exception may leave through the C ABI)
        zm.resize(count);
        w.resize(B0);
        if (indexed) {
            cnt.assign(n_commitments, 0);
            which.resize(B0);
            start.resize(B0 + 1);
            order.resize(B0);
        }
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the weights and indices");
    }
    for (size_t k = 0; k < count; k++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)zs + 32 * k, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a point z >= modulus");
        zm[k] = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
        if (zm[k] == tm) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t equals a point z_k (draw another t)");
        if (indexed && commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
    }
    const Fr one = Fr::one(), minus_one = from_mont(neg(Fr::one()));  // the witness's weight (Montgomery) | D's scalar (canonical)

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const int is_mont = sfmt == KZG_FR_MONT_LE_32 ? 1 : 0;
    const size_t fold_blocks = (B0 + VCB_FOLD_CELLS - 1) / VCB_FOLD_CELLS, bucket_bytes = 3 * (size_t)VCB_G * VCB_SET * sizeof(G1Xyzz);
    const size_t c_bytes = indexed ? std::max<size_t>(n_commitments, 1) * 32 : 32;
    KZG_TRY(lane_reserve(ctx, lane, bucket_bytes + sizeof(VcbSums) + c_bytes + BP * (psz + sizeof(G1Xyzz)) + B0 * (3 * 4 + 5 * 32) + (fold_blocks + 4) * 32 + 65536));
    struct Drain {  // nothing of the call is in flight once its host-side buffers go out of scope
        hipStream_t st;
        ~Drain() { hipStreamSynchronize(st); }
    } drain{st};
    int *bad = (int *)lane_alloc(ctx, lane, 256);
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, lane, 256);
    G1Affine *d_parts = (G1Affine *)lane_alloc(ctx, lane, 4 * sizeof(G1Affine));
    G1Xyzz *bk = (G1Xyzz *)lane_alloc(ctx, lane, bucket_bytes);
    VcbSums *sums = (VcbSums *)lane_alloc(ctx, lane, sizeof(VcbSums));
    Fr *d_yagg = (Fr *)lane_alloc(ctx, lane, 3 * 32), *d_part = (Fr *)lane_alloc(ctx, lane, fold_blocks * 32);  // g2 (sfmt), g2, -g2
    Fr *d_c = (Fr *)lane_alloc(ctx, lane, c_bytes);
    uint32_t *d_which = (uint32_t *)lane_alloc(ctx, lane, B0 * 4), *d_start = (uint32_t *)lane_alloc(ctx, lane, (B0 + 1) * 4);
    uint32_t *d_order = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    Fr *d_rho = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s1 = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_s2 = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    Fr *d_x = (Fr *)lane_alloc(ctx, lane, B0 * 32), *d_y = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    uint8_t *raw = (uint8_t *)lane_alloc(ctx, lane, BP * psz);
    G1Xyzz *W = (G1Xyzz *)lane_alloc(ctx, lane, BP * sizeof(G1Xyzz));
    if (!bad || !d_ok || !d_parts || !bk || !sums || !d_yagg || !d_part || !d_c || !d_which || !d_start || !d_order || !d_rho || !d_s1 || !d_s2 ||
        !d_x || !d_y || !raw || !W)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    G1Xyzz *bk1 = bk, *bk2 = bk + (size_t)VCB_G * VCB_SET, *bk3 = bk + 2 * (size_t)VCB_G * VCB_SET;
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, bucket_bytes, st));         // zz = 0: the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, sizeof(VcbSums), st));    // the Ragg slot stays the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_yagg, 0, 3 * 32, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_c, 0, c_bytes, st));
    size_t slots = 1;  // slice slots any chunk has used (gs[0], pi and D take slot 0)
    // ---- the witness: P1 = pi, P2 = t pi ----
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_rho, one.v, 32, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_x, t, 32, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, pi, psz, hipMemcpyHostToDevice, st));
    KZG_TRY(decode_points(ctx, st, raw, 1, pfmt, W, bad, untrusted_level(ctx)));
    KZG_LAUNCH(ctx, st, "k_veb_scalars", k_veb_scalars, 1, 256, 0, (const Fr *)d_rho, (const Fr *)d_x, (size_t)1, is_mont, d_s1, d_s2);
    KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s2, 1, bk1, bk2, 2));
    // ---- D: one more commitment, of weight -1 ----
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_s1, minus_one.v, 32, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, d_point, psz, hipMemcpyHostToDevice, st));
    KZG_TRY(decode_points(ctx, st, raw, 1, pfmt, W, bad, untrusted_level(ctx)));
    KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s1, 1, bk3, bk3, 1));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    // ---- values and commitments against w_k = r^k / (t - z_k); r^k walks across the chunk boundaries ----
    Fr rk = Fr::one();
    for (size_t k0 = 0; k0 < count; k0 += chunk) {
        const size_t B = std::min(chunk, count - k0);
        if (!mo_weights(zm.data() + k0, B, rm, tm, &rk, w.data())) return fail(ctx, KZG_ERR_INTERNAL, std::string(who) + ": t equals a point");
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_rho, w.data(), B * 32, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_y, (const uint8_t *)ys + k0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_TRY(vcb_fold(ctx, st, d_y, d_rho, B, 0, d_part, d_yagg));
        if (indexed) {  // the chunk's claims listed per commitment, commitments in the order of their first claim
            size_t lists = 0;
            const uint32_t *cm = commitment_idx + k0;
            for (size_t k = 0; k < B; k++)
                if (!cnt[cm[k]]++) which[lists++] = cm[k];
            uint32_t at = 0;
            for (size_t g = 0; g < lists; g++) {
                start[g] = at;
                at += cnt[which[g]];
                cnt[which[g]] = start[g];
            }
            start[lists] = at;
            for (size_t k = 0; k < B; k++) order[cnt[cm[k]]++] = (uint32_t)k;
            for (size_t g = 0; g < lists; g++) cnt[which[g]] = 0;
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_which, which.data(), lists * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_start, start.data(), (lists + 1) * 4, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_order, order.data(), B * 4, hipMemcpyHostToDevice, st));
            KZG_TRY(vcb_cweights(ctx, st, d_rho, d_which, d_start, d_order, lists, d_c));
        } else {  // W_k = w_k: the chunk's commitments into the third set at once
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)commitments + k0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
            KZG_TRY(vcb_canon(ctx, st, d_rho, B, 1, d_s1));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_s1, d_s1, B, bk3, bk3, 1));
        }
        slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        // the host lists and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (indexed) {  // E: the commitments against the canonical W, in chunks like the claims
        for (size_t m0 = 0; m0 < n_commitments; m0 += BP) {
            const size_t B = std::min(BP, n_commitments - m0);
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)commitments + m0 * psz, B * psz, hipMemcpyHostToDevice, st));
            KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
            KZG_TRY(vcb_canon(ctx, st, d_c + m0, B, 1, d_c + m0));
            KZG_TRY(vb_accumulate(ctx, st, (const G1Xyzz *)W, d_c + m0, d_c + m0, B, bk3, bk3, 1));
            slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        }
    }
    // - [g2] gs[0]: one more pair of the third set (row 0 of the SRS table is gs itself)
    KZG_LAUNCH(ctx, st, "k_veb_yagg", k_veb_yagg, 1, 1, 0, (const Fr *)d_yagg, is_mont, d_yagg + 1, d_yagg + 2);
    KZG_TRY(vb_accumulate(ctx, st, (const G1Affine *)gs->table, d_yagg + 2, d_yagg + 2, 1, bk3, bk3, 1));
    KZG_TRY(vb_reduce(ctx, st, bk, (uint32_t)slots, sums));
    return vcb_conclude(ctx, lane, sums, hs->pts, hs->lines, hs->h_pts, hs->h_lines, bad, d_ok, d_parts, nullptr, ok);
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
