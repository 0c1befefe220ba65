// g2_msm.hip -- kzg_msm_g2_bucket: a G2 multi-exponentiation by the bucket method, for the n the verifier of a batched opening past
// 16,384 points needs (hz = [Z(tau)]_2, k + 1 terms).  kzg_msm_g2 (pairing.hip) spends a 255-bit double-and-add per term and sums
// the terms in one workgroup; here a term costs 32 mixed additions and the rest does not grow with n.  The shape is the one of the
// G1 variable-base sum (k_vcb_bucket / k_vcb_reduce, verify_cosets_batch.hip), on the Fq2 arithmetic of tower.h:
//   k_vcb_canon     the scalars canonical and reduced (any scalar >= r counts as its residue BEFORE the digits are taken: the top
//                   window of a value below r < 2^255 is at most 127 + 1, so no carry leaves it)
//   k_g2b_bucket    workgroup (slice, window): the window's signed 8-bit digit (vc_digit) of the slice's <= S scalars, a counting
//                   sort of the point indices by |digit| in LDS, then thread b walks the list of bucket b + 1 with g2_madd into the
//                   bucket it owns: arena[slot][window][b], slot = the slice's index inside its chunk.  No atomics on points.
//   k_g2b_reduce    workgroup (window): thread b folds the slots of bucket b + 1, then sum_b (b + 1) B_b by a suffix scan and a tree
//                   sum in LDS (7 rounds each)
//   k_g2b_finish    one thread: the Horner chain over the 32 window sums (31 x 8 doublings, 31 additions), affine on the device
// The arena has G slice slots (option "g2_msm_slots", default 16) of 32 x 128 Jacobian buckets of 288 B: 18.9 MB at the default,
// whatever n is; chunk after chunk of G x S points (option "g2_msm_slice": S, default 2048) adds into it.  Beside it the workspace
// holds the staged canonical scalars, 32 B per term.  DESIGN.md section 3.6b.
#include "vcb_shared.h"

namespace kzg {

constexpr uint32_t G2B_S = 2048;   // default and largest slice: 16-bit sorted entries, the sign in bit 15
constexpr uint32_t G2B_G = 16;     // default and largest number of slice slots
constexpr size_t G2B_SET = (size_t)VC_W * VC_D;  // buckets of one slot: 32 windows x 128
static_assert(G2B_S <= 32768, "the sorted entries keep the sign in bit 15");

// n <= slots x S points of one chunk; the grid has ceil(n / S) slices, so p0 < n.  sc: canonical, reduced.
__global__ __launch_bounds__(128) void k_g2b_bucket(const G2Affine *pts, const Fr *sc, size_t n, uint32_t S, G2Jacobian *bk) {
    __shared__ uint32_t cnt[VC_D], cur[VC_D];
    __shared__ uint16_t dig[G2B_S], ent[G2B_S];
    const uint32_t t = threadIdx.x, slot = blockIdx.x, win = blockIdx.y;
    bk += ((size_t)slot * VC_W + win) * VC_D;
    const size_t p0 = (size_t)slot * S;
    const uint32_t m = (uint32_t)(n - p0 < S ? n - p0 : S);
    cnt[t] = 0;
    __syncthreads();
    for (uint32_t p = t; p < m; p += 128) {
        const int d = vc_digit(sc[p0 + p].v, (int)win);
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);  // <= 128
        dig[p] = (uint16_t)(mag | (d < 0 ? 0x8000u : 0u));
        if (mag) atomicAdd(&cnt[mag - 1], 1u);
    }
    __syncthreads();
    uint32_t first = 0;
    for (uint32_t b = 0; b < t; b++) first += cnt[b];
    cur[t] = first;
    __syncthreads();
    for (uint32_t p = t; p < m; p += 128) {
        const uint32_t d = dig[p], mag = d & 0x7fffu;
        if (mag) ent[atomicAdd(&cur[mag - 1], 1u)] = (uint16_t)(p | (d & 0x8000u));  // a place below the slice's count of non-zero digits
    }
    __syncthreads();
    const uint32_t len = cnt[t];
    if (!len) return;
    G2Jacobian acc = bk[t];
    for (uint32_t e = first; e < first + len; e++) {
        const uint32_t x = ent[e];
        G2Affine p = pts[p0 + (x & 0x7fffu)];
        if (x & 0x8000u) f2_neg(p.y, p.y);
        g2_madd(acc, acc, p);
    }
    bk[t] = acc;
}

// Workgroup (window): out[window] = sum_b (b + 1) sum_{g < slots} bk[g][window][b]
__global__ __launch_bounds__(128) void k_g2b_reduce(const G2Jacobian *bk, uint32_t slots, G2Jacobian *out) {
    __shared__ G2Jacobian sh[VC_D];
    const uint32_t t = threadIdx.x, win = blockIdx.x;
    const G2Jacobian *b = bk + (size_t)win * VC_D + t;
    G2Jacobian acc = b[0], o;
    for (uint32_t g = 1; g < slots; g++) {
        o = b[(size_t)g * G2B_SET];
        g2_add(acc, acc, o);
    }
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = 1; s < VC_D; s <<= 1) {  // suffix sums: sh[t] = sum_{u >= t} B_u
        const bool on = t + s < VC_D;
        if (on) o = sh[t + s];
        __syncthreads();
        if (on) {
            g2_add(acc, acc, o);
            sh[t] = acc;
        }
        __syncthreads();
    }
    for (uint32_t s = VC_D / 2; s >= 1; s >>= 1) {
        if (t < s) {
            o = sh[t + s];
            g2_add(acc, acc, o);
            sh[t] = acc;
        }
        __syncthreads();
    }
    if (t == 0) out[win] = acc;
}

// sum_w 2^(8 w) win[w], affine
__global__ __launch_bounds__(64) void k_g2b_finish(const G2Jacobian *win, G2Affine *out) {
    if (blockIdx.x || threadIdx.x) return;
    G2Jacobian acc = win[VC_W - 1], o;
    for (int w = VC_W - 2; w >= 0; w--) {
        for (int i = 0; i < VC_C; i++) g2_dbl(acc, acc);
        o = win[w];
        g2_add(acc, acc, o);
    }
    G2Affine a;
    g2_to_affine(a, acc);
    *out = a;
}

size_t g2_msm_bucket_workspace_bytes(const kzg_ctx *ctx) {
    const size_t slots = ctx->opt_g2_msm_slots ? (size_t)ctx->opt_g2_msm_slots : G2B_G;
    return align_up(slots * G2B_SET * sizeof(G2Jacobian), 256) + align_up(VC_W * sizeof(G2Jacobian), 256);
}

// sum_i d_sc[i] srs[offset + i] -> d_out (affine) on lane 0's stream; d_sc canonical and reduced; the arena comes from lane 0
// (g2_msm_bucket_workspace_bytes)
int g2_msm_bucket_device(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, const Fr *d_sc, size_t n, G2Affine *d_out) {
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the G2 points are resident on another GPU than this context's");
    hipStream_t st = ctx->lanes[0].stream;
    const uint32_t S = ctx->opt_g2_msm_slice ? (uint32_t)ctx->opt_g2_msm_slice : G2B_S;
    const size_t slots = ctx->opt_g2_msm_slots ? (size_t)ctx->opt_g2_msm_slots : G2B_G, CH = slots * S;
    G2Jacobian *bk = (G2Jacobian *)lane_alloc(ctx, 0, slots * G2B_SET * sizeof(G2Jacobian));
    G2Jacobian *win = (G2Jacobian *)lane_alloc(ctx, 0, VC_W * sizeof(G2Jacobian));
    if (!bk || !win) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, slots * G2B_SET * sizeof(G2Jacobian), st));  // Z = 0: the identity
    size_t used = 1;
    for (size_t i0 = 0; i0 < n; i0 += CH) {
        const size_t B = std::min(CH, n - i0), slices = (B + S - 1) / S;
        KZG_LAUNCH(ctx, st, "k_g2b_bucket", k_g2b_bucket, dim3((unsigned)slices, VC_W), 128, 0, srs->pts + offset + i0, d_sc + i0, B, S, bk);
        used = std::max(used, slices);
    }
    KZG_LAUNCH(ctx, st, "k_g2b_reduce", k_g2b_reduce, VC_W, 128, 0, (const G2Jacobian *)bk, (uint32_t)used, win);
    KZG_LAUNCH(ctx, st, "k_g2b_finish", k_g2b_finish, 1, 64, 0, (const G2Jacobian *)win, d_out);
    return KZG_OK;
}

#ifdef KZG_TEST_HOOKS
__global__ __launch_bounds__(64) void k_test_g2_madd(const G2Jacobian *acc, const G2Affine *pts, size_t n, G2Affine *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G2Jacobian a = acc[i];
    G2Affine p = pts[i], r;
    g2_madd(a, a, p);
    g2_to_affine(r, a);
    out[i] = r;
}
#endif

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_msm_g2_bucket(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, const void *scalars, size_t n, int sfmt, int flags,
                                 void *out, int ofmt) {
    if (!ctx || !srs || !out || (!scalars && n)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = g2_point_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G2 point format");
    if (n > srs->n || offset > srs->n - n) return fail(ctx, KZG_ERR_SHAPE, "MSM range exceeds the SRS (reference: slice index panic)");
    if (srs->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the G2 points are resident on another GPU than this context's");
    KZG_TRY(lane_reserve(ctx, 0, align_up(n * 32 + 32, 256) + g2_msm_bucket_workspace_bytes(ctx) + 8192));
    hipStream_t st = ctx->lanes[0].stream;
    Fr *ds = (Fr *)lane_alloc(ctx, 0, n * 32 + 32);
    G2Affine *res = (G2Affine *)lane_alloc(ctx, 0, sizeof(G2Affine));
    uint8_t *enc = (uint8_t *)lane_alloc(ctx, 0, 512);
    if (!ds || !res || !enc) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const Fr *src = (const Fr *)scalars;
    if (n && !(flags & KZG_IN_DEVICE)) {
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(ds, scalars, n * 32, hipMemcpyHostToDevice, st));
        src = ds;
    }
    KZG_TRY(vcb_canon(ctx, st, src, n, sfmt == KZG_FR_MONT_LE_32 ? 1 : 0, ds));
    KZG_TRY(g2_msm_bucket_device(ctx, srs, offset, ds, n, res));
    KZG_TRY(g2_encode_run(ctx, st, res, 1, ofmt, enc));
    KZG_TRY(lane_pinned(ctx, 0, 4096));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(ctx->lanes[0].pinned, enc, psz, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    memcpy(out, ctx->lanes[0].pinned, psz);
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

#ifdef KZG_TEST_HOOKS
// out[i] = acc[i] + pts[i] through g2_madd, one thread per record: acc Jacobian Montgomery 288 B (any Z; Z = 0 the identity), pts and
// out affine Montgomery 192 B (all zero the identity)
extern "C" int kzg_test_g2_madd(kzg_ctx *ctx, const void *acc_jacobian, const void *pts_affine, size_t n, void *out_affine) {
    if (!ctx || !acc_jacobian || !pts_affine || !out_affine || !n || n > 4096) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(lane_reserve(ctx, 0, n * (sizeof(G2Jacobian) + 2 * sizeof(G2Affine)) + 8192));
    hipStream_t st = ctx->lanes[0].stream;
    G2Jacobian *da = (G2Jacobian *)lane_alloc(ctx, 0, n * sizeof(G2Jacobian));
    G2Affine *dp = (G2Affine *)lane_alloc(ctx, 0, n * sizeof(G2Affine)), *dout = (G2Affine *)lane_alloc(ctx, 0, n * sizeof(G2Affine));
    if (!da || !dp || !dout) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(da, acc_jacobian, n * sizeof(G2Jacobian), hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dp, pts_affine, n * sizeof(G2Affine), hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_test_g2_madd", k_test_g2_madd, (unsigned)((n + 63) / 64), 64, 0, (const G2Jacobian *)da, (const G2Affine *)dp, n, dout);
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out_affine, dout, n * sizeof(G2Affine), hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}
#endif
