// verify_cosets_batch.hip -- kzg_verify_cosets_batch: ONE verdict for any number of coset openings, by a random linear combination
// of the per-cell equations of verify_cosets.hip.  Not a reference method.  Notation as there: N = 2^log_n, l = 2^log_l, K = N / l.
//
// Cell k: commitment index m_k, coset i_k, interpolant r_k, proof pi_k, h_k = w^(i_k l); weights rho_k = r^k over the whole call.
//   a_j = sum_k rho_k r_{k,j}        Ragg = sum_j a_j gs[j]        c_m = sum_{k: m_k = m} rho_k        Cagg = sum_m c_m C_m
//   P1 = sum_k rho_k pi_k            P2 = sum_k (rho_k h_k) pi_k
//   ok = [ e(P1, hs[l]) e(-(P2 + Cagg - Ragg), hs[0]) == 1 ]
// Per chunk of B cells: the proofs are decoded, rho = r^(k0 + k) (k_powers), the interpolants (k_vc_interp), then
//   k_vcb_scalars   rho_k and rho_k h_k as canonical scalars
//   k_vcb_fold / k_vcb_fold2   a_j += sum_k rho_k r_{k,j}: partial sums per 64 cells, then one thread per j adds them in order
//   k_vcb_cweights  c_m += sum rho_k over the chunk's cells of commitment m (lists from a counting sort on the host)
//   k_vcb_bucket    the variable-base sum: bucket (slice-slot, window, |digit|) += +-pi_k for both scalar sets
// and after the last chunk the same bucket kernel over the commitments with the scalars c, then k_vcb_reduce (slots folded, each
// window's 128 buckets to sum_b b B_b), the fixed-base sum of `a` (k_vc_sum) and the finish of vcb_finish.h on the calling thread or
// in the one-thread kernel k_vcb_finish.  The buckets live in the lane arena for the whole call and every bucket has one owner
// thread, so chunk after chunk adds into them without atomics.  DESIGN.md section 3.5f.
//
// The file also holds, next to the stages they launch, the driver core this call shares with the three of verify_eval_batch.hip
// (vcb_shared.h): vcb_work, vcb_points, vcb_commit_weights, vcb_cagg.  vcb_run below is what is this call's alone.
#include <algorithm>
#include <chrono>
#include <vector>

#include "vcb_shared.h"

namespace kzg {

// any scalar of sfmt -> canonical and reduced
__global__ __launch_bounds__(256) void k_vcb_canon(const Fr *in, size_t n, int is_mont, Fr *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = is_mont ? from_mont(in[i]) : mul(in[i], Fr::one());
}

// s1[k] = rho_k, s2[k] = rho_k h_k, canonical; h_k = w^(i_k l) = pos_hi[e >> 10] pos_lo[e & 1023], e = i_k l < N (as k_vc_check forms it)
__global__ __launch_bounds__(256) void k_vcb_scalars(const Fr *rho, const uint32_t *ids, size_t count, uint32_t log_l, const Fr *wlo,
                                                     const Fr *whi, Fr *s1, Fr *s2) {
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint32_t e = ids[k] << log_l;
    const Fr p = rho[k];
    s1[k] = from_mont(p);
    s2[k] = from_mont(mul(p, mul(whi[e >> 10], wlo[e & 1023])));
}

// part[blk l + j] = sum over the workgroup's 64 cells of rho_k r_{k,j}.  256 / l cells side by side, thread (row, j); the rows fold in
// LDS in a fixed order.  r is in the caller's scalar format and rho Montgomery, so the products keep the format of r.
__global__ __launch_bounds__(256) void k_vcb_fold(const Fr *r, const Fr *rho, size_t count, uint32_t log_l, Fr *part) {
    __shared__ Fr sh[256];
    const uint32_t l = 1u << log_l, j = threadIdx.x & (l - 1), row = threadIdx.x >> log_l, rows = 256u >> log_l;
    const size_t k0 = (size_t)blockIdx.x * VCB_FOLD_CELLS;
    Fr acc = Fr::zero();
    for (uint32_t c = row; c < VCB_FOLD_CELLS && k0 + c < count; c += rows) acc = add(acc, mul(r[((k0 + c) << log_l) + j], rho[k0 + c]));
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (row == 0) {
        for (uint32_t q = 1; q < rows; q++) acc = add(acc, sh[(q << log_l) + j]);
        part[((size_t)blockIdx.x << log_l) + j] = acc;
    }
}
__global__ __launch_bounds__(256) void k_vcb_fold2(const Fr *part, uint32_t blocks, uint32_t l, Fr *a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= l) return;
    Fr acc = a[j];
    for (uint32_t b = 0; b < blocks; b++) acc = add(acc, part[(size_t)b * l + j]);
    a[j] = acc;
}

// one workgroup per non-empty list: c[m] += sum of rho over order[start[g] .. start[g + 1]) (Montgomery)
__global__ __launch_bounds__(64) void k_vcb_cweights(const Fr *rho, const uint32_t *which, const uint32_t *start, const uint32_t *order, Fr *c) {
    __shared__ Fr sh[64];
    const uint32_t g = blockIdx.x, t = threadIdx.x, e0 = start[g], e1 = start[g + 1];
    Fr acc = Fr::zero();
    for (uint32_t e = e0 + t; e < e1; e += 64) acc = add(acc, rho[order[e]]);
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = 32; s >= 1; s >>= 1) {
        if (t < s) sh[t] = add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) c[which[g]] = add(c[which[g]], sh[0]);
}

// ---- the variable-base sum ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ G1Affine vcb_point(const G1Affine *pts, size_t i) { return pts[i]; }
__device__ __forceinline__ G1Affine vcb_point(const G1Xyzz *pts, size_t i) {  // decode_points leaves zz = zzz = 1, or the identity
    G1Affine a;
    if (pts[i].zz.is_zero()) return G1Affine::inf();
    a.x = pts[i].x;
    a.y = pts[i].y;
    return a;
}

// Workgroup (slice, window, set): the window's digit of the slice's <= S canonical scalars, a counting sort of the point indices by
// |digit| in LDS (128 counters, a scan, a scatter), then thread b walks the contiguous list of bucket b + 1 with mixed additions into
// the bucket it owns.  The order inside a list is whatever the scatter left; the sum of a list does not depend on it, and g1_madd
// handles P + P, P + (-P) and the identity.  Set z takes the scalars sc[z] into the buckets bk[z]; the points are shared.
template <class PT>
__global__ __launch_bounds__(128) void k_vcb_bucket(const PT *pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1) {
    __shared__ uint32_t cnt[VC_D], cur[VC_D];
    __shared__ uint16_t dig[VCB_S], ent[VCB_S];
    const uint32_t t = threadIdx.x, slot = blockIdx.x, win = blockIdx.y;
    const Fr *sc = blockIdx.z ? sc1 : sc0;
    G1Xyzz *bk = (blockIdx.z ? bk1 : bk0) + ((size_t)slot * VC_W + win) * VC_D;
    const size_t p0 = (size_t)slot * VCB_S;
    const uint32_t m = (uint32_t)(n - p0 < VCB_S ? n - p0 : VCB_S);  // the grid has ceil(n / S) slices: p0 < n
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
        if (mag) ent[atomicAdd(&cur[mag - 1], 1u)] = (uint16_t)(p | (d & 0x8000u));  // a slot below the slice's count of non-zero digits
    }
    __syncthreads();
    const uint32_t len = cnt[t];
    if (!len) return;
    G1Xyzz acc = bk[t];
    for (uint32_t e = first; e < first + len; e++) {
        const uint32_t x = ent[e];
        G1Affine p = vcb_point(pts, p0 + (x & 0x7fffu));
        if (x & 0x8000u) p = g1_neg(p);
        acc = g1_madd(acc, p);
    }
    bk[t] = acc;
}

// Workgroup (window, set): thread b folds the `slots` slice slots of bucket b + 1, then the 128 buckets become sum_b (b + 1) B_b by a
// suffix scan (7 rounds) and a tree sum of the suffixes (7 rounds) in LDS.  out[set][window].
__global__ __launch_bounds__(128) void k_vcb_reduce(const G1Xyzz *bk, uint32_t slots, G1Xyzz *out) {
    __shared__ G1Xyzz sh[VC_D];
    const uint32_t t = threadIdx.x, win = blockIdx.x, set = blockIdx.y;
    const G1Xyzz *b = bk + (size_t)set * VCB_G * VCB_SET + (size_t)win * VC_D + t;
    G1Xyzz acc = b[0];
    for (uint32_t g = 1; g < slots; g++) acc = g1_add(acc, b[(size_t)g * VCB_SET]);
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = 1; s < VC_D; s <<= 1) {  // suffix sums: sh[t] = sum_{u >= t} B_u
        const bool on = t + s < VC_D;
        G1Xyzz o;
        if (on) o = sh[t + s];
        __syncthreads();
        if (on) {
            acc = g1_add(acc, o);
            sh[t] = acc;
        }
        __syncthreads();
    }
    for (uint32_t s = VC_D / 2; s >= 1; s >>= 1) {
        if (t < s) sh[t] = g1_add(sh[t], sh[t + s]);
        __syncthreads();
    }
    if (t == 0) out[(size_t)set * VC_W + win] = sh[0];
}

// the finish on the GPU (option host_pairing = 0): the three Horner chains side by side on lanes 0 .. 2 of the one wave (lockstep: the
// time of one chain), then one thread for the pairing check, as k_vc_check
__global__ __launch_bounds__(64) void k_vcb_finish(const VcbSums *sums, const G2Affine *hq, const Fq2 *lines, uint8_t *ok, G1Affine *parts) {
    __shared__ G1Xyzz tot[3];
    if (blockIdx.x) return;
    if (threadIdx.x < 3) vcb_horner(tot[threadIdx.x], sums->win[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) ok[0] = vcb_check(tot, sums->ragg, hq, lines, parts) ? 1 : 0;
}

namespace {
template <class PT>
int vb_accumulate_any(kzg_ctx *ctx, hipStream_t st, const PT *d_pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1, int sets) {
    if (!n) return KZG_OK;
    KZG_LAUNCH(ctx, st, "k_vcb_bucket", k_vcb_bucket<PT>, dim3(vcb_grid(n, VCB_S), VC_W, sets), 128, 0, d_pts, sc0, sc1, n, bk0, bk1);
    return KZG_OK;
}
}  // namespace

// ---- the stages behind vcb_shared.h --------------------------------------------------------------------------------------------
int vb_accumulate(kzg_ctx *ctx, hipStream_t st, const G1Xyzz *d_pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1, int sets) {
    return vb_accumulate_any(ctx, st, d_pts, sc0, sc1, n, bk0, bk1, sets);
}
int vb_accumulate(kzg_ctx *ctx, hipStream_t st, const G1Affine *d_pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1, int sets) {
    return vb_accumulate_any(ctx, st, d_pts, sc0, sc1, n, bk0, bk1, sets);
}

int vb_reduce(kzg_ctx *ctx, hipStream_t st, const G1Xyzz *d_bk, uint32_t slots, VcbSums *d_sums) {
    KZG_LAUNCH(ctx, st, "k_vcb_reduce", k_vcb_reduce, dim3(VC_W, 3), 128, 0, d_bk, slots, &d_sums->win[0][0]);
    return KZG_OK;
}

int vcb_canon(kzg_ctx *ctx, hipStream_t st, const Fr *d_in, size_t n, int is_mont, Fr *d_out) {
    if (!n) return KZG_OK;
    KZG_LAUNCH(ctx, st, "k_vcb_canon", k_vcb_canon, vcb_grid(n), 256, 0, d_in, n, is_mont, d_out);
    return KZG_OK;
}

int vcb_fold(kzg_ctx *ctx, hipStream_t st, const Fr *d_r, const Fr *d_rho, size_t B, uint32_t log_l, Fr *d_part, Fr *d_a) {
    const uint32_t fb = vcb_grid(B, VCB_FOLD_CELLS), l = 1u << log_l;
    KZG_LAUNCH(ctx, st, "k_vcb_fold", k_vcb_fold, fb, 256, 0, d_r, d_rho, B, log_l, d_part);
    KZG_LAUNCH(ctx, st, "k_vcb_fold2", k_vcb_fold2, vcb_grid(l), 256, 0, (const Fr *)d_part, fb, l, d_a);
    return KZG_OK;
}

int vcb_cweights(kzg_ctx *ctx, hipStream_t st, const Fr *d_rho, const uint32_t *d_which, const uint32_t *d_start, const uint32_t *d_order,
                 size_t lists, Fr *d_c) {
    KZG_LAUNCH(ctx, st, "k_vcb_cweights", k_vcb_cweights, (unsigned)lists, 64, 0, d_rho, d_which, d_start, d_order, d_c);
    return KZG_OK;
}

int load_challenge(kzg_ctx *ctx, const char *who, const void *r, int sfmt, Fr *mont) {
    Fr x;
    memcpy(x.v, r, 32);
    if (!is_canonical(x) || x.is_zero()) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": the challenge r must be in [1, modulus)");
    *mont = sfmt == KZG_FR_MONT_LE_32 ? x : to_mont(x);
    return KZG_OK;
}

int vcb_conclude(kzg_ctx *ctx, int lane, const VcbSums *d_sums, const G2Affine *d_hq, const Fq2 *d_lines, const G2Affine *h_hq,
                 const Fq2 *h_lines, const int *d_bad, uint8_t *d_ok, G1Affine *d_parts, void *points, int *ok) {
    hipStream_t st = ctx->lanes[lane].stream;
    const bool on_host = ctx->opt_host_pairing != 0;
    KZG_TRY(lane_pinned(ctx, lane, 1024 + sizeof(VcbSums)));
    char *pin = ctx->lanes[lane].pinned;
    if (!on_host) {
        KZG_LAUNCH(ctx, st, "k_vcb_finish", k_vcb_finish, 1, 64, 0, d_sums, d_hq, d_lines, d_ok, points ? d_parts : (G1Affine *)nullptr);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(pin + 64, d_ok, 1, hipMemcpyDeviceToHost, st));
        if (points) KZG_HIP_CHECK(ctx, hipMemcpyAsync(pin + 128, d_parts, 4 * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
    } else {
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(pin + 1024, d_sums, sizeof(VcbSums), hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(pin, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    // the decode flag before the verdict, as fetch_ok
    if (*(int *)pin) return fail(ctx, KZG_ERR_BAD_POINT, "an input point failed to decode, is not on the curve or not in the r-torsion subgroup");
    int verdict;
    if (on_host) {
        const auto t0 = std::chrono::steady_clock::now();
        verdict = vcb_finish(*(const VcbSums *)(pin + 1024), h_hq, h_lines, points ? (G1Affine *)(pin + 128) : nullptr) ? 1 : 0;
        if (ctx->prof) {  // the calling thread's share of the call, beside the kernels of kzg_prof_get
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::lock_guard<std::mutex> lk(ctx->prof_mu);
            ProfEntry &e = ctx->prof_map["vcb_host_finish"];
            e.launches++;
            e.total_ms += ms;
        }
    } else {
        verdict = pin[64] ? 1 : 0;
    }
    if (points) memcpy(points, pin + 128, 4 * sizeof(G1Affine));
    *ok = verdict;
    return KZG_OK;
}

// ---- the driver core behind vcb_shared.h -----------------------------------------------------------------------------------------
int vcb_work(kzg_ctx *ctx, int lane, int pfmt, size_t B0, size_t BP, size_t c_count, size_t extra_bytes, size_t slots0, VcbWork *w) {
    const size_t psz = point_format_bytes(pfmt), set = (size_t)VCB_G * VCB_SET, bucket_bytes = 3 * set * sizeof(G1Xyzz);
    KZG_TRY(lane_reserve(ctx, lane, bucket_bytes + sizeof(VcbSums) + c_count * 32 + BP * (psz + sizeof(G1Xyzz)) + B0 * (3 * 4 + 3 * 32) +
                                        extra_bytes + 65536));
    w->ctx = ctx;
    w->lane = lane;
    w->pfmt = pfmt;
    w->st = ctx->lanes[lane].stream;
    w->psz = psz;
    w->BP = BP;
    w->slots = slots0;
    w->bad = (int *)lane_alloc(ctx, lane, 256);
    w->d_ok = (uint8_t *)lane_alloc(ctx, lane, 256);
    w->d_parts = (G1Affine *)lane_alloc(ctx, lane, 4 * sizeof(G1Affine));
    G1Xyzz *bk = (G1Xyzz *)lane_alloc(ctx, lane, bucket_bytes);
    w->sums = (VcbSums *)lane_alloc(ctx, lane, sizeof(VcbSums));
    w->d_c = (Fr *)lane_alloc(ctx, lane, c_count * 32);
    w->d_which = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    w->d_start = (uint32_t *)lane_alloc(ctx, lane, (B0 + 1) * 4);
    w->d_order = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    w->d_rho = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    w->d_s1 = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    w->d_s2 = (Fr *)lane_alloc(ctx, lane, B0 * 32);
    w->raw = (uint8_t *)lane_alloc(ctx, lane, BP * psz);
    w->W = (G1Xyzz *)lane_alloc(ctx, lane, BP * sizeof(G1Xyzz));
    if (!w->bad || !w->d_ok || !w->d_parts || !bk || !w->sums || !w->d_c || !w->d_which || !w->d_start || !w->d_order || !w->d_rho ||
        !w->d_s1 || !w->d_s2 || !w->raw || !w->W)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    for (int s = 0; s < 3; s++) w->bk[s] = bk + s * set;
    KZG_HIP_CHECK(ctx, hipMemsetAsync(w->bad, 0, sizeof(int), w->st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, bucket_bytes, w->st));  // zz = 0: the identity
    KZG_HIP_CHECK(ctx, hipMemsetAsync(w->d_c, 0, c_count * 32, w->st));
    return KZG_OK;
}

int vcb_points(VcbWork *w, const void *src, size_t B, const Fr *sc0, const Fr *sc1, G1Xyzz *bk0, G1Xyzz *bk1, int sets) {
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->raw, src, B * w->psz, hipMemcpyHostToDevice, w->st));
    KZG_TRY(decode_points(w->ctx, w->st, w->raw, B, w->pfmt, w->W, w->bad, untrusted_level(w->ctx)));
    KZG_TRY(vb_accumulate(w->ctx, w->st, (const G1Xyzz *)w->W, sc0, sc1, B, bk0, bk1, sets));
    w->slots = std::max(w->slots, (B + VCB_S - 1) / VCB_S);
    return KZG_OK;
}

int vcb_commit_weights(VcbWork *w, VcbLists *lists, const uint32_t *cm, size_t B) {
    const size_t n = lists->build(cm, B);
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_which, lists->which.data(), n * 4, hipMemcpyHostToDevice, w->st));
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_start, lists->start.data(), (n + 1) * 4, hipMemcpyHostToDevice, w->st));
    KZG_HIP_CHECK(w->ctx, hipMemcpyAsync(w->d_order, lists->order.data(), B * 4, hipMemcpyHostToDevice, w->st));
    return vcb_cweights(w->ctx, w->st, w->d_rho, w->d_which, w->d_start, w->d_order, n, w->d_c);
}

int vcb_cagg(VcbWork *w, const void *commitments, size_t n_commitments) {
    for (size_t m0 = 0; m0 < n_commitments; m0 += w->BP) {
        const size_t B = std::min(w->BP, n_commitments - m0);
        KZG_TRY(vcb_canon(w->ctx, w->st, w->d_c + m0, B, 1, w->d_c + m0));
        KZG_TRY(vcb_points(w, (const uint8_t *)commitments + m0 * w->psz, B, w->d_c + m0, w->d_c + m0, w->bk[2], w->bk[2], 1));
    }
    return KZG_OK;
}

namespace {
struct BatchParts {  // the extra outputs of kzg_test_verify_cosets_batch_parts (host)
    void *a = nullptr, *cw = nullptr, *points = nullptr;
};

int vcb_run(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments, const uint32_t *commitment_idx,
            const size_t *coset_ids, const void *cells, const void *proofs, size_t count, const void *r, int sfmt, int pfmt, int flags, int *ok,
            const BatchParts *parts) {
    const char *who = "kzg_verify_cosets_batch";
    // ---- shape: everything is decided before memory is touched or a kernel launched (the rules of kzg_verify_cosets) ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (!plan) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL plan");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / proofs are affine (G1Affine)");
    if (plan->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the plan is resident on another GPU than this context's");
    if (!count) {
        if (ok) *ok = 1;
        return KZG_OK;
    }
    if (!commitments || !commitment_idx || !coset_ids || !cells || !proofs || !r || !ok) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL argument");
    Fr rm;
    KZG_TRY(load_challenge(ctx, who, r, sfmt, &rm));
    const uint32_t log_l = plan->log_l;
    const size_t l = (size_t)1 << log_l, K = (size_t)1 << (plan->log_n - log_l);
    if (count > (SIZE_MAX >> 6) / l || n_commitments > (SIZE_MAX >> 9)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": count too large");
    const size_t chunk = vc_chunk(ctx, plan), B0 = std::min(chunk, count), BP = std::min(chunk, std::max(count, n_commitments));
    std::vector<uint32_t> meta;  // ids, then commitment indices, as the kernels read them
    VcbLists lists;
    bool room = lists.reserve(n_commitments, B0);
    try {  // (no exception may leave through the C ABI)
        meta.resize(2 * count);
    } catch (const std::bad_alloc &) {
        room = false;
    }
    if (!room) return fail(ctx, KZG_ERR_ALLOC, std::string(who) + ": host memory for the ids");
    for (size_t k = 0; k < count; k++) {
        if (coset_ids[k] >= K) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": coset id >= K");
        if (commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": commitment index >= n_commitments");
        meta[k] = (uint32_t)coset_ids[k];
        meta[count + k] = commitment_idx[k];
    }

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    StreamDrain drain{st};
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t fold_blocks = (B0 + VCB_FOLD_CELLS - 1) / VCB_FOLD_CELLS;
    VcbWork w;  // no gs[0] pair here: no slice slot is in use before the first chunk
    KZG_TRY(vcb_work(ctx, lane, pfmt, B0, BP, std::max<size_t>(n_commitments, 1), B0 * (4 + (in_dev ? 1 : 2) * l * 32) + (fold_blocks + 1) * l * 32, 0, &w));
    Fr *d_a = (Fr *)lane_alloc(ctx, lane, l * 32), *d_part = (Fr *)lane_alloc(ctx, lane, fold_blocks * l * 32);
    uint32_t *d_ids = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    Fr *d_cells = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, B0 * l * 32), *d_r = (Fr *)lane_alloc(ctx, lane, B0 * l * 32);
    if (!d_a || !d_part || !d_ids || (!in_dev && !d_cells) || !d_r) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_a, 0, l * 32, st));
    for (size_t k0 = 0; k0 < count; k0 += chunk) {
        const size_t B = std::min(chunk, count - k0);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_ids, meta.data() + k0, B * 4, hipMemcpyHostToDevice, st));
        const Fr *src = (const Fr *)((const uint8_t *)cells + k0 * l * 32);
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_cells, src, B * l * 32, hipMemcpyHostToDevice, st));
            src = d_cells;
        }
        KZG_TRY(powers_run(ctx, st, rm, k0, B, w.d_rho));
        KZG_TRY(vc_interp(ctx, st, plan, src, d_ids, B, d_r));
        KZG_LAUNCH(ctx, st, "k_vcb_scalars", k_vcb_scalars, vcb_grid(B), 256, 0, (const Fr *)w.d_rho, (const uint32_t *)d_ids, B, log_l,
                   (const Fr *)plan->pos_lo, (const Fr *)plan->pos_hi, w.d_s1, w.d_s2);
        KZG_TRY(vcb_fold(ctx, st, d_r, w.d_rho, B, log_l, d_part, d_a));                                    // a
        KZG_TRY(vcb_commit_weights(&w, &lists, meta.data() + count + k0, B));                               // c
        KZG_TRY(vcb_points(&w, (const uint8_t *)proofs + k0 * psz, B, w.d_s1, w.d_s2, w.bk[0], w.bk[1], 2));  // P1, P2
        // the host lists and the chunk's device buffers are free again
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    KZG_TRY(vcb_cagg(&w, commitments, n_commitments));
    KZG_TRY(vb_reduce(ctx, st, w.bk[0], (uint32_t)w.slots, w.sums));
    KZG_TRY(vc_sum(ctx, st, plan, d_a, 1, sfmt, &w.sums->ragg));
    if (parts) {
        if (sfmt == KZG_FR_MONT_LE_32) KZG_TRY(vcb_canon(ctx, st, d_a, l, 1, d_a));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(parts->a, d_a, l * 32, hipMemcpyDeviceToHost, st));
        if (n_commitments) KZG_HIP_CHECK(ctx, hipMemcpyAsync(parts->cw, w.d_c, n_commitments * 32, hipMemcpyDeviceToHost, st));
    }
    return vcb_conclude(ctx, lane, w.sums, plan->hq, plan->lines, plan->h_hq, plan->h_lines, w.bad, w.d_ok, w.d_parts, parts ? parts->points : nullptr, ok);
}
}  // namespace

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_verify_cosets_batch(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                                       const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs,
                                       size_t count, const void *r, int sfmt, int pfmt, int flags, int *ok) {
    return vcb_run(ctx, plan, commitments, n_commitments, commitment_idx, coset_ids, cells, proofs, count, r, sfmt, pfmt, flags, ok, nullptr);
}

#ifdef KZG_TEST_HOOKS
#include "../../include/kzg_mi355x_test.h"
extern "C" int kzg_test_verify_cosets_batch_parts(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                                                  const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs,
                                                  size_t count, const void *r, int sfmt, int pfmt, int flags, int *ok, void *out_a, void *out_cw,
                                                  void *out_points) {
    if (!out_a || !out_cw || !out_points || !count) return KZG_ERR_SHAPE;
    BatchParts parts;
    parts.a = out_a;
    parts.cw = out_cw;
    parts.points = out_points;
    return vcb_run(ctx, plan, commitments, n_commitments, commitment_idx, coset_ids, cells, proofs, count, r, sfmt, pfmt, flags, ok, &parts);
}

// the variable-base routine alone over row 0 of a resident SRS: out = sum_i scalars[i] srs[offset + i], affine Montgomery
extern "C" int kzg_test_vb_msm(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n, int sfmt, void *out) {
    if (!ctx || !srs || !scalars || !out || !n) return KZG_ERR_SHAPE;
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return KZG_ERR_SHAPE;
    if (offset > srs->n || n > srs->n - offset || srs->device != ctx->device) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    const size_t CH = (size_t)VCB_G * VCB_S, B0 = std::min(CH, n), set_bytes = (size_t)VCB_G * VCB_SET * sizeof(G1Xyzz);
    KZG_TRY(lane_reserve(ctx, 0, 3 * set_bytes + sizeof(VcbSums) + B0 * 64 + 65536));
    G1Xyzz *bk = (G1Xyzz *)lane_alloc(ctx, 0, 3 * set_bytes);  // k_vcb_reduce walks three sets: two stay empty
    VcbSums *sums = (VcbSums *)lane_alloc(ctx, 0, sizeof(VcbSums));
    Fr *d_in = (Fr *)lane_alloc(ctx, 0, B0 * 32), *d_sc = (Fr *)lane_alloc(ctx, 0, B0 * 32);
    G1Affine *d_out = (G1Affine *)lane_alloc(ctx, 0, 4 * sizeof(G1Affine));
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, 0, 256);
    if (!bk || !sums || !d_in || !d_sc || !d_out || !d_ok) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bk, 0, 3 * set_bytes, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, sizeof(VcbSums), st));
    size_t slots = 0;
    for (size_t i0 = 0; i0 < n; i0 += CH) {
        const size_t B = std::min(CH, n - i0);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, (const uint8_t *)scalars + i0 * 32, B * 32, hipMemcpyHostToDevice, st));
        KZG_TRY(vcb_canon(ctx, st, d_in, B, sfmt == KZG_FR_MONT_LE_32 ? 1 : 0, d_sc));
        KZG_TRY(vb_accumulate(ctx, st, (const G1Affine *)srs->table + offset + i0, d_sc, d_sc, B, bk, bk, 1));
        slots = std::max(slots, (B + VCB_S - 1) / VCB_S);
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    KZG_TRY(vb_reduce(ctx, st, bk, (uint32_t)slots, sums));
    VcbSums h;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(&h, sums, sizeof(VcbSums), hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    G1Xyzz sum;
    vcb_horner(sum, h.win[0]);
    const G1Affine a = g1_to_affine(sum);
    memcpy(out, &a, sizeof(G1Affine));
    return KZG_OK;
}
#endif
