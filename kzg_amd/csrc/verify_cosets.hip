// verify_cosets.hip -- kzg_verify_cosets: one verdict per cell for any number of coset openings (the cells kzg_witness_cosets_* proves
// and kzg_recover_cosets consumes), against a plan built once per (SRS, domain, coset size).  Not a reference method.
//
// Coset i of the size-N domain is { w^(i + tK) : t < l }, K = N / l, nu = w^K, vanishing polynomial X^l - w^(il).  A cell is the l
// values v_t = p(w^(i + tK)); its opening is pi_i = [(p - r_i) / (X^l - w^(il))]_1 with r_i the interpolant through the cell.
//   1. k_vc_interp   r_i from the values, Fr only: u = iNTT_l(v) over nu, r_{i,j} = u_j w^(-ij)    (r_i(w^i nu^t) = sum_j u_j nu^(jt) = v_t)
//   2. k_vc_sum      R_i = [r_i(tau)]_1 = sum_j r_{i,j} gs[j]: the same l bases for every cell, so the sum is gathered from a window
//                    table T[win][j][d] = [d 2^(c win)] gs[j] (affine, d = 1 .. 2^(c-1), signed digits): no doubling, no bucket
//   3. k_vc_check    e(pi_i, [tau^l]H - [w^(il)]H) == e(C - R_i, H)  rearranged to  e(pi_i, hs[l]) e(-([w^(il)] pi_i + C - R_i), hs[0]) == 1:
//                    both G2 arguments are plan constants with stored Miller lines, so a check is one G1 scalar multiplication,
//                    the shared Miller loop and the final exponentiation -- the shape of k_verify_eval (pairing.hip)
// The three stay separate kernels: the table walk wants every lane of the chip (one wave per cell), the pairing one thread per cell
// and its whole register budget.  DESIGN.md section 3.5e.
#include <algorithm>
#include <new>
#include <vector>

#include "verify_cosets_shared.h"

namespace kzg {

// ---- plan construction -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vc_base(const G1Affine *gs, uint32_t l, G1Xyzz *base) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < l) base[j] = G1Xyzz::from_affine(gs[j]);
}

// row[j D + d - 1] = [d] base[j], d = 1 .. D
__global__ __launch_bounds__(256) void k_vc_row(const G1Xyzz *base, uint32_t l, G1Xyzz *row) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= l * VC_D) return;
    const uint32_t d = (i & (VC_D - 1)) + 1;
    const G1Xyzz b = base[i / VC_D];
    G1Xyzz acc = G1Xyzz::inf();
    for (int bit = 31 - __clz(d); bit >= 0; bit--) {
        acc = g1_dbl(acc);
        if ((d >> bit) & 1) acc = g1_add(acc, b);
    }
    row[i] = acc;
}

// the next window's base: [2^c] base[j] = 2 [D] base[j]
__global__ __launch_bounds__(256) void k_vc_next(const G1Xyzz *row, uint32_t l, G1Xyzz *base) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < l) base[j] = g1_dbl(row[(size_t)j * VC_D + VC_D - 1]);
}

// hq = { hs[0], hs[l] } and their stored Miller lines
__global__ __launch_bounds__(64) void k_vc_lines(const G2Affine *hs, size_t l, G2Affine *hq, Fq2 *lines) {
    const int j = threadIdx.x;
    if (j >= 2) return;
    const G2Affine q = hs[j ? l : 0];
    hq[j] = q;
    g2_precompute_lines(q, lines + (size_t)j * 2 * MILLER_LINES);
}

// ---- 1. interpolation --------------------------------------------------------------------------------------------------------
// 256 / l cells per workgroup, one thread per value.  Bit-reversed into LDS, log_l decimation-in-time stages over nu^-1, then the
// scaling by w^(-ij) / l = hi[e >> 10] lo[e & 1023], e = ij mod N (lo carries the 1 / l).  The twiddles are Montgomery residues,
// so the values keep the form they came in (canonical or Montgomery); a value >= r is reduced on the way in.
__global__ __launch_bounds__(256) void k_vc_interp(const Fr *cells, const uint32_t *ids, size_t count, uint32_t log_n, uint32_t log_l,
                                                   const Fr *nu_inv, const Fr *lo, const Fr *hi, Fr *r) {
    __shared__ Fr sh[256];
    const uint32_t l = 1u << log_l;
    const uint32_t t = threadIdx.x & (l - 1), cl = threadIdx.x >> log_l;
    const size_t cell = (size_t)blockIdx.x * (256u >> log_l) + cl;
    const bool live = cell < count;
    Fr *x = sh + ((size_t)cl << log_l);
    if (live) x[log_l ? __brev(t) >> (32 - log_l) : 0u] = mul(cells[(cell << log_l) + t], Fr::one());
    __syncthreads();
    for (uint32_t s = 0; s < log_l; s++) {
        if (live && t < (l >> 1)) {
            const uint32_t j = t & ((1u << s) - 1u), i0 = ((t >> s) << (s + 1)) | j, i1 = i0 + (1u << s);
            const Fr u = x[i0], v = mul(x[i1], nu_inv[j << (log_l - 1 - s)]);
            x[i0] = add(u, v);
            x[i1] = sub(u, v);
        }
        __syncthreads();
    }
    if (live) {
        const uint32_t e = (uint32_t)(((uint64_t)ids[cell] * t) & ((1ull << log_n) - 1ull));
        r[(cell << log_l) + t] = mul(x[t], mul(hi[e >> 10], lo[e & 1023]));
    }
}

// ---- 2. fixed-base sum -------------------------------------------------------------------------------------------------------
// One wave per cell: lane e takes the (base, window) pairs e, e + 64, ... of the cell's l W, adds its table entries into one XYZZ
// accumulator (mixed additions) and the 64 partial sums fold in LDS in six rounds.  out[cell] = R.
__global__ __launch_bounds__(64) void k_vc_sum(const Fr *r, uint32_t log_l, int is_mont, const G1Affine *table, G1Xyzz *out) {
    __shared__ uint32_t sc[(1u << VC_MAX_LOG_L) * 8];
    __shared__ G1Xyzz part[64];
    const uint32_t l = 1u << log_l, lane = threadIdx.x;
    const size_t cell = blockIdx.x;
    for (uint32_t j = lane; j < l; j += 64) {
        Fr s = r[(cell << log_l) + j];
        s = is_mont ? from_mont(s) : mul(s, Fr::one());
#pragma unroll
        for (int i = 0; i < 8; i++) sc[j * 8 + i] = s.v[i];
    }
    __syncthreads();
    G1Xyzz acc = G1Xyzz::inf();
    for (uint32_t e = lane; e < l * VC_W; e += 64) {
        const uint32_t j = e / VC_W, win = e % VC_W;
        const int d = vc_digit(sc + j * 8, (int)win);
        if (d == 0) continue;
        G1Affine p = table[(((size_t)win << log_l) + j) * VC_D + (uint32_t)(d < 0 ? -d : d) - 1u];
        if (d < 0) p = g1_neg(p);
        acc = g1_madd(acc, p);
    }
    part[lane] = acc;
    __syncthreads();
    for (uint32_t s = 32; s >= 1; s >>= 1) {
        if (lane < s) part[lane] = g1_add(part[lane], part[lane + s]);
        __syncthreads();
    }
    if (lane == 0) out[cell] = part[0];
}

// ---- 3. check ----------------------------------------------------------------------------------------------------------------
// one thread per cell, as k_verify_eval: P0 = pi against hs[l], P1 = -([w^(il)] pi + C - R) against hs[0], stored lines for both.
// An identity proof contributes 1, which leaves C == R (what FK20 emits for n <= l, with r = p).
__global__ __launch_bounds__(64) void k_vc_check(const uint32_t *ids, const uint32_t *cidx, uint32_t log_l, const Fr *wlo, const Fr *whi,
                                                 const G1Xyzz *Cs, const G1Xyzz *Ws, const G1Xyzz *Rs, const G2Affine *hq, const Fq2 *lines,
                                                 size_t count, uint8_t *ok) {
    size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    uint32_t k[8];
    G1Affine P[2];
    G2Affine Q[2], T[2];
    const Fq2 *tabs[2] = {lines + 2 * MILLER_LINES, lines};  // pair 0 against hs[l], pair 1 against hs[0]
    const G1Affine w = g1_to_affine(Ws[c]);
    const uint32_t e = ids[c] << log_l;  // il < N
    const Fr x = from_mont(mul(whi[e >> 10], wlo[e & 1023]));
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = x.v[i];
    G1Xyzz nr = Rs[c];
    if (!nr.y.is_zero()) nr.y = neg(nr.y);
    const G1Xyzz acc = g1_add(g1_add(g1_scalar_mul(w, k), Cs[cidx[c]]), nr);
    P[0] = w;
    P[1] = g1_neg(g1_to_affine(acc));
    Q[0] = hq[1];
    Q[1] = hq[0];
    ok[c] = pairing_product_is_one(P, Q, T, 2, tabs) ? 1 : 0;
}

}  // namespace kzg

using namespace kzg;

namespace {
static inline unsigned vc_grid(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

void vc_release(kzg_cosets_verifier *p) {
    if (!p) return;
    if (p->table) hipFree(p->table);
    if (p->hq) hipFree(p->hq);
    if (p->lines) hipFree(p->lines);
    if (p->ninv_lo) hipFree(p->ninv_lo);
    delete p;
}

}  // namespace

// stages 1 and 2 of a chunk of B cells on stream st: d_cells (sfmt) -> d_r (sfmt) -> d_R
int kzg::vc_interp(kzg_ctx *ctx, hipStream_t st, const kzg_cosets_verifier *p, const Fr *d_cells, const uint32_t *d_ids, size_t B, Fr *d_r) {
    KZG_LAUNCH(ctx, st, "k_vc_interp", k_vc_interp, vc_grid(B, 256u >> p->log_l), 256, 0, d_cells, d_ids, B, p->log_n, p->log_l,
               (const Fr *)p->nu_inv, (const Fr *)p->ninv_lo, (const Fr *)p->ninv_hi, d_r);
    return KZG_OK;
}
int kzg::vc_sum(kzg_ctx *ctx, hipStream_t st, const kzg_cosets_verifier *p, const Fr *d_r, size_t B, int sfmt, G1Xyzz *d_R) {
    KZG_LAUNCH(ctx, st, "k_vc_sum", k_vc_sum, (unsigned)B, 64, 0, d_r, p->log_l, sfmt == KZG_FR_MONT_LE_32 ? 1 : 0, (const G1Affine *)p->table,
               d_R);
    return KZG_OK;
}

size_t kzg::vc_chunk(const kzg_ctx *ctx, const kzg_cosets_verifier *p) {
    size_t chunk = std::max<size_t>(1, std::min(VC_CHUNK_CELLS, VC_CHUNK_SCALARS >> p->log_l));
    if (ctx->opt_verify_cosets_chunk > 0) chunk = std::min(chunk, (size_t)ctx->opt_verify_cosets_chunk);
    return chunk;
}

extern "C" int kzg_cosets_verifier_setup(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, uint32_t log_n, uint32_t log_l,
                                         kzg_cosets_verifier **out) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!gs || !hs || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: NULL argument");
    Guard g(ctx);
    if (log_n > VC_MAX_LOG_N) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: log_n <= 22 (the FK20 plans' limit)");
    if (log_l > log_n) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: coset larger than the domain");
    if (log_l > VC_MAX_LOG_L) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: log_l <= 8 (cosets of up to 256 points)");
    const size_t N = (size_t)1 << log_n, l = (size_t)1 << log_l;
    if (gs->n < l) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: the G1 SRS has fewer than l points");
    if (hs->n < l + 1) return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: the G2 SRS has fewer than l + 1 points");
    if (gs->device != ctx->device || hs->device != ctx->device)
        return fail(ctx, KZG_ERR_SHAPE, "kzg_cosets_verifier_setup: the SRS is resident on another GPU than this context's");
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[0].stream;
    kzg_cosets_verifier *p = new (std::nothrow) kzg_cosets_verifier();
    if (!p) return fail(ctx, KZG_ERR_ALLOC, "kzg_cosets_verifier_setup: host memory");
    p->log_n = log_n;
    p->log_l = log_l;
    p->device = ctx->device;
    p->table_bytes = (size_t)VC_W * l * VC_D * sizeof(G1Affine);
    const size_t hi_n = std::max<size_t>(1, N >> 10), nu_n = std::max<size_t>(1, l >> 1);
    G1Xyzz *base = nullptr, *row = nullptr;
    int rc = KZG_OK;
    if (hipMalloc((void **)&p->table, p->table_bytes) != hipSuccess || hipMalloc((void **)&p->hq, 2 * sizeof(G2Affine)) != hipSuccess ||
        hipMalloc((void **)&p->lines, 2 * 2 * MILLER_LINES * sizeof(Fq2)) != hipSuccess ||
        hipMalloc((void **)&p->ninv_lo, (2 * 1024 + 2 * hi_n + nu_n) * sizeof(Fr)) != hipSuccess ||
        hipMalloc((void **)&base, l * sizeof(G1Xyzz)) != hipSuccess || hipMalloc((void **)&row, l * VC_D * sizeof(G1Xyzz)) != hipSuccess)
        rc = fail(ctx, KZG_ERR_ALLOC, "kzg_cosets_verifier_setup: hipMalloc");
    auto build = [&]() -> int {
        p->ninv_hi = p->ninv_lo + 1024;
        p->pos_lo = p->ninv_hi + hi_n;
        p->pos_hi = p->pos_lo + 1024;
        p->nu_inv = p->pos_hi + hi_n;
        const Fr w = host_omega(log_n), winv = inv(w), linv = inv(from_u64<FrParams>((uint64_t)l));
        KZG_TRY(pow_table(ctx, st, winv, linv, 1024, p->ninv_lo));
        KZG_TRY(pow_table(ctx, st, pow_u64(winv, 1024), Fr::one(), hi_n, p->ninv_hi));
        KZG_TRY(pow_table(ctx, st, w, Fr::one(), 1024, p->pos_lo));
        KZG_TRY(pow_table(ctx, st, pow_u64(w, 1024), Fr::one(), hi_n, p->pos_hi));
        KZG_TRY(pow_table(ctx, st, pow_u64(winv, (uint64_t)(N >> log_l)), Fr::one(), nu_n, p->nu_inv));
        KZG_LAUNCH(ctx, st, "k_vc_lines", k_vc_lines, 1, 64, 0, (const G2Affine *)hs->pts, l, p->hq, p->lines);
        KZG_LAUNCH(ctx, st, "k_vc_base", k_vc_base, vc_grid(l), 256, 0, (const G1Affine *)gs->table, (uint32_t)l, base);
        for (int win = 0; win < VC_W; win++) {
            KZG_LAUNCH(ctx, st, "k_vc_row", k_vc_row, vc_grid(l * VC_D), 256, 0, (const G1Xyzz *)base, (uint32_t)l, row);
            KZG_TRY(batch_to_affine(ctx, st, row, p->table + (size_t)win * l * VC_D, l * VC_D));
            if (win + 1 < VC_W) KZG_LAUNCH(ctx, st, "k_vc_next", k_vc_next, vc_grid(l), 256, 0, (const G1Xyzz *)row, (uint32_t)l, base);
        }
        return KZG_OK;
    };
    if (rc == KZG_OK) rc = build();
    if (hipStreamSynchronize(st) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "kzg_cosets_verifier_setup: a kernel failed");
    if (rc == KZG_OK && hipGetLastError() != hipSuccess) rc = fail(ctx, KZG_ERR_HIP, "kzg_cosets_verifier_setup: a launch failed");
    if (rc == KZG_OK && (hipMemcpy(p->h_hq, p->hq, sizeof(p->h_hq), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(p->h_lines, p->lines, sizeof(p->h_lines), hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(ctx, KZG_ERR_HIP, "kzg_cosets_verifier_setup: the host copy of the Miller lines");
    if (base) hipFree(base);
    if (row) hipFree(row);
    if (ctx->prof) prof_collect(ctx);
    if (rc != KZG_OK) {
        vc_release(p);
        return rc;
    }
    *out = p;
    return KZG_OK;
}

extern "C" void kzg_cosets_verifier_free(kzg_ctx *ctx, kzg_cosets_verifier *plan) {
    if (!plan) return;
    if (ctx) {
        Guard g(ctx);  // waits for the leased lanes: no call still reads the plan
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->lanes[0].stream);
    }
    vc_release(plan);
}

extern "C" int kzg_cosets_verifier_shape(const kzg_cosets_verifier *plan, size_t *domain, size_t *coset_size, size_t *table_bytes) {
    if (!plan) return KZG_ERR_SHAPE;
    if (domain) *domain = (size_t)1 << plan->log_n;
    if (coset_size) *coset_size = (size_t)1 << plan->log_l;
    if (table_bytes) *table_bytes = plan->table_bytes;
    return KZG_OK;
}

extern "C" int kzg_verify_cosets(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                                 const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs, size_t count,
                                 int sfmt, int pfmt, int flags, uint8_t *ok) {
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (!plan) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_cosets: NULL plan");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(pfmt);
    if (!psz || pfmt == KZG_G1_JACOBIAN_MONT_144) return fail(ctx, KZG_ERR_SHAPE, "commitments / proofs are affine (G1Affine)");
    if (plan->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "the plan is resident on another GPU than this context's");
    if (!count) return KZG_OK;
    if (!commitments || !commitment_idx || !coset_ids || !cells || !proofs || !ok) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_cosets: NULL argument");
    const uint32_t log_l = plan->log_l;
    const size_t l = (size_t)1 << log_l, K = (size_t)1 << (plan->log_n - log_l);
    if (count > (SIZE_MAX >> 6) / l || n_commitments > (SIZE_MAX >> 9)) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_cosets: count too large");
    std::vector<uint32_t> meta;  // ids, then commitment indices, as the kernels read them
    std::vector<uint8_t> verdict;
    try {  // (no exception may leave through the C ABI)
        meta.resize(2 * count);
        verdict.resize(count);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "kzg_verify_cosets: host memory for the ids");
    }
    for (size_t k = 0; k < count; k++) {
        if (coset_ids[k] >= K) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_cosets: coset id >= K");
        if (commitment_idx[k] >= n_commitments) return fail(ctx, KZG_ERR_SHAPE, "kzg_verify_cosets: commitment index >= n_commitments");
        meta[k] = (uint32_t)coset_ids[k];
        meta[count + k] = commitment_idx[k];
    }

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t chunk = vc_chunk(ctx, plan), B0 = std::min(chunk, count);
    KZG_TRY(lane_reserve(ctx, lane, n_commitments * (psz + sizeof(G1Xyzz)) + B0 * (9 + psz + 2 * sizeof(G1Xyzz) + (in_dev ? 1 : 2) * l * 32) + 65536));
    StreamDrain drain{st};
    int *bad = (int *)lane_alloc(ctx, lane, 256);
    uint8_t *d_ok = (uint8_t *)lane_alloc(ctx, lane, B0);
    uint32_t *d_ids = (uint32_t *)lane_alloc(ctx, lane, B0 * 4), *d_cidx = (uint32_t *)lane_alloc(ctx, lane, B0 * 4);
    Fr *d_cells = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, B0 * l * 32), *d_r = (Fr *)lane_alloc(ctx, lane, B0 * l * 32);
    uint8_t *raw = (uint8_t *)lane_alloc(ctx, lane, B0 * psz);
    G1Xyzz *W = (G1Xyzz *)lane_alloc(ctx, lane, B0 * sizeof(G1Xyzz)), *R = (G1Xyzz *)lane_alloc(ctx, lane, B0 * sizeof(G1Xyzz));
    if (!bad || !d_ok || !d_ids || !d_cidx || (!in_dev && !d_cells) || !d_r || !raw || !W || !R) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    G1Xyzz *C = nullptr;
    KZG_TRY(g1_inputs(ctx, lane, commitments, n_commitments, pfmt, &C, bad));
    for (size_t k0 = 0; k0 < count; k0 += chunk) {
        const size_t B = std::min(chunk, count - k0);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_ids, meta.data() + k0, B * 4, hipMemcpyHostToDevice, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_cidx, meta.data() + count + k0, B * 4, hipMemcpyHostToDevice, st));
        const Fr *src = (const Fr *)((const uint8_t *)cells + k0 * l * 32);
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_cells, src, B * l * 32, hipMemcpyHostToDevice, st));
            src = d_cells;
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(raw, (const uint8_t *)proofs + k0 * psz, B * psz, hipMemcpyHostToDevice, st));
        KZG_TRY(decode_points(ctx, st, raw, B, pfmt, W, bad, untrusted_level(ctx)));
        KZG_TRY(vc_interp(ctx, st, plan, src, d_ids, B, d_r));
        KZG_TRY(vc_sum(ctx, st, plan, d_r, B, sfmt, R));
        KZG_LAUNCH(ctx, st, "k_vc_check", k_vc_check, vc_grid(B, 64), 64, 0, (const uint32_t *)d_ids, (const uint32_t *)d_cidx, log_l,
                   (const Fr *)plan->pos_lo, (const Fr *)plan->pos_hi, (const G1Xyzz *)C, (const G1Xyzz *)W, (const G1Xyzz *)R,
                   (const G2Affine *)plan->hq, (const Fq2 *)plan->lines, B, d_ok);
        KZG_TRY(fetch_ok(ctx, lane, d_ok, bad, B, verdict.data() + k0));  // synchronises: the chunk's buffers are free again
    }
    KZG_HIP_CHECK(ctx, hipGetLastError());
    memcpy(ok, verdict.data(), count);
    return KZG_OK;
}

#ifdef KZG_TEST_HOOKS
#include "../../include/kzg_mi355x_test.h"
// stage 0: in = count x l cell values (sfmt) of the cosets coset_ids -> out = count x l interpolant coefficients (sfmt)
// stage 1: in = count x l scalars (sfmt) -> out = count points sum_j in[k l + j] gs[j], affine Montgomery
extern "C" int kzg_test_verify_cosets_stage(kzg_ctx *ctx, const kzg_cosets_verifier *plan, int stage, const size_t *coset_ids, const void *in,
                                            size_t count, int sfmt, void *out) {
    if (!ctx || !plan || !in || !out || !count || (stage != 0 && stage != 1) || (stage == 0 && !coset_ids)) return KZG_ERR_SHAPE;
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t l = (size_t)1 << plan->log_l, K = (size_t)1 << (plan->log_n - plan->log_l);
    std::vector<uint32_t> ids(count, 0);
    for (size_t k = 0; stage == 0 && k < count; k++) {
        if (coset_ids[k] >= K) return fail(ctx, KZG_ERR_SHAPE, "coset id >= K");
        ids[k] = (uint32_t)coset_ids[k];
    }
    KZG_TRY(lane_reserve(ctx, 0, count * (4 + 2 * l * 32 + sizeof(G1Xyzz) + sizeof(G1Affine)) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    uint32_t *d_ids = (uint32_t *)lane_alloc(ctx, 0, count * 4);
    Fr *d_in = (Fr *)lane_alloc(ctx, 0, count * l * 32), *d_r = (Fr *)lane_alloc(ctx, 0, count * l * 32);
    G1Xyzz *R = (G1Xyzz *)lane_alloc(ctx, 0, count * sizeof(G1Xyzz));
    G1Affine *A = (G1Affine *)lane_alloc(ctx, 0, count * sizeof(G1Affine));
    if (!d_ids || !d_in || !d_r || !R || !A) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_ids, ids.data(), count * 4, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, in, count * l * 32, hipMemcpyHostToDevice, st));
    if (stage == 0) {
        KZG_TRY(vc_interp(ctx, st, plan, d_in, d_ids, count, d_r));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, d_r, count * l * 32, hipMemcpyDeviceToHost, st));
    } else {
        KZG_TRY(vc_sum(ctx, st, plan, d_in, count, sfmt, R));
        KZG_TRY(batch_to_affine(ctx, st, R, A, count));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, A, count * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}
// pretend the plan / the G2 points are resident on GPU `device` (the "another GPU" errors on a one-GPU box)
extern "C" int kzg_test_cosets_verifier_set_device(kzg_cosets_verifier *plan, int device) {
    if (!plan) return KZG_ERR_SHAPE;
    plan->device = device;
    return KZG_OK;
}
extern "C" int kzg_test_srs_g2_set_device(kzg_srs_g2 *srs, int device) {
    if (!srs) return KZG_ERR_SHAPE;
    srs->device = device;
    return KZG_OK;
}
#endif
