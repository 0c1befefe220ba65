// open_eval.hip -- an evaluation-form polynomial opened at ANY point z of Fr, for a batch of polynomials, in Fr (the MSM against
// the Lagrange SRS is the caller's: kzg_open_eval in capi.hip).  With f_i = p(w^i), i < d = 2^k:
//   z off the domain    y = (z^d - 1)/d  sum_i f_i w^i / (z - w^i)         (barycentric form over the roots of unity)
//                       q_i = (f_i - y) / (w^i - z)                        (the values of (p - y)/(X - z) on the domain)
//   z = w^m             y = f_m and q is div_by_omega_i of (f - f_m): quotient_eval_run (poly.hip), unchanged
// Which case a point is in is decided on the host (open_point_classify): no zero denominator reaches the batch inversion.
// The kernels are batch-wide: blockIdx.y is the polynomial of the chunk.  A chunk holds at most OE_MAX_CHUNK polynomials; the
// denominators w^i - z are formed and inverted once per DISTINCT z of the chunk (a batch that shares one challenge pays once).
//   w^i / (w^i - z) = 1 + z / (w^i - z), so sum_i f_i w^i inv_i = sum_i f_i + z sum_i f_i inv_i with inv_i = 1 / (w^i - z): the
//   evaluation pass takes one product per element and reads no power table (the trick of k_eval_quotient).
// Every constant is in Montgomery form and every map f -> y, f -> q is linear: the outputs have the form the evaluations have.
#include <algorithm>

#include "common.h"

namespace kzg {

constexpr int OE_LO_LOG = 10, OE_LO = 1 << OE_LO_LOG;  // w^i = lo[i mod 1024] hi[i / 1024]: two tables of 1024 and max(1, d / 1024) powers, built per call

struct OpenZs {  // the distinct off-domain points of a chunk
    Fr z[OE_MAX_CHUNK];  // Montgomery
    Fr c[OE_MAX_CHUNK];  // (z^d - 1) / d
};
struct OpenMap {  // polynomial of the chunk -> its distinct point, -1 = on the domain (not this file's kernels' business)
    int u[OE_MAX_CHUNK];
};

// tab[j] = w^j for j < OE_LO, tab[OE_LO + j] = w^(OE_LO j) for j < hi_n
__global__ __launch_bounds__(256) void k_open_powtab(Fr w, Fr w_hi, uint32_t hi_n, Fr *tab) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= OE_LO + hi_n) return;
    tab[j] = j < OE_LO ? pow_u64(w, (uint64_t)j) : pow_u64(w_hi, (uint64_t)(j - OE_LO));
}

// den[u d + i] = w^i - z_u, u < nz
__global__ __launch_bounds__(256) void k_open_denoms(const Fr *tab, size_t d, OpenZs zs, int nz, Fr *den) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    Fr w = mul(tab[i & (OE_LO - 1)], tab[OE_LO + (i >> OE_LO_LOG)]);
    for (int u = 0; u < nz; u++) den[(size_t)u * d + i] = sub(w, zs.z[u]);
}

// a caller's scalar (any value below 2^256 < 3r in the canonical format) as a residue below r
__device__ __forceinline__ Fr oe_load(const Fr *p) { return fr_residue(*p); }

// the sums of a and of b over the block (256 threads), in every thread
__device__ __forceinline__ void block_sum2(Fr &a, Fr &b, Fr *sh) {
    const int t = threadIdx.x;
    sh[t] = a;
    sh[256 + t] = b;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            sh[t] = add(sh[t], sh[t + off]);
            sh[256 + t] = add(sh[256 + t], sh[256 + t + off]);
        }
        __syncthreads();
    }
    a = sh[0];
    b = sh[256];
    __syncthreads();
}

// partial[b nblk + block] = sum_{i in block} f_i w^i / (w^i - z) = sum f_i + z sum f_i inv_i
__global__ __launch_bounds__(256) void k_open_eval_partials(const Fr *evals, size_t d, const Fr *inv, OpenZs zs, OpenMap map, Fr *partial) {
    __shared__ Fr sh[512];
    const int b = blockIdx.y, u = map.u[b];
    if (u < 0) return;  // uniform: an on-domain polynomial
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr f = Fr::zero(), g = Fr::zero();
    if (i < d) {
        f = oe_load(evals + (size_t)b * d + i);
        g = mul(f, inv[(size_t)u * d + i]);
    }
    block_sum2(f, g, sh);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = add(f, mul(zs.z[u], g));
}

// y_b = -(z^d - 1)/d  sum partial: the sum above runs over 1 / (w^i - z), the formula over 1 / (z - w^i)
__global__ __launch_bounds__(256) void k_open_eval_finish(const Fr *partial, uint32_t nblk, OpenZs zs, OpenMap map, Fr *y) {
    __shared__ Fr sh[512];
    const int b = blockIdx.x, u = map.u[b];
    if (u < 0) return;
    Fr acc = Fr::zero(), none = Fr::zero();
    for (uint32_t k = threadIdx.x; k < nblk; k += blockDim.x) acc = add(acc, partial[(size_t)b * nblk + k]);
    block_sum2(acc, none, sh);
    if (threadIdx.x == 0) y[b] = neg(mul(zs.c[u], acc));
}

// q_i = (f_i - y_b) / (w^i - z); y_b comes from device memory (no host round trip behind the evaluation)
__global__ __launch_bounds__(256) void k_open_quotient(const Fr *evals, size_t d, const Fr *inv, OpenMap map, const Fr *y, Fr *q) {
    const int b = blockIdx.y, u = map.u[b];
    if (u < 0) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    q[(size_t)b * d + i] = mul(sub(oe_load(evals + (size_t)b * d + i), y[b]), inv[(size_t)u * d + i]);
}

// y = f_m for a point of the domain: the caller's word taken to its residue (a plain copy would hand a word >= r back as the value)
__global__ __launch_bounds__(64) void k_open_value_on_domain(const Fr *f_m, Fr *y) {
    if (threadIdx.x == 0) *y = oe_load(f_m);
}

// The two evaluation kernels with an indirection (kzg_multiopen_eval_commit): claim b of the launch names its polynomial, vidx[b], and
// its point of the chunk, pu[b]; the tables and the points' constants are device memory, read uniformly per block.
__global__ __launch_bounds__(256) void k_open_eval_partials_idx(const Fr *evals, size_t d, const Fr *inv, const uint32_t *vidx, const uint32_t *pu,
                                                                const Fr *z, Fr *partial) {
    __shared__ Fr sh[512];
    const size_t b = blockIdx.y, u = pu[b];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr f = Fr::zero(), g = Fr::zero();
    if (i < d) {
        f = oe_load(evals + (size_t)vidx[b] * d + i);
        g = mul(f, inv[u * d + i]);
    }
    block_sum2(f, g, sh);
    if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = add(f, mul(z[u], g));
}

__global__ __launch_bounds__(256) void k_open_eval_finish_idx(const Fr *partial, uint32_t nblk, const uint32_t *pu, const Fr *c, Fr *y) {
    __shared__ Fr sh[512];
    const size_t b = blockIdx.x;
    Fr acc = Fr::zero(), none = Fr::zero();
    for (uint32_t k = threadIdx.x; k < nblk; k += blockDim.x) acc = add(acc, partial[b * nblk + k]);
    block_sum2(acc, none, sh);
    if (threadIdx.x == 0) y[b] = neg(mul(c[pu[b]], acc));
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// z^d == 1 <=> z = w^m.  s_j = z^(2^j) (k squarings); bit j of m is read from s_(k-1-j) = rho_j^(m mod 2^(j+1)) with
// rho_j = w^(2^(k-1-j)) a primitive 2^(j+1)-th root: it is rho_j^(m mod 2^j) for a zero bit and minus that for a one.  The powers
// rho_j^(2^i) are the roots rho_(j-i) themselves, so a level costs one product per bit already set and the whole walk no table.
int open_point_classify(uint32_t log_d, const Fr &z_mont, OpenPoint *pt) {
    const uint32_t k = log_d;
    Fr s[FR_TWO_ADICITY + 1], rho[FR_TWO_ADICITY + 1];
    s[0] = z_mont;
    for (uint32_t j = 0; j < k; j++) s[j + 1] = sqr(s[j]);
    pt->z = z_mont;
    pt->m = 0;
    pt->on_domain = s[k] == Fr::one();
    if (!pt->on_domain) {
        pt->c = mul(sub(s[k], Fr::one()), inv(from_u64<FrParams>((uint64_t)1 << k)));
        return KZG_OK;
    }
    pt->c = Fr::zero();
    if (k == 0) return KZG_OK;
    rho[k - 1] = host_omega(log_d);
    for (uint32_t j = k - 1; j > 0; j--) rho[j - 1] = sqr(rho[j]);  // rho[0] = -1
    size_t m = 0;
    for (uint32_t j = 0; j < k; j++) {
        Fr e = Fr::one();
        for (uint32_t i = 0; i < j; i++)
            if ((m >> i) & 1) e = mul(e, rho[j - i]);
        const Fr &v = s[k - 1 - j];
        if (v == e) continue;
        if (v != neg(e)) return KZG_ERR_INTERNAL;
        m |= (size_t)1 << j;
    }
    if (pow_u64(host_omega(log_d), (uint64_t)m) != z_mont) return KZG_ERR_INTERNAL;
    pt->m = m;
    return KZG_OK;
}

size_t open_eval_fr_workspace_bytes(size_t d, size_t B, size_t nz) {
    const size_t hi_n = std::max<size_t>(1, d >> OE_LO_LOG), nblk = (d + 255) / 256;
    // the power tables | denominators and inverses (one set per distinct point) | block partials of both paths | slack for alignment
    return align_up((OE_LO + hi_n) * 32, 256) + 2 * align_up(nz * d * 32, 256) + 2 * align_up(B * nblk * 32 + 256, 256) + 8192;
}
size_t open_eval_fr_workspace_bytes(size_t d, size_t B) { return open_eval_fr_workspace_bytes(d, B, B); }  // at most one point per polynomial

// One chunk on the lane's stream: y (and q unless d_q is null) of B <= OE_MAX_CHUNK polynomials, polynomial b at d_evals + b d,
// its quotient at d_q + b d, its value at d_y + b.  Takes its scratch from the lane's arena and gives it back (stream order
// makes the next chunk's re-use safe).
int open_eval_fr_run(kzg_ctx *ctx, int lane, const Fr *d_evals, uint32_t log_d, size_t B, const OpenPoint *pts, int sfmt, Fr *d_y, Fr *d_q) {
    if (B == 0) return KZG_OK;
    if (B > (size_t)OE_MAX_CHUNK) return fail(ctx, KZG_ERR_INTERNAL, "open_eval chunk");
    hipStream_t st = ctx->lanes[lane].stream;
    const size_t d = (size_t)1 << log_d, mark = ctx->lanes[lane].arena_used;
    const uint32_t nblk = (uint32_t)((d + 255) / 256), hi_n = (uint32_t)std::max<size_t>(1, d >> OE_LO_LOG);
    OpenZs zs;
    OpenMap map;
    int nz = 0;
    for (size_t b = 0; b < B; b++) {
        map.u[b] = -1;
        if (pts[b].on_domain) continue;
        int u = 0;
        while (u < nz && zs.z[u] != pts[b].z) u++;
        if (u == nz) {
            zs.z[nz] = pts[b].z;
            zs.c[nz] = pts[b].c;
            nz++;
        }
        map.u[b] = u;
    }
    for (int u = nz; u < OE_MAX_CHUNK; u++) zs.z[u] = zs.c[u] = Fr::zero();
    for (size_t b = B; b < (size_t)OE_MAX_CHUNK; b++) map.u[b] = -1;
    int rc = KZG_OK;
    if (nz) {
        Fr *tab = (Fr *)lane_alloc(ctx, lane, (size_t)(OE_LO + hi_n) * 32);
        Fr *den = (Fr *)lane_alloc(ctx, lane, (size_t)nz * d * 32), *iv = (Fr *)lane_alloc(ctx, lane, (size_t)nz * d * 32);
        Fr *partial = (Fr *)lane_alloc(ctx, lane, B * nblk * 32);
        if (!tab || !den || !iv || !partial) return fail(ctx, KZG_ERR_ALLOC, "open_eval workspace not reserved");
        const Fr w = host_omega(log_d);
        KZG_LAUNCH(ctx, st, "k_open_powtab", k_open_powtab, (OE_LO + hi_n + 255) / 256, 256, 0, w, pow_u64(w, (uint64_t)OE_LO), hi_n, tab);
        KZG_LAUNCH(ctx, st, "k_open_denoms", k_open_denoms, nblk, 256, 0, (const Fr *)tab, d, zs, nz, den);
        KZG_TRY(batch_inverse(ctx, st, den, iv, (size_t)nz * d));
        KZG_LAUNCH(ctx, st, "k_open_eval_partials", k_open_eval_partials, dim3(nblk, (unsigned)B), 256, 0, d_evals, d, (const Fr *)iv, zs, map, partial);
        KZG_LAUNCH(ctx, st, "k_open_eval_finish", k_open_eval_finish, (unsigned)B, 256, 0, (const Fr *)partial, nblk, zs, map, d_y);
        if (d_q) KZG_LAUNCH(ctx, st, "k_open_quotient", k_open_quotient, dim3(nblk, (unsigned)B), 256, 0, d_evals, d, (const Fr *)iv, map, (const Fr *)d_y, d_q);
    }
    for (size_t b = 0; b < B && rc == KZG_OK; b++) {
        if (!pts[b].on_domain) continue;
        KZG_LAUNCH(ctx, st, "k_open_value_on_domain", k_open_value_on_domain, 1, 64, 0, d_evals + b * d + pts[b].m, d_y + b);
        if (d_q) rc = quotient_eval_run(ctx, lane, d_evals + b * d, log_d, pts[b].m, sfmt, d_q + b * d);
    }
    ctx->lanes[lane].arena_used = mark;
    return rc;
}

// ---- the stages above for a caller with its own tables (kzg_multiopen_eval_commit) ----
size_t open_powtab_bytes(size_t d) { return (OE_LO + std::max<size_t>(1, d >> OE_LO_LOG)) * 32; }

int open_powtab_run(kzg_ctx *ctx, hipStream_t st, uint32_t log_d, Fr *d_tab) {
    const uint32_t hi_n = (uint32_t)std::max<size_t>(1, ((size_t)1 << log_d) >> OE_LO_LOG);
    const Fr w = host_omega(log_d);
    KZG_LAUNCH(ctx, st, "k_open_powtab", k_open_powtab, (OE_LO + hi_n + 255) / 256, 256, 0, w, pow_u64(w, (uint64_t)OE_LO), hi_n, d_tab);
    return KZG_OK;
}

int open_inverses_run(kzg_ctx *ctx, hipStream_t st, uint32_t log_d, const Fr *d_tab, const Fr *z_mont, int nz, Fr *d_den, Fr *d_inv) {
    if (nz <= 0) return KZG_OK;
    if (nz > OE_MAX_CHUNK) return fail(ctx, KZG_ERR_INTERNAL, "open_eval chunk");
    const size_t d = (size_t)1 << log_d;
    OpenZs zs;
    for (int u = 0; u < OE_MAX_CHUNK; u++) {
        zs.z[u] = u < nz ? z_mont[u] : Fr::zero();
        zs.c[u] = Fr::zero();  // (k_open_denoms reads the points alone)
    }
    KZG_LAUNCH(ctx, st, "k_open_denoms", k_open_denoms, (unsigned)((d + 255) / 256), 256, 0, d_tab, d, zs, nz, d_den);
    return batch_inverse(ctx, st, d_den, d_inv, (size_t)nz * d);
}

int open_eval_values_idx_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_evals, uint32_t log_d, const Fr *d_inv, const uint32_t *d_vidx,
                             const uint32_t *d_pu, const Fr *d_z, const Fr *d_c, size_t B, Fr *d_partial, Fr *d_y) {
    const size_t d = (size_t)1 << log_d;
    const uint32_t nblk = (uint32_t)((d + 255) / 256);
    for (size_t b0 = 0; b0 < B; b0 += 65535) {  // (gridDim.y); d_partial: min(B, 65535) x nblk scalars
        const size_t n = std::min<size_t>(65535, B - b0);
        KZG_LAUNCH(ctx, st, "k_open_eval_partials_idx", k_open_eval_partials_idx, dim3(nblk, (unsigned)n), 256, 0, d_evals, d, d_inv, d_vidx + b0,
                   d_pu + b0, d_z, d_partial);
        KZG_LAUNCH(ctx, st, "k_open_eval_finish_idx", k_open_eval_finish_idx, (unsigned)n, 256, 0, (const Fr *)d_partial, nblk, d_pu + b0, d_c, d_y + b0);
    }
    return KZG_OK;
}

}  // namespace kzg
