// multiopen.hip -- the Fr kernels of the two-element multiproof (kzg_multiopen_* in capi.hip): N claims
// p_{m(k)}(z_k) = y_k at any number of points answered by one quotient commitment D = [g]_1 and one witness,
//   g(X) = sum_k r^k (p_{m(k)}(X) - y_k) / (X - z_k) = sum_u (F_u - Y_u) / (X - z_u),  F_u = sum_{k in u} r^k p_{m(k)},  Y_u = sum_{k in u} r^k y_k
// over the distinct points z_u.
//   k_fr_lincomb       out[j] (+)= sum_k weight[k] v[idx[k] d + j]: k_fr_fold (fold.hip) with arbitrary weights and gathered vectors
//   k_multiopen_accum  evaluation form, off the domain: g_j += sum_u (sum_{k in u} r^k f_{m(k),j} - Y_u) / (w^j - z_u) for a chunk of
//                      at most 16 distinct points in ONE pass: every input element is read once per claim that names it, every
//                      inverse once, and neither a quotient nor an F_u is written
//   k_multiopen_ysum   Y_u from the chunk's values where the evaluation stage left them (no host round trip): one block per point
//   k_multiopen_gather the values at points of the domain
// Both big kernels keep the fold's shape: one element per thread, blocks of 256, the elements of FOLD_U terms requested before the
// first is used.  weight[k], idx[k] and the claim ranges are indexed by loop counters alone: wave-uniform, read through the scalar
// cache, multiplied out of SGPRs as gamma is in the fold.  Weights are Montgomery and the maps linear: the output has the inputs' form.
// Inputs may be any 256-bit value (a caller's canonical scalars): they count as their residue, the oe_load rule of open_eval.hip.
#include <algorithm>

#include "common.h"

namespace kzg {

constexpr int FOLD_U = 4;  // terms whose elements a lane has requested before it uses the first (fold.hip)

__device__ __forceinline__ Fr mo_residue(Fr f) { return fr_residue(f); }  // any value below 2^256 < 3r as a residue below r (field.h)

// sum_{k0 <= k < k1} weight[k] v[idx[k] d + j] for the lane's j (p = v + j)
__device__ __forceinline__ Fr mo_terms(const Fr *p, size_t d, const uint32_t *idx, const Fr *weight, size_t k0, size_t k1, Fr acc) {
    size_t k = k0;
    for (; k + FOLD_U <= k1; k += FOLD_U) {
        Fr x[FOLD_U];
#pragma unroll
        for (int u = 0; u < FOLD_U; u++) x[u] = p[(size_t)idx[k + u] * d];
#pragma unroll
        for (int u = 0; u < FOLD_U; u++) acc = add(acc, mul(mo_residue(x[u]), weight[k + u]));
    }
    for (; k < k1; k++) acc = add(acc, mul(mo_residue(p[(size_t)idx[k] * d]), weight[k]));
    return acc;
}

// grid ceil(d / 256)
__global__ __launch_bounds__(256) void k_fr_lincomb(const Fr *v, size_t d, const uint32_t *idx, const Fr *weight, size_t count, int carry, Fr *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d) return;
    out[j] = mo_terms(v + j, d, idx, weight, 0, count, carry ? mo_residue(out[j]) : Fr::zero());
}

// grid ceil(d / 256); claims of point u: [pstart[u], pstart[u + 1]) of idx / w; inv[u d + j] = 1 / (w^j - z_u)
__global__ __launch_bounds__(256) void k_multiopen_accum(const Fr *v, size_t d, const uint32_t *idx, const Fr *w, const uint32_t *pstart, int nz,
                                                         const Fr *Y, const Fr *inv, Fr *g) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d) return;
    Fr acc = g[j];
    for (int u = 0; u < nz; u++) {
        const Fr iv = inv[(size_t)u * d + j];  // requested with the point's first elements
        const Fr s = mo_terms(v + j, d, idx, w, pstart[u], pstart[u + 1], Fr::zero());
        acc = add(acc, mul(sub(s, Y[u]), iv));
    }
    g[j] = acc;
}

// one block of 64 threads per point of the chunk: the point's claims strided over the lanes, then a tree over LDS (a point may carry
// thousands of claims)
__global__ __launch_bounds__(64) void k_multiopen_ysum(const Fr *y, const Fr *w, const uint32_t *pstart, Fr *Y) {
    __shared__ Fr sh[64];
    const int u = blockIdx.x, t = threadIdx.x;
    Fr acc = Fr::zero();
    for (uint32_t k = pstart[u] + t; k < pstart[u + 1]; k += 64) acc = add(acc, mul(mo_residue(y[k]), w[k]));
    sh[t] = acc;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (t < off) sh[t] = add(sh[t], sh[t + off]);
        __syncthreads();
    }
    if (t == 0) Y[u] = sh[0];
}

__global__ __launch_bounds__(256) void k_multiopen_gather(const Fr *v, size_t d, const uint32_t *idx, const uint32_t *at, size_t count, Fr *y) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= count) return;
    y[s] = v[(size_t)idx[s] * d + at[s]];
}

int lincomb_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const Fr *d_weight, size_t count, bool carry,
                Fr *d_out) {
    if (!d) return KZG_OK;
    const size_t nblk = (d + 255) / 256;
    if (nblk > 0x7fffffffu) return fail(ctx, KZG_ERR_SHAPE, "lincomb: vectors too long");
    KZG_LAUNCH(ctx, st, "k_fr_lincomb", k_fr_lincomb, (unsigned)nblk, 256, 0, d_v, d, d_idx, d_weight, count, carry ? 1 : 0, d_out);
    return KZG_OK;
}

int multiopen_gather_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const uint32_t *d_at, size_t count, Fr *d_y) {
    if (!count) return KZG_OK;
    KZG_LAUNCH(ctx, st, "k_multiopen_gather", k_multiopen_gather, (unsigned)((count + 255) / 256), 256, 0, d_v, d, d_idx, d_at, count, d_y);
    return KZG_OK;
}

int multiopen_accum_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const Fr *d_w, const uint32_t *d_pstart,
                        int nz, const Fr *d_y, Fr *d_Y, const Fr *d_inv, Fr *d_g) {
    if (nz <= 0 || !d) return KZG_OK;
    if (nz > OE_MAX_CHUNK) return fail(ctx, KZG_ERR_INTERNAL, "multiopen chunk");
    KZG_LAUNCH(ctx, st, "k_multiopen_ysum", k_multiopen_ysum, (unsigned)nz, 64, 0, d_y, d_w, d_pstart, d_Y);
    KZG_LAUNCH(ctx, st, "k_multiopen_accum", k_multiopen_accum, (unsigned)((d + 255) / 256), 256, 0, d_v, d, d_idx, d_w, d_pstart, nz,
               (const Fr *)d_Y, d_inv, d_g);
    return KZG_OK;
}

}  // namespace kzg
