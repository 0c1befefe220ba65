// recover.hip -- kzg_recover_cosets: a polynomial of at most n coefficients from any `known` of the K = N / l cosets
// C_i = { w^(i + tK) : t < l } of its size-N domain with known l >= n (erasure recovery; Fr only, no SRS).  Not a reference method.
//
// With M the ids of the missing cosets, m = |M|, nu = w^l (a primitive K-th root of unity):
//   Z(X) = prod_{i in M} (X^l - nu^i) = Zs(X^l),  Zs(Y) = prod_{i in M} (Y - nu^i)   -- Z(w^j) = Zs(nu^(j mod K)): constant on a coset
//   1. E Z on the domain: every known cell times the one factor Zs(nu^id), zero on the missing cosets       (k_rec_scatter)
//   2. iNTT_N: the coefficients of p Z exactly (deg <= n - 1 + m l < N); the cells are values of a polynomial of fewer than n
//      coefficients iff coefficients [n + m l, N) vanish                                                    (k_rec_check)
//   3. p Z on the coset 7 H (Z has no root there: 7^l nu^j is not a K-th root of unity), times 1 / Zs(7^l nu^(j mod K)), back
//      to coefficients: p                                                                        (k_rec_divide, k_rec_emit)
// What depends on the id set alone -- Zs, its values on the K-th roots of unity and the K inverses on the coset -- is built once
// per call, before the chunk loop.
//
// Zs in O(m log^2 m): a product tree over the roots, padded with zero roots (factors Y) to Mpad = REC_LEAF 2^k.  A monic
// polynomial of degree d is kept as its d low coefficients (the leading 1 is implicit), so a level of the tree is one array of
// Mpad elements whatever its degree.  Leaves: one workgroup multiplies REC_LEAF linear factors in LDS (k_rec_leaf).  A level
// multiplies pairs a = Y^d + a', b = Y^d + b':  a b = Y^2d + Y^d (a' + b') + a' b', and a' b' (degree <= 2d - 2) is a cyclic
// product of size S = 2d that does not wrap.  ALL pairs of a level are transformed together: a decimation-in-frequency transform
// forward (natural in, bit-reversed out), the pointwise product, a decimation-in-time transform back (bit-reversed in, natural
// out), so no permutation pass exists.  S <= 1024: one workgroup per pair does all of it in LDS (k_rec_mul_small).  Larger S:
// radix-2 stages over the whole level in global memory while the butterfly span exceeds an LDS tile (k_rec_stage), the remaining
// 11 stages per 2048-element tile in LDS (k_rec_tile).  The launch count depends on log(Mpad) only: roots, leaves, the twiddle
// table, one launch for each of the two small levels and 5 + 2 (s - 11) for a level of 2^s >= 2^11 points -- 122 launches at
// Mpad = 2^19 (2^20 / l = 1, half the points missing).
#include <algorithm>
#include <new>
#include <vector>

#include "common.h"

namespace kzg {

constexpr uint32_t REC_LEAF = 256;          // roots per leaf workgroup (tests/recover_model.py LEAF)
constexpr uint32_t REC_SMALL_LOG = 10;      // products of up to 2^10 points: both operands of a pair in one workgroup's LDS
constexpr uint32_t REC_TILE_LOG = 11;       // LDS tile of the larger transforms: 2048 x 32 B = 64 KiB
constexpr uint32_t REC_MAX_LOG = 22;        // the FK20 plans' limit: what is recovered can be opened
// polynomials per chunk: the rule of fk20_run (g1ntt.hip), max(1, min(4096, 2^21 / 2N))
constexpr size_t REC_MAX_CHUNK = 4096, REC_CHUNK_POINTS = (size_t)1 << 21;

static inline unsigned rec_grid(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

// roots[i] = nu^miss[i] (nu^id = hi[id >> 10] lo[id & 1023]) for i < m, zero up to mpad
__global__ __launch_bounds__(256) void k_rec_roots(const uint32_t *miss, size_t m, size_t mpad, const Fr *lo, const Fr *hi, Fr *roots) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mpad) return;
    Fr r = Fr::zero();
    if (i < m) {
        const uint32_t id = miss[i];
        r = mul(hi[id >> 10], lo[id & 1023]);
    }
    roots[i] = r;
}

// out[b L .. (b + 1) L) = the L low coefficients of prod_{i < L} (Y - roots[b L + i]); thread j owns coefficient j
__global__ __launch_bounds__(REC_LEAF) void k_rec_leaf(const Fr *roots, Fr *out) {
    __shared__ Fr c[REC_LEAF];
    const uint32_t j = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * REC_LEAF;
    c[j] = Fr::zero();
    __syncthreads();
    for (uint32_t i = 0; i < REC_LEAF; i++) {
        // (Y^i + sum_{k < i} c_k Y^k) (Y - r): c_j <- c_{j-1} - r c_j for j <= i, with c_i = 1
        const Fr r = roots[base + i];
        const Fr cj = j < i ? c[j] : Fr::one();
        const Fr cm = j >= 1 ? c[j - 1] : Fr::zero();
        __syncthreads();
        if (j <= i) c[j] = sub(cm, mul(r, cj));
        __syncthreads();
    }
    out[base + j] = c[j];
}

// w_2h^(+-j), j < h = 2^log_h, from tw[i] = w_T^i (i < T / 2, T = 2^log_t): w^-j = -w^(h - j)
__device__ __forceinline__ Fr rec_tw(const Fr *tw, uint32_t j, uint32_t log_h, uint32_t log_t, bool inverse) {
    const uint32_t sh = log_t - 1 - log_h;
    if (!inverse) return tw[(size_t)j << sh];
    if (j == 0) return Fr::one();
    return neg(tw[(size_t)((1u << log_h) - j) << sh]);
}

// one radix-2 butterfly of the stage with half span 2^log_h on pair p.  Forward (DIF): (u, v) -> (u + v, (u - v) w); inverse
// (DIT): (u, v) -> (u + v w^-1, u - v w^-1): the stages of one undo the stages of the other up to the factor 2
template <class Ptr>
__device__ __forceinline__ void rec_butterfly(Ptr x, size_t p, uint32_t log_h, const Fr *tw, uint32_t log_t, bool inverse) {
    const size_t h = (size_t)1 << log_h;
    const uint32_t j = (uint32_t)(p & (h - 1));
    const size_t i0 = ((p >> log_h) << (log_h + 1)) | j, i1 = i0 + h;
    const Fr w = rec_tw(tw, j, log_h, log_t, inverse);
    const Fr u = x[i0];
    if (!inverse) {
        const Fr v = x[i1];
        x[i0] = add(u, v);
        x[i1] = mul(sub(u, v), w);
    } else {
        const Fr v = mul(x[i1], w);
        x[i0] = add(u, v);
        x[i1] = sub(u, v);
    }
}

// a whole transform of 2^s points in LDS (y: a second array taken through the same stages, or nullptr)
__device__ __forceinline__ void rec_lds_ntt(Fr *x, Fr *y, uint32_t s, const Fr *tw, uint32_t log_t, bool inverse) {
    const size_t pairs = ((size_t)1 << s) >> 1;
    for (uint32_t st = 0; st < s; st++) {
        const uint32_t log_h = inverse ? st : s - 1 - st;
        for (size_t p = threadIdx.x; p < pairs; p += blockDim.x) {
            rec_butterfly(x, p, log_h, tw, log_t, inverse);
            if (y) rec_butterfly(y, p, log_h, tw, log_t, inverse);
        }
        __syncthreads();
    }
}

// one pair per workgroup, S = 2^s <= 1024: nxt[q S .. (q + 1) S) = low coefficients of (Y^d + a')(Y^d + b'), d = S / 2.  Dynamic
// LDS, 2 S elements (32 KiB at S = 512, 64 KiB at S = 1024): the smaller level is not charged for the larger one's arrays
extern __shared__ __attribute__((aligned(16))) uint4 rec_lds[];
__global__ __launch_bounds__(256) void k_rec_mul_small(const Fr *cur, Fr *nxt, uint32_t s, const Fr *tw, uint32_t log_t, Fr sinv) {
    const size_t S = (size_t)1 << s, d = S >> 1;
    Fr *A = (Fr *)rec_lds, *B = A + S;
    const Fr *a = cur + (size_t)blockIdx.x * S, *b = a + d;
    for (size_t k = threadIdx.x; k < S; k += blockDim.x) {
        A[k] = k < d ? a[k] : Fr::zero();
        B[k] = k < d ? b[k] : Fr::zero();
    }
    __syncthreads();
    rec_lds_ntt(A, B, s, tw, log_t, false);
    for (size_t k = threadIdx.x; k < S; k += blockDim.x) A[k] = mul(A[k], B[k]);
    __syncthreads();
    rec_lds_ntt(A, (Fr *)nullptr, s, tw, log_t, true);
    for (size_t k = threadIdx.x; k < S; k += blockDim.x) {
        Fr v = mul(A[k], sinv);
        if (k >= d) v = add(v, add(a[k - d], b[k - d]));  // Y^d (a' + b'); the Y^2d term is the implicit leading 1
        nxt[(size_t)blockIdx.x * S + k] = v;
    }
}

// f[i 2d + k] = cur[i d + k] for k < d, zero for d <= k < 2d: every polynomial of the level zero-padded to the product size
__global__ __launch_bounds__(256) void k_rec_pad(const Fr *cur, Fr *f, uint32_t log_d, size_t total) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t d = (size_t)1 << log_d, i = e >> (log_d + 1), k = e & (2 * d - 1);
    f[e] = k < d ? cur[(i << log_d) + k] : Fr::zero();
}

// one radix-2 stage over every array of the buffer at once (arrays of 2^(log_h + 1) or more points, contiguous)
__global__ __launch_bounds__(256) void k_rec_stage(Fr *x, size_t pairs, uint32_t log_h, const Fr *tw, uint32_t log_t, int inverse) {
    size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pairs) return;
    rec_butterfly(x, p, log_h, tw, log_t, inverse != 0);
}

// the stages with half span < 2^s of every 2^s-point tile of the buffer, in LDS (s <= REC_TILE_LOG)
__global__ __launch_bounds__(256) void k_rec_tile(Fr *x, uint32_t s, const Fr *tw, uint32_t log_t, int inverse) {
    __shared__ Fr sh[1 << REC_TILE_LOG];
    const size_t n = (size_t)1 << s;
    Fr *g = x + (size_t)blockIdx.x * n;
    for (size_t k = threadIdx.x; k < n; k += blockDim.x) sh[k] = g[k];
    __syncthreads();
    rec_lds_ntt(sh, (Fr *)nullptr, s, tw, log_t, inverse != 0);
    for (size_t k = threadIdx.x; k < n; k += blockDim.x) g[k] = sh[k];
}

// g[q S + k] = f[2q S + k] f[(2q + 1) S + k]
__global__ __launch_bounds__(256) void k_rec_pointwise(const Fr *f, Fr *g, uint32_t log_s, size_t total) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t q = e >> log_s, k = e & (((size_t)1 << log_s) - 1);
    g[e] = mul(f[((2 * q) << log_s) + k], f[((2 * q + 1) << log_s) + k]);
}

// nxt[q S + k] = g[q S + k] / S + (k >= d ? a'[k - d] + b'[k - d] : 0), a' = cur[q S ..), b' = cur[q S + d ..)
__global__ __launch_bounds__(256) void k_rec_combine(const Fr *g, const Fr *cur, Fr *nxt, uint32_t log_s, size_t total, Fr sinv) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t d = ((size_t)1 << log_s) >> 1, k = e & (2 * d - 1);
    Fr v = mul(g[e], sinv);
    if (k >= d) v = add(v, add(cur[e - d], cur[e]));
    nxt[e] = v;
}

// The tree's result is Y^pad Zs(Y) without its leading 1: Zs's m + 1 coefficients zero-padded to K, twice (for its values on
// the K-th roots of unity and on their coset)
__global__ __launch_bounds__(256) void k_rec_zs_load(const Fr *t, size_t pad, size_t m, size_t K, Fr *zv, Fr *zc) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    const Fr v = j < m ? t[pad + j] : (j == m ? Fr::one() : Fr::zero());
    zv[j] = v;
    zc[j] = v;
}

// work[b N + id_j + t K] = cells[(b known + j) l + t] Zs(nu^id_j) (Montgomery), zero on the missing cosets.  The cells of a
// polynomial are one contiguous run, and thread g reads element g of it: the loads are the coalesced side, the stores go out
// with stride K along t.  The zeros are written with the coset id running fastest (adjacent ids: adjacent addresses).  One
// polynomial per blockIdx.y, so every index inside it fits 32 bits (N <= 2^22) and the one division left is a 32-bit one.
__global__ __launch_bounds__(256) void k_rec_scatter(const Fr *cells, uint32_t log_n, uint32_t log_l, uint32_t known, const uint32_t *ids,
                                                     const uint32_t *miss, const Fr *zv, int to_m, Fr *work) {
    const uint32_t N = 1u << log_n, l = 1u << log_l, kl = known << log_l, log_k = log_n - log_l;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    Fr *out = work + ((size_t)blockIdx.y << log_n);
    if (g < kl) {
        const uint32_t id = ids[g >> log_l];
        Fr v = cells[(size_t)blockIdx.y * kl + g];
        if (to_m) v = to_mont(v);
        out[id + ((g & (l - 1)) << log_k)] = mul(v, zv[id]);
    } else {
        const uint32_t m = (N >> log_l) - known, h = g - kl, t = h / m;
        out[miss[h - t * m] + (t << log_k)] = Fr::zero();
    }
}

// flags[b] |= 1 if a coefficient [lo, N) of polynomial b = blockIdx.y is non-zero
__global__ __launch_bounds__(256) void k_rec_check(const Fr *work, uint32_t log_n, uint32_t lo, int *flags) {
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << log_n)) return;
    if (!work[((size_t)blockIdx.y << log_n) + i].is_zero()) atomicOr(flags + blockIdx.y, 1);
}

// work[b N + j] *= zinv[j mod K]
__global__ __launch_bounds__(256) void k_rec_divide(Fr *work, size_t total, const Fr *zinv, size_t kmask) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) work[e] = mul(work[e], zinv[e & kmask]);
}

// coefficients [0, n) of every polynomial in the caller's format: to coeffs (stride n) and / or, zero-padded to N, to ev (stride
// N; may be `work` itself)
__global__ __launch_bounds__(256) void k_rec_emit(const Fr *work, uint32_t log_n, size_t n, size_t batch, int from_m, Fr *coeffs, Fr *ev) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= batch << log_n) return;
    const size_t b = e >> log_n, i = e & (((size_t)1 << log_n) - 1);
    Fr v = Fr::zero();
    if (i < n) {
        v = work[e];
        if (from_m) v = from_mont(v);
        if (coeffs) coeffs[b * n + i] = v;
    }
    if (ev) ev[e] = v;
}

// Zs from the ids of the missing cosets: zs[0, mpad) = the low coefficients of Y^(mpad - m) Zs(Y).  roots, t0, t1, g: mpad
// elements each, f: 2 mpad, tw: mpad / 2
static int rec_zero_poly(kzg_ctx *ctx, hipStream_t st, const uint32_t *d_miss, size_t m, size_t mpad, const Fr *lo, const Fr *hi,
                         Fr *roots, Fr *t0, Fr *t1, Fr *f, Fr *g, Fr *tw, Fr **zs) {
    const uint32_t log_t = (uint32_t)ilog2_ceil(mpad);
    KZG_LAUNCH(ctx, st, "k_rec_roots", k_rec_roots, rec_grid(mpad), 256, 0, d_miss, m, mpad, lo, hi, roots);
    KZG_LAUNCH(ctx, st, "k_rec_leaf", k_rec_leaf, (unsigned)(mpad / REC_LEAF), REC_LEAF, 0, (const Fr *)roots, t0);
    if (mpad > REC_LEAF) KZG_TRY(pow_table(ctx, st, host_omega(log_t), Fr::one(), mpad / 2, tw));
    Fr *cur = t0, *nxt = t1;
    for (uint32_t s = (uint32_t)ilog2_ceil(REC_LEAF) + 1; s <= log_t; s++) {  // products of S = 2^s points
        const Fr sinv = inv(from_u64<FrParams>((uint64_t)1 << s));
        if (s <= REC_SMALL_LOG) {
            KZG_LAUNCH(ctx, st, "k_rec_mul_small", k_rec_mul_small, (unsigned)(mpad >> s), 256, (2 * sizeof(Fr)) << s, (const Fr *)cur, nxt, s, (const Fr *)tw,
                       log_t, sinv);
        } else {
            const uint32_t tile = REC_TILE_LOG;  // s >= 11
            KZG_LAUNCH(ctx, st, "k_rec_pad", k_rec_pad, rec_grid(2 * mpad), 256, 0, (const Fr *)cur, f, s - 1, 2 * mpad);
            for (uint32_t lh = s - 1; lh >= tile; lh--)
                KZG_LAUNCH(ctx, st, "k_rec_stage", k_rec_stage, rec_grid(mpad), 256, 0, f, mpad, lh, (const Fr *)tw, log_t, 0);
            KZG_LAUNCH(ctx, st, "k_rec_tile", k_rec_tile, (unsigned)((2 * mpad) >> tile), 256, 0, f, tile, (const Fr *)tw, log_t, 0);
            KZG_LAUNCH(ctx, st, "k_rec_pointwise", k_rec_pointwise, rec_grid(mpad), 256, 0, (const Fr *)f, g, s, mpad);
            KZG_LAUNCH(ctx, st, "k_rec_tile", k_rec_tile, (unsigned)(mpad >> tile), 256, 0, g, tile, (const Fr *)tw, log_t, 1);
            for (uint32_t lh = tile; lh < s; lh++)
                KZG_LAUNCH(ctx, st, "k_rec_stage", k_rec_stage, rec_grid(mpad / 2), 256, 0, g, mpad / 2, lh, (const Fr *)tw, log_t, 1);
            KZG_LAUNCH(ctx, st, "k_rec_combine", k_rec_combine, rec_grid(mpad), 256, 0, (const Fr *)g, (const Fr *)cur, nxt, s, mpad, sinv);
        }
        std::swap(cur, nxt);
    }
    *zs = cur;
    return KZG_OK;
}

// `count` transforms of 2^log_n points, transform i at d + i 2^log_n; shift 7 (coset) or none.  Each takes its scratch from the
// arena mark again: they are ordered on the lane's stream (as ntt_each in g1ntt.hip)
static int rec_ntt_each(kzg_ctx *ctx, int lane, size_t mark, Fr *d, size_t count, uint32_t log_n, int inverse, bool coset) {
    const Fr g7 = from_u64<FrParams>(FR_MULT_GENERATOR);
    for (size_t i = 0; i < count; i++) {
        ctx->lanes[lane].arena_used = mark;
        Fr *x = d + (i << log_n);
        if (coset) KZG_TRY(coset_ntt_run(ctx, lane, x, log_n, inverse, g7));
        else KZG_TRY(ntt_run(ctx, lane, x, log_n, inverse));
    }
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_recover_cosets(kzg_ctx *ctx, uint32_t log_n, uint32_t log_l, size_t n, const size_t *coset_ids, size_t known,
                                  const void *cells, size_t batch, int sfmt, int flags, void *out_coeffs, void *out_evals, int *status) {
    // ---- shape: everything is decided before memory is touched or a kernel launched ----
    if (!ctx) return KZG_ERR_SHAPE;
    if (log_n > REC_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: log_n <= 22 (the FK20 plans' limit)");
    if (log_l > log_n) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: coset larger than the domain");
    const size_t N = (size_t)1 << log_n, l = (size_t)1 << log_l, K = N >> log_l;
    const uint32_t log_k = log_n - log_l;
    if (n == 0 || n > N) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: 1 <= n <= N");
    if (known == 0 || known > K) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: 1 <= known <= K");
    if (known * l < n) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: known * l < n (too few cosets for n coefficients)");
    if (!coset_ids || !cells) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: NULL coset_ids or cells");
    if (!out_coeffs && !out_evals) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: no output");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    std::vector<uint32_t> ids, miss;
    try {  // (no exception may leave through the C ABI)
        ids.resize(known);
        std::vector<uint8_t> seen(K, 0);
        for (size_t j = 0; j < known; j++) {
            if (coset_ids[j] >= K) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: coset id >= K");
            if (seen[coset_ids[j]]) return fail(ctx, KZG_ERR_SHAPE, "kzg_recover_cosets: duplicate coset id");
            seen[coset_ids[j]] = 1;
            ids[j] = (uint32_t)coset_ids[j];
        }
        miss.reserve(K - known);
        for (size_t i = 0; i < K; i++)
            if (!seen[i]) miss.push_back((uint32_t)i);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "kzg_recover_cosets: host memory for the coset ids");
    }
    if (batch == 0) return KZG_OK;
    if (batch > SIZE_MAX / (N * 32)) return fail(ctx, KZG_ERR_SHAPE, "batch too large");
    const size_t m = K - known;
    size_t mpad = REC_LEAF;
    while (mpad < m) mpad *= 2;

    kzg::Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const int canonical = sfmt == KZG_FR_CANONICAL_LE_32;
    const size_t chunk = std::max<size_t>(1, std::min(REC_MAX_CHUNK, REC_CHUNK_POINTS / (2 * N)));
    const size_t B0 = std::min(chunk, batch), kl = known * l;
    const size_t hi_n = std::max<size_t>(1, K >> 10);

    // arena: what the whole call keeps | the larger of the tree's scratch and a chunk's buffers (the chunks start where the tree did)
    const size_t keep = align_up(known * 4, 256) + align_up((m ? m : 1) * 4, 256) + 2 * align_up(K * 32, 256) + align_up(B0 * 4, 256);
    const size_t tree = 6 * align_up(mpad * 32, 256) + align_up(mpad * 16, 256) + align_up(K * 32, 256) + align_up((1024 + hi_n) * 32, 256) +
                        ntt_workspace_bytes(log_k);
    const size_t per_chunk = align_up(B0 * N * 32, 256) + (in_dev ? 0 : align_up(B0 * kl * 32, 256)) +
                             ((out_dev || !out_coeffs) ? 0 : align_up(B0 * n * 32, 256)) + ntt_workspace_bytes(log_n);
    KZG_TRY(lane_reserve(ctx, lane, keep + std::max(tree, per_chunk) + 65536));
    KZG_TRY(lane_pinned(ctx, lane, B0 * sizeof(int) + 4096));
    StreamDrain drain{st};
    uint32_t *d_ids = (uint32_t *)lane_alloc(ctx, lane, known * 4), *d_miss = (uint32_t *)lane_alloc(ctx, lane, (m ? m : 1) * 4);
    Fr *zv = (Fr *)lane_alloc(ctx, lane, K * 32), *zinv = (Fr *)lane_alloc(ctx, lane, K * 32);
    int *d_flags = (int *)lane_alloc(ctx, lane, B0 * sizeof(int));
    if (!d_ids || !d_miss || !zv || !zinv || !d_flags) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const size_t mark = ctx->lanes[lane].arena_used;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_ids, ids.data(), known * 4, hipMemcpyHostToDevice, st));
    if (m) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_miss, miss.data(), m * 4, hipMemcpyHostToDevice, st));

    // ---- once per call: Zs, Zs(nu^j) and 1 / Zs(7^l nu^j), j < K ----
    {
        kzg::ProfScope setup(ctx, st, "recover_setup");
        Fr *roots = (Fr *)lane_alloc(ctx, lane, mpad * 32), *t0 = (Fr *)lane_alloc(ctx, lane, mpad * 32);
        Fr *t1 = (Fr *)lane_alloc(ctx, lane, mpad * 32), *f = (Fr *)lane_alloc(ctx, lane, 2 * mpad * 32);
        Fr *g = (Fr *)lane_alloc(ctx, lane, mpad * 32), *tw = (Fr *)lane_alloc(ctx, lane, mpad * 16);
        Fr *zc = (Fr *)lane_alloc(ctx, lane, K * 32), *ptab = (Fr *)lane_alloc(ctx, lane, (1024 + hi_n) * 32);
        if (!roots || !t0 || !t1 || !f || !g || !tw || !zc || !ptab) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        const Fr nu = host_omega(log_k);
        KZG_TRY(pow_table(ctx, st, nu, Fr::one(), 1024, ptab));
        KZG_TRY(pow_table(ctx, st, pow_u64(nu, 1024), Fr::one(), hi_n, ptab + 1024));
        Fr *zs = nullptr;
        KZG_TRY(rec_zero_poly(ctx, st, d_miss, m, mpad, ptab, ptab + 1024, roots, t0, t1, f, g, tw, &zs));
        KZG_LAUNCH(ctx, st, "k_rec_zs_load", k_rec_zs_load, rec_grid(K), 256, 0, (const Fr *)zs, mpad - m, m, K, zv, zc);
        const size_t ntt_mark = ctx->lanes[lane].arena_used;
        KZG_TRY(ntt_run(ctx, lane, zv, log_k, 0));
        ctx->lanes[lane].arena_used = ntt_mark;
        KZG_TRY(coset_ntt_run(ctx, lane, zc, log_k, 0, pow_u64(from_u64<FrParams>(FR_MULT_GENERATOR), (uint64_t)l)));
        KZG_TRY(batch_inverse(ctx, st, zc, zinv, K));
    }

    // ---- the polynomials, in chunks ----
    ctx->lanes[lane].arena_used = mark;  // ordered behind the tree on the lane's stream
    Fr *work = (Fr *)lane_alloc(ctx, lane, B0 * N * 32);
    uint8_t *d_in = in_dev ? nullptr : (uint8_t *)lane_alloc(ctx, lane, B0 * kl * 32);
    uint8_t *d_stage = (out_dev || !out_coeffs) ? nullptr : (uint8_t *)lane_alloc(ctx, lane, B0 * n * 32);
    if (!work || (!in_dev && !d_in) || (!out_dev && out_coeffs && !d_stage)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const size_t ntt_mark = ctx->lanes[lane].arena_used;
    const size_t lo = n + m * l;  // coefficients [lo, N) of p Z vanish iff the cells are consistent
    int *h_flags = (int *)ctx->lanes[lane].pinned;
    bool any_bad = false;
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t B = std::min(chunk, batch - b0);
        const uint8_t *src = (const uint8_t *)cells + b0 * kl * 32;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * kl * 32, hipMemcpyHostToDevice, st));
            src = d_in;
        }
        KZG_HIP_CHECK(ctx, hipMemsetAsync(d_flags, 0, B * sizeof(int), st));
        KZG_LAUNCH(ctx, st, "k_rec_scatter", k_rec_scatter, dim3(rec_grid(N), (unsigned)B), 256, 0, (const Fr *)src, log_n, log_l,
                   (uint32_t)known, (const uint32_t *)d_ids, (const uint32_t *)d_miss, (const Fr *)zv, canonical, work);
        KZG_TRY(rec_ntt_each(ctx, lane, ntt_mark, work, B, log_n, 1, false));
        if (lo < N)
            KZG_LAUNCH(ctx, st, "k_rec_check", k_rec_check, dim3(rec_grid(N - lo), (unsigned)B), 256, 0, (const Fr *)work, log_n, (uint32_t)lo,
                       d_flags);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(h_flags, d_flags, B * sizeof(int), hipMemcpyDeviceToHost, st));
        KZG_TRY(rec_ntt_each(ctx, lane, ntt_mark, work, B, log_n, 0, true));
        KZG_LAUNCH(ctx, st, "k_rec_divide", k_rec_divide, rec_grid(B * N), 256, 0, work, B * N, (const Fr *)zinv, K - 1);
        KZG_TRY(rec_ntt_each(ctx, lane, ntt_mark, work, B, log_n, 1, true));
        Fr *d_c = !out_coeffs ? nullptr : (out_dev ? (Fr *)((uint8_t *)out_coeffs + b0 * n * 32) : (Fr *)d_stage);
        Fr *d_e = !out_evals ? nullptr : (out_dev ? (Fr *)((uint8_t *)out_evals + b0 * N * 32) : work);
        KZG_LAUNCH(ctx, st, "k_rec_emit", k_rec_emit, rec_grid(B * N), 256, 0, (const Fr *)work, log_n, n, B, canonical, d_c, d_e);
        if (out_coeffs && !out_dev)
            KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out_coeffs + b0 * n * 32, d_stage, B * n * 32, hipMemcpyDeviceToHost, st));
        if (out_evals) {  // the transform is linear: canonical coefficients in, canonical evaluations out
            KZG_TRY(rec_ntt_each(ctx, lane, ntt_mark, d_e, B, log_n, 0, false));
            if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out_evals + b0 * N * 32, d_e, B * N * 32, hipMemcpyDeviceToHost, st));
        }
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));  // the chunk's flags, once; the staging buffers are free again
        for (size_t b = 0; b < B; b++) {
            const int bad = h_flags[b] ? 1 : 0;
            if (status) status[b0 + b] = bad;
            any_bad |= bad != 0;
        }
    }
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    if (any_bad && !status) return fail(ctx, KZG_ERR_POINT_NOT_ON_POLY, "point not on polynomial!");
    return KZG_OK;
}
