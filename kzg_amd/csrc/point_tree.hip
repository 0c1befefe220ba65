// point_tree.hip -- a reusable, device-resident sub-product tree over an arbitrary point set (kzg_point_tree_*): SubProductTree
// (src/polynomial.rs:303-365), Polynomial::multi_eval (:229-233) and lagrange_interpolation_with_tree (:237-293) in O(k log^2 k).
// DESIGN.md section 3.4g; tests/point_tree_model.py is the big-int model of exactly these steps.
//
//   1. The k points are padded with K - k dummy points 0 to K = next_pow2(k): every node of level j is monic of degree exactly
//      d = 2^j and is stored as its low d coefficients (`low`, K scalars per level), the leading 1 implicit.  The root is X^(K-k) M.
//   2. Build.  Parents of up to `leaf` points (PT_LEAF, option "point_tree_leaf") are schoolbook products, one lane per coefficient
//      (k_pt_build_sb).  Above, the parent of two degree-d children is their product modulo X^(2d) - 1: the children's 2d-point
//      transforms (`hat`, kept in the plan: 2K scalars per level, the down and up steps need exactly these again), a pointwise
//      product and one inverse transform; the leading 1 lands on coefficient 0 and is subtracted (k_pt_sub_one).
//   3. Once per plan: G = 1 / rev(root) mod y^K by series_inverse_run (poly_divide.hip), kept transformed at 2K points with the
//      1 / 2K of the inverse transform folded in (`ghat`); x_i^K; M = root >> (K - k); den_i = M'(x_i) through the plan's own
//      evaluation, inverted by batch_inverse_mul, whose zero flag is `distinct`.
//   4. Evaluation of a block of at most K coefficients: f_root = rev_K(p) G mod y^K (one product of 2K points).  Going down, a node
//      of D = 2d points with vector f_v gives its left child f_l[t] = sum_{j <= d} m_j f_v[t + j], t < d, m the RIGHT sibling, and
//      the right child the same with the left sibling: cyclic at size D no wanted index wraps.  Schoolbook (k_pt_down_sb) for
//      D <= leaf; above, an inverse-direction transform of f_v, the product with the sibling's `hat` and a forward-direction
//      transform.  At the leaves f[0] is the value.
//   5. n > K: ceil(n / K) blocks run as one more batch dimension; k_pt_horner combines them per point in x_i^K.
//   6. Combine going up: N_v = N_l M_r + N_r M_l at size D; dummy leaves carry 0; the answer is coefficients [K - k, K) of the root.
//
// Transforms (pt_ntt_run): decimation in frequency, natural order in and bit-reversed spectrum out, or decimation in time the other
// way round, with the table of w or of 1 / w -- every spectrum here only meets spectra of the same order, so no permutation pass
// exists.  Stages of up to 2^PT_SMALL_LOG points run in one workgroup's LDS (k_pt_ntt_lds), batched over everything of a level in
// one launch; the stages above run one butterfly per lane over global memory (k_pt_ntt_stage).  The LDS tile is stored a 32-bit
// word per plane with one pad word per 64 elements: lanes of a wave touch neighbouring words of one plane, and the strided pairs of
// the short stages fall into different banks.
//
// Forms: the tree, its transforms, G, the twiddles and the points are Montgomery; every step is linear in the caller's data, whose
// Montgomery products with those leave it in the form it came in.  Raw inputs may be any 256-bit value: the load kernels reduce.
#include <algorithm>
#include <optional>

#include "common.h"

namespace kzg {

constexpr int PT_T = 256;                // threads per workgroup
constexpr int PT_LEAF = 16;              // nodes of up to this many points are schoolbook products (default and largest leaf)
constexpr int PT_SMALL_LOG = 10;         // transforms of up to 2^this points stay in one workgroup's LDS
constexpr size_t PT_CHUNK_ELEMS = (size_t)1 << 21;  // units (blocks x polynomials, or vectors) per chunk: max(1, this / K)
constexpr uint32_t PT_S = 1u << PT_SMALL_LOG, PT_PLANE = PT_S + PT_S / 64;

static inline unsigned pt_grid(size_t n) { return (unsigned)((n + PT_T - 1) / PT_T); }

// ---------------------------------------------------------------------------------------------
// transforms
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pt_slot(uint32_t e) { return e + (e >> 6); }
__device__ __forceinline__ Fr pt_lds_get(const uint32_t *lds, uint32_t e) {
    Fr v;
    const uint32_t s = pt_slot(e);
#pragma unroll
    for (int w = 0; w < 8; w++) v.v[w] = lds[w * PT_PLANE + s];
    return v;
}
__device__ __forceinline__ void pt_lds_put(uint32_t *lds, uint32_t e, const Fr &v) {
    const uint32_t s = pt_slot(e);
#pragma unroll
    for (int w = 0; w < 8; w++) lds[w * PT_PLANE + s] = v.v[w];
}

// the stages of half-width below 2^log_t (log_t <= PT_SMALL_LOG) on the PT_S elements from blockIdx.x PT_S on
template <int DIT>
__global__ __launch_bounds__(PT_T) void k_pt_ntt_lds(Fr *d, size_t total, uint32_t log_t, const Fr *tw, uint32_t log_tw) {
    __shared__ uint32_t lds[8 * PT_PLANE];
    const uint32_t t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * PT_S;
    const uint32_t cnt = total - base < PT_S ? (uint32_t)(total - base) : PT_S;  // a multiple of 2^log_t
    for (uint32_t e = t; e < cnt; e += PT_T) pt_lds_put(lds, e, d[base + e]);
    __syncthreads();
    for (uint32_t s = 0; s < log_t; s++) {
        const uint32_t log_h = DIT ? s : log_t - 1 - s, h = 1u << log_h;
        for (uint32_t bf = t; bf < cnt / 2; bf += PT_T) {
            const uint32_t j = bf & (h - 1), a = ((bf - j) << 1) + j, b = a + h;
            const Fr w = tw[(size_t)j << (log_tw - 1 - log_h)];
            const Fr u = pt_lds_get(lds, a), v = pt_lds_get(lds, b);
            if (DIT) {
                const Fr vw = mul(v, w);
                pt_lds_put(lds, a, add(u, vw));
                pt_lds_put(lds, b, sub(u, vw));
            } else {
                pt_lds_put(lds, a, add(u, v));
                pt_lds_put(lds, b, mul(sub(u, v), w));
            }
        }
        __syncthreads();
    }
    for (uint32_t e = t; e < cnt; e += PT_T) d[base + e] = pt_lds_get(lds, e);
}

// one stage of half-width 2^log_h over global memory, a butterfly per lane
template <int DIT>
__global__ __launch_bounds__(PT_T) void k_pt_ntt_stage(Fr *d, size_t total, uint32_t log_h, const Fr *tw, uint32_t log_tw) {
    const size_t bf = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (bf >= total / 2) return;
    const size_t h = (size_t)1 << log_h, j = bf & (h - 1), a = ((bf - j) << 1) + j, b = a + h;
    const Fr w = tw[j << (log_tw - 1 - log_h)];
    const Fr u = d[a], v = d[b];
    if (DIT) {
        const Fr vw = mul(v, w);
        d[a] = add(u, vw);
        d[b] = sub(u, vw);
    } else {
        d[a] = add(u, v);
        d[b] = mul(sub(u, v), w);
    }
}

int pt_ntt_run(kzg_ctx *ctx, hipStream_t st, Fr *d, size_t total, uint32_t log_t, int dit, const Fr *tw, uint32_t log_tw) {
    if (log_t == 0 || total == 0) return KZG_OK;
    const uint32_t ls = std::min<uint32_t>(log_t, PT_SMALL_LOG);
    const unsigned gl = (unsigned)((total + PT_S - 1) / PT_S);
    if (!dit) {
        for (uint32_t lh = log_t; lh-- > ls;) KZG_LAUNCH(ctx, st, "k_pt_ntt_stage", k_pt_ntt_stage<0>, pt_grid(total / 2), PT_T, 0, d, total, lh, tw, log_tw);
        KZG_LAUNCH(ctx, st, "k_pt_ntt_lds", k_pt_ntt_lds<0>, gl, PT_T, 0, d, total, ls, tw, log_tw);
    } else {
        KZG_LAUNCH(ctx, st, "k_pt_ntt_lds", k_pt_ntt_lds<1>, gl, PT_T, 0, d, total, ls, tw, log_tw);
        for (uint32_t lh = ls; lh < log_t; lh++) KZG_LAUNCH(ctx, st, "k_pt_ntt_stage", k_pt_ntt_stage<1>, pt_grid(total / 2), PT_T, 0, d, total, lh, tw, log_tw);
    }
    return KZG_OK;
}

// ---------------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------------
// level 0: the low coefficient -x of X - x
__global__ __launch_bounds__(PT_T) void k_pt_leaves(const Fr *xs, size_t K, Fr *low0) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i < K) low0[i] = neg(xs[i]);
}

// parent[v D + t] = coefficient t < D of (a + X^d)(b + X^d), a / b the low coefficients of the children 2v, 2v + 1 (D = 2d)
__global__ __launch_bounds__(PT_T) void k_pt_build_sb(const Fr *child, Fr *parent, size_t K, uint32_t log_d) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= K) return;
    const uint32_t d = 1u << log_d, t = (uint32_t)g & (2 * d - 1);
    const Fr *a = child + (g - t), *b = a + d;
    Fr acc = Fr::zero();
    for (uint32_t i = 0; i < d; i++)
        if (t >= i && t - i < d) acc = add(acc, mul(a[i], b[t - i]));
    if (t >= d) acc = add(acc, add(a[t - d], b[t - d]));
    parent[g] = acc;
}

// hat[c D + t] = coefficient t of child c of degree d with its leading 1, zero above: what the D-point transform takes
__global__ __launch_bounds__(PT_T) void k_pt_hat_load(const Fr *low, Fr *hat, size_t twoK, uint32_t log_d) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= twoK) return;
    const size_t d = (size_t)1 << log_d, t = g & (2 * d - 1), c = g >> (log_d + 1);
    hat[g] = t < d ? low[c * d + t] : (t == d ? Fr::one() : Fr::zero());
}

// out[v D + u] = scale hat[2v D + u] hat[(2v + 1) D + u]
__global__ __launch_bounds__(PT_T) void k_pt_build_mul(const Fr *hat, Fr *out, size_t K, uint32_t log_D, Fr scale) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= K) return;
    const size_t u = g & (((size_t)1 << log_D) - 1), l = ((g - u) << 1) + u;
    out[g] = mul(scale, mul(hat[l], hat[l + ((size_t)1 << log_D)]));
}

// the wrapped leading 1 of every node of D points
__global__ __launch_bounds__(PT_T) void k_pt_sub_one(Fr *low, size_t nodes, uint32_t log_D) {
    const size_t v = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (v < nodes) low[v << log_D] = sub(low[v << log_D], Fr::one());
}

// f[0] = 1, f[i] = root[K - i]: the first K coefficients of rev(root + X^K)
__global__ __launch_bounds__(PT_T) void k_pt_rev_root(const Fr *root, size_t K, Fr *f) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i < K) f[i] = i ? root[K - i] : Fr::one();
}

// dst[i] = scale src[i] for i < cnt, zero for cnt <= i < total
__global__ __launch_bounds__(PT_T) void k_pt_scale_pad(const Fr *src, size_t cnt, Fr scale, Fr *dst, size_t total) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i < total) dst[i] = i < cnt ? mul(src[i], scale) : Fr::zero();
}

// X[i] = x_i^(2^log_K)
__global__ __launch_bounds__(PT_T) void k_pt_xpow(const Fr *xs, size_t K, uint32_t log_K, Fr *X) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i >= K) return;
    Fr v = xs[i];
    for (uint32_t s = 0; s < log_K; s++) v = sqr(v);
    X[i] = v;
}

// M[j] = root[K - k + j] for j < k, M[k] = 1; dM[j] = (j + 1) M[j + 1] for j < k
__global__ __launch_bounds__(PT_T) void k_pt_true_m(const Fr *root, size_t K, size_t k, Fr *M, Fr *dM) {
    const size_t j = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (j > k) return;
    M[j] = j < k ? root[K - k + j] : Fr::one();
    if (j < k) {
        Fr c = Fr::zero();
        c.v[0] = (uint32_t)(j + 1);
        c.v[1] = (uint32_t)((uint64_t)(j + 1) >> 32);
        dM[j] = mul(to_mont(c), j + 1 < k ? root[K - k + j + 1] : Fr::one());
    }
}

__global__ __launch_bounds__(PT_T) void k_pt_fill(Fr *p, size_t n, Fr v) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---------------------------------------------------------------------------------------------
// evaluation (down)
// ---------------------------------------------------------------------------------------------
// R[unit 2K + t] = coefficient K - 1 - t of block blk0 + unit % nb of polynomial unit / nb (mod r; zero beyond n) for t < K, zero above
__global__ __launch_bounds__(PT_T) void k_pt_load_rev(const Fr *src, size_t n, size_t pstride, uint32_t log_K, size_t blk0, size_t nb, size_t total, Fr *R) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t K = (size_t)1 << log_K, unit = g >> (log_K + 1), t = g & (2 * K - 1);
    Fr v = Fr::zero();
    if (t < K) {
        const size_t idx = ((blk0 + unit % nb) << log_K) + (K - 1 - t);
        if (idx < n) v = fr_residue(src[(unit / nb) * pstride + idx]);
    }
    R[g] = v;
}

// a[i] *= b[i & mask]
__global__ __launch_bounds__(PT_T) void k_pt_mul_bcast(Fr *a, const Fr *b, size_t total, size_t mask) {
    const size_t i = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (i < total) a[i] = mul(a[i], b[i & mask]);
}

// A[c d + t] = R[c D + t] for t < d (D = 2d): the low half of every D-block
__global__ __launch_bounds__(PT_T) void k_pt_compact(const Fr *R, Fr *A, size_t total, uint32_t log_d) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t t = g & (((size_t)1 << log_d) - 1);
    A[g] = R[((g - t) << 1) + t];
}

// R[unit 2K + c D + u] = scale A[unit K + (c / 2) D + u] hat[(c ^ 1) D + u]: the spectrum of the parent against the sibling's
__global__ __launch_bounds__(PT_T) void k_pt_down_mul(const Fr *A, const Fr *hat, Fr *R, size_t total, uint32_t log_D, uint32_t log_K, Fr scale) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t K = (size_t)1 << log_K, D = (size_t)1 << log_D, unit = g >> (log_K + 1), r = g & (2 * K - 1), c = r >> log_D, u = r & (D - 1);
    R[g] = mul(mul(A[(unit << log_K) + ((c >> 1) << log_D) + u], scale), hat[((c ^ 1) << log_D) + u]);
}

// out[c d + t] = sum_{j < d} m[j] f[t + j] + f[t + d], f the parent's D values, m the low coefficients of child c's sibling
__global__ __launch_bounds__(PT_T) void k_pt_down_sb(const Fr *in, const Fr *low, Fr *out, size_t total, uint32_t log_d, uint32_t log_K) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t d = (size_t)1 << log_d, t = g & (d - 1), cg = g >> log_d, c = cg & ((((size_t)1 << log_K) >> log_d) - 1);
    const Fr *f = in + ((cg >> 1) << (log_d + 1)) + t, *m = low + ((c ^ 1) << log_d);
    Fr acc = f[d];
    for (size_t j = 0; j < d; j++) acc = add(acc, mul(f[j], m[j]));
    out[g] = acc;
}

// out[p ostride + i] = sum_blk V[(p nb + blk) K + i] X_i^blk (+ out[..] X_i^nb with carry): the blocks of a polynomial, highest first
__global__ __launch_bounds__(PT_T) void k_pt_horner(const Fr *V, const Fr *X, size_t P, size_t nb, uint32_t log_K, size_t k, int carry, Fr *out, size_t ostride) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= P * k) return;
    const size_t p = g / k, i = g - p * k;
    const Fr x = X[i];
    Fr acc = carry ? out[p * ostride + i] : Fr::zero();
    for (size_t b = nb; b-- > 0;) acc = add(mul(acc, x), V[((p * nb + b) << log_K) + i]);
    out[p * ostride + i] = acc;
}

// ---------------------------------------------------------------------------------------------
// combination (up)
// ---------------------------------------------------------------------------------------------
// A[unit K + i] = cs[unit k + i] mod r (times w[i] if w) for i < k, zero for the dummy leaves
__global__ __launch_bounds__(PT_T) void k_pt_up_load(const Fr *cs, size_t k, uint32_t log_K, size_t total, const Fr *w, Fr *A) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t unit = g >> log_K, i = g & (((size_t)1 << log_K) - 1);
    Fr v = Fr::zero();
    if (i < k) {
        v = fr_residue(cs[unit * k + i]);
        if (w) v = mul(v, w[i]);
    }
    A[g] = v;
}

// out[v D + t] = coefficient t of N_l (M_r + X^d) + N_r (M_l + X^d)
__global__ __launch_bounds__(PT_T) void k_pt_up_sb(const Fr *in, const Fr *low, Fr *out, size_t total, uint32_t log_d, uint32_t log_K) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const uint32_t d = 1u << log_d, t = (uint32_t)g & (2 * d - 1);
    const size_t nbase = g - t, mbase = nbase & (((size_t)1 << log_K) - 1);
    const Fr *nl = in + nbase, *nr = nl + d, *ml = low + mbase, *mr = ml + d;
    Fr acc = Fr::zero();
    for (uint32_t i = 0; i < d; i++) {
        if (t >= i && t - i < d) acc = add(acc, add(mul(nl[i], mr[t - i]), mul(nr[i], ml[t - i])));
        if (t == i + d) acc = add(acc, add(nl[i], nr[i]));
    }
    out[g] = acc;
}

// R[c D + t] = A[c d + t] for t < d, zero above
__global__ __launch_bounds__(PT_T) void k_pt_up_pad(const Fr *A, Fr *R, size_t total, uint32_t log_d) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t d = (size_t)1 << log_d, t = g & (2 * d - 1);
    R[g] = t < d ? A[((g - t) >> 1) + t] : Fr::zero();
}

// A[v D + u] = scale (R[2v D + u] hat[(2v' + 1) D + u] + R[(2v + 1) D + u] hat[2v' D + u]), v' the node within its unit
__global__ __launch_bounds__(PT_T) void k_pt_up_mul(const Fr *R, const Fr *hat, Fr *A, size_t total, uint32_t log_D, uint32_t log_K, Fr scale) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t D = (size_t)1 << log_D, u = g & (D - 1), l = ((g - u) << 1) + u, hl = (((g & (((size_t)1 << log_K) - 1)) - u) << 1) + u;
    A[g] = mul(scale, add(mul(R[l], hat[hl + D]), mul(R[l + D], hat[hl])));
}

// out[unit k + j] = A[unit K + K - k + j]
__global__ __launch_bounds__(PT_T) void k_pt_up_emit(const Fr *A, size_t k, uint32_t log_K, size_t total, Fr *out) {
    const size_t g = (size_t)blockIdx.x * PT_T + threadIdx.x;
    if (g >= total) return;
    const size_t unit = g / k, j = g - unit * k;
    out[g] = A[(unit << log_K) + (((size_t)1 << log_K) - k) + j];
}

}  // namespace kzg

using namespace kzg;

struct kzg_point_tree {
    int device = 0;
    size_t k = 0, K = 0, leaf = 0, bytes = 0;
    uint32_t log_K = 0, log_leaf = 0;
    int distinct = 0;
    Fr *low = nullptr;    // (log_K + 1) x K: level j at low + j K, node v at + v 2^j
    Fr *hat = nullptr;    // levels j with leaf <= 2^j < K: (j - log_leaf) 2K + c 2^(j+1): child c's transform of 2^(j+1) points
    Fr *ghat = nullptr;   // 2K: the transform of G / 2K
    Fr *tw = nullptr, *twi = nullptr;  // max(K, 1) each: w^j and w^-j of the 2K-th root of unity
    Fr *xs = nullptr, *xK = nullptr;   // K each: the padded points and their K-th powers
    Fr *dinv = nullptr;   // k: 1 / M'(x_i), zero where it does not exist
    Fr *mtrue = nullptr;  // k + 1: M
    const Fr *level(uint32_t j) const { return low + (size_t)j * K; }
    const Fr *hat_level(uint32_t j) const { return hat + (size_t)(j - log_leaf) * 2 * K; }
    ~kzg_point_tree() {
        for (Fr *p : {low, hat, ghat, tw, twi, xs, xK, dinv, mtrue})
            if (p) hipFree(p);
    }
};

namespace kzg {

static Fr pt_inv_pow2(uint32_t log) {  // 1 / 2^log, Montgomery
    Fr two = dbl(Fr::one()), v = Fr::one();
    for (uint32_t i = 0; i < log; i++) v = mul(v, two);
    return inv(v);
}

// The values of P polynomials' blocks [blk0, blk0 + nb) at the plan's points, combined over the blocks into out[p ostride + i], i < k
// (with carry: on top of out[..] X_i^nb).  d_src: device coefficients, polynomial p at + p pstride, n each.  d_R: P nb 2K elements,
// d_A: P nb K.
static int pt_eval_core(kzg_ctx *ctx, hipStream_t st, const kzg_point_tree *pl, const Fr *d_src, size_t n, size_t pstride, size_t P, size_t blk0,
                        size_t nb, int carry, Fr *d_R, Fr *d_A, Fr *d_out, size_t ostride) {
    const size_t K = pl->K, units = P * nb, tK = units * K, t2K = 2 * tK;
    const uint32_t lk = pl->log_K;
    KZG_LAUNCH(ctx, st, "k_pt_load_rev", k_pt_load_rev, pt_grid(t2K), PT_T, 0, d_src, n, pstride, lk, blk0, nb, t2K, d_R);
    KZG_TRY(pt_ntt_run(ctx, st, d_R, t2K, lk + 1, 0, pl->tw, lk + 1));
    KZG_LAUNCH(ctx, st, "k_pt_mul_bcast", k_pt_mul_bcast, pt_grid(t2K), PT_T, 0, d_R, (const Fr *)pl->ghat, t2K, 2 * K - 1);
    KZG_TRY(pt_ntt_run(ctx, st, d_R, t2K, lk + 1, 1, pl->twi, lk + 1));
    KZG_LAUNCH(ctx, st, "k_pt_compact", k_pt_compact, pt_grid(tK), PT_T, 0, (const Fr *)d_R, d_A, tK, lk);
    Fr *cur = d_A, *oth = d_R;
    for (uint32_t ld = lk; ld-- > 0;) {  // nodes of D = 2^(ld + 1) points to their children of d = 2^ld
        const size_t D = (size_t)2 << ld;
        if (D > pl->leaf) {  // (cur == d_A: the schoolbook levels are the last ones)
            KZG_TRY(pt_ntt_run(ctx, st, d_A, tK, ld + 1, 0, pl->twi, lk + 1));
            KZG_LAUNCH(ctx, st, "k_pt_down_mul", k_pt_down_mul, pt_grid(t2K), PT_T, 0, (const Fr *)d_A, pl->hat_level(ld), d_R, t2K, ld + 1, lk, pt_inv_pow2(ld + 1));
            KZG_TRY(pt_ntt_run(ctx, st, d_R, t2K, ld + 1, 1, pl->tw, lk + 1));
            KZG_LAUNCH(ctx, st, "k_pt_compact", k_pt_compact, pt_grid(tK), PT_T, 0, (const Fr *)d_R, d_A, tK, ld);
        } else {
            KZG_LAUNCH(ctx, st, "k_pt_down_sb", k_pt_down_sb, pt_grid(tK), PT_T, 0, (const Fr *)cur, pl->level(ld), oth, tK, ld, lk);
            std::swap(cur, oth);
        }
    }
    KZG_LAUNCH(ctx, st, "k_pt_horner", k_pt_horner, pt_grid(P * pl->k), PT_T, 0, (const Fr *)cur, (const Fr *)pl->xK, P, nb, lk, pl->k, carry, d_out, ostride);
    return KZG_OK;
}

// d_out[u k + j] = coefficient j of sum_i c_ui w_i M / (X - x_i) for `units` vectors d_cs (device, k each); d_R: units 2K, d_A: units K
static int pt_combine_core(kzg_ctx *ctx, hipStream_t st, const kzg_point_tree *pl, const Fr *d_cs, size_t units, const Fr *d_w, Fr *d_R, Fr *d_A,
                           Fr *d_out) {
    const size_t K = pl->K, tK = units * K, t2K = 2 * tK;
    const uint32_t lk = pl->log_K;
    KZG_LAUNCH(ctx, st, "k_pt_up_load", k_pt_up_load, pt_grid(tK), PT_T, 0, d_cs, pl->k, lk, tK, d_w, d_A);
    Fr *cur = d_A, *oth = d_R;
    for (uint32_t ld = 0; ld < lk; ld++) {  // children of d = 2^ld points to their parents of D = 2d
        const size_t D = (size_t)2 << ld;
        if (D <= pl->leaf) {
            KZG_LAUNCH(ctx, st, "k_pt_up_sb", k_pt_up_sb, pt_grid(tK), PT_T, 0, (const Fr *)cur, pl->level(ld), oth, tK, ld, lk);
            std::swap(cur, oth);
            continue;
        }
        if (cur != d_A) {  // an odd number of schoolbook levels left the sums in d_R
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_A, cur, tK * 32, hipMemcpyDeviceToDevice, st));
            cur = d_A;
            oth = d_R;
        }
        KZG_LAUNCH(ctx, st, "k_pt_up_pad", k_pt_up_pad, pt_grid(t2K), PT_T, 0, (const Fr *)d_A, d_R, t2K, ld);
        KZG_TRY(pt_ntt_run(ctx, st, d_R, t2K, ld + 1, 0, pl->tw, lk + 1));
        KZG_LAUNCH(ctx, st, "k_pt_up_mul", k_pt_up_mul, pt_grid(tK), PT_T, 0, (const Fr *)d_R, pl->hat_level(ld), d_A, tK, ld + 1, lk, pt_inv_pow2(ld + 1));
        KZG_TRY(pt_ntt_run(ctx, st, d_A, tK, ld + 1, 1, pl->twi, lk + 1));
    }
    KZG_LAUNCH(ctx, st, "k_pt_up_emit", k_pt_up_emit, pt_grid(units * pl->k), PT_T, 0, (const Fr *)cur, pl->k, lk, units * pl->k, d_out);
    return KZG_OK;
}

static int pt_malloc(kzg_ctx *ctx, kzg_point_tree *pl, Fr **p, size_t elems) {
    if (hipMalloc((void **)p, elems * 32) != hipSuccess) {
        *p = nullptr;
        return fail(ctx, KZG_ERR_ALLOC, "hipMalloc(point tree)");
    }
    pl->bytes += elems * 32;
    return KZG_OK;
}

static int pt_build(kzg_ctx *ctx, kzg_point_tree *pl, const std::vector<Fr> &xm) {
    const size_t k = pl->k, K = pl->K;
    const uint32_t lk = pl->log_K;
    const int lane = 0;
    hipStream_t st = ctx->lanes[lane].stream;
    const size_t nhat = lk > pl->log_leaf ? lk - pl->log_leaf : 0;
    KZG_TRY(pt_malloc(ctx, pl, &pl->low, (size_t)(lk + 1) * K));
    if (nhat) KZG_TRY(pt_malloc(ctx, pl, &pl->hat, nhat * 2 * K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->ghat, 2 * K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->tw, K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->twi, K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->xs, K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->xK, K));
    KZG_TRY(pt_malloc(ctx, pl, &pl->dinv, k));
    KZG_TRY(pt_malloc(ctx, pl, &pl->mtrue, k + 1));
    // the workspace: R (2K), A (K), f, g, dM, den, tmp (K each), the two scratch buffers of the series inverse (2K each) and its transforms'
    KZG_TRY(lane_reserve(ctx, lane, 12 * align_up(K * 32, 256) + ntt_workspace_bytes(lk + 1) + align_up(sizeof(int), 256) + 65536));
    Fr *d_R = (Fr *)lane_alloc(ctx, lane, 2 * K * 32), *d_A = (Fr *)lane_alloc(ctx, lane, K * 32), *d_f = (Fr *)lane_alloc(ctx, lane, K * 32);
    Fr *d_g = (Fr *)lane_alloc(ctx, lane, K * 32), *d_dM = (Fr *)lane_alloc(ctx, lane, K * 32), *d_den = (Fr *)lane_alloc(ctx, lane, K * 32);
    Fr *d_tmp = (Fr *)lane_alloc(ctx, lane, K * 32), *d_sA = (Fr *)lane_alloc(ctx, lane, 2 * K * 32), *d_sG = (Fr *)lane_alloc(ctx, lane, 2 * K * 32);
    int *d_flag = (int *)lane_alloc(ctx, lane, sizeof(int));
    if (!d_R || !d_A || !d_f || !d_g || !d_dM || !d_den || !d_tmp || !d_sA || !d_sG || !d_flag) return fail(ctx, KZG_ERR_ALLOC, "workspace");

    const Fr w = host_omega(lk + 1);
    KZG_TRY(pow_table(ctx, st, w, Fr::one(), K, pl->tw));
    KZG_TRY(pow_table(ctx, st, inv(w), Fr::one(), K, pl->twi));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(pl->xs, xm.data(), K * 32, hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_pt_xpow", k_pt_xpow, pt_grid(K), PT_T, 0, (const Fr *)pl->xs, K, lk, pl->xK);
    KZG_LAUNCH(ctx, st, "k_pt_leaves", k_pt_leaves, pt_grid(K), PT_T, 0, (const Fr *)pl->xs, K, pl->low);
    for (uint32_t ld = 0; ld < lk; ld++) {  // level ld -> ld + 1
        const size_t D = (size_t)2 << ld;
        Fr *child = pl->low + (size_t)ld * K, *parent = child + K;
        if (D <= pl->leaf) {
            KZG_LAUNCH(ctx, st, "k_pt_build_sb", k_pt_build_sb, pt_grid(K), PT_T, 0, (const Fr *)child, parent, K, ld);
            continue;
        }
        Fr *hat = pl->hat + (size_t)(ld - pl->log_leaf) * 2 * K;
        KZG_LAUNCH(ctx, st, "k_pt_hat_load", k_pt_hat_load, pt_grid(2 * K), PT_T, 0, (const Fr *)child, hat, 2 * K, ld);
        KZG_TRY(pt_ntt_run(ctx, st, hat, 2 * K, ld + 1, 0, pl->tw, lk + 1));
        KZG_LAUNCH(ctx, st, "k_pt_build_mul", k_pt_build_mul, pt_grid(K), PT_T, 0, (const Fr *)hat, parent, K, ld + 1, pt_inv_pow2(ld + 1));
        KZG_TRY(pt_ntt_run(ctx, st, parent, K, ld + 1, 1, pl->twi, lk + 1));
        KZG_LAUNCH(ctx, st, "k_pt_sub_one", k_pt_sub_one, pt_grid(K / D), PT_T, 0, parent, K / D, ld + 1);
    }
    const Fr *root = pl->level(lk);
    // G = 1 / rev(root) mod y^K, kept as its 2K-point transform over 2K
    KZG_LAUNCH(ctx, st, "k_pt_rev_root", k_pt_rev_root, pt_grid(K), PT_T, 0, root, K, d_f);
    const size_t base = ctx->opt_poly_divide_base ? (size_t)ctx->opt_poly_divide_base : 64;
    KZG_TRY(series_inverse_run(ctx, lane, d_f, K, K, base, d_g, d_sA, d_sG));
    KZG_LAUNCH(ctx, st, "k_pt_scale_pad", k_pt_scale_pad, pt_grid(2 * K), PT_T, 0, (const Fr *)d_g, K, pt_inv_pow2(lk + 1), pl->ghat, 2 * K);
    KZG_TRY(pt_ntt_run(ctx, st, pl->ghat, 2 * K, lk + 1, 0, pl->tw, lk + 1));
    // M, M' and den_i = M'(x_i) through the plan's own evaluation; 1 / den_i
    KZG_LAUNCH(ctx, st, "k_pt_true_m", k_pt_true_m, pt_grid(k + 1), PT_T, 0, root, K, k, pl->mtrue, d_dM);
    KZG_TRY(pt_eval_core(ctx, st, pl, d_dM, k, k, 1, 0, 1, 0, d_R, d_A, d_den, k));
    KZG_LAUNCH(ctx, st, "k_pt_fill", k_pt_fill, pt_grid(k), PT_T, 0, pl->dinv, k, Fr::one());
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), st));
    KZG_TRY(batch_inverse_mul(ctx, st, d_den, pl->dinv, d_tmp, k, d_flag));
    int flag = 0;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    pl->distinct = flag ? 0 : 1;
    return KZG_OK;
}

static int pt_check(kzg_ctx *ctx, const kzg_point_tree *pl, int sfmt, const char *who) {
    if (!pl) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL plan");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (pl->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": the point tree is resident on another GPU");
    return KZG_OK;
}

// combine (d_w null) and interpolate (d_w = 1 / M'(x_i)): `batch` vectors in chunks of max(1, PT_CHUNK_ELEMS / K)
static int pt_combine(kzg_ctx *ctx, const kzg_point_tree *pl, const void *cs, size_t batch, int flags, const Fr *d_w, void *out) {
    const size_t k = pl->k, K = pl->K;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const size_t C = std::min(batch, std::max<size_t>(1, PT_CHUNK_ELEMS / K));
    KZG_TRY(lane_reserve(ctx, lane, align_up(C * 2 * K * 32, 256) + align_up(C * K * 32, 256) + (in_dev ? 0 : align_up(C * k * 32, 256)) +
                                        (out_dev ? 0 : align_up(C * k * 32, 256)) + 65536));
    Fr *d_R = (Fr *)lane_alloc(ctx, lane, C * 2 * K * 32), *d_A = (Fr *)lane_alloc(ctx, lane, C * K * 32);
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, C * k * 32), *d_o = out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, C * k * 32);
    if (!d_R || !d_A || (!in_dev && !d_in) || (!out_dev && !d_o)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const size_t B = std::min(C, batch - b0);
        const Fr *src = (const Fr *)cs + b0 * k;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * k * 32, hipMemcpyHostToDevice, st));
            src = d_in;
        }
        Fr *dst = out_dev ? (Fr *)out + b0 * k : d_o;
        KZG_TRY(pt_combine_core(ctx, st, pl, src, B, d_w, d_R, d_A, dst));
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)out + b0 * k, d_o, B * k * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

// what the callers of other translation units read of a plan (common.h)
void point_tree_view(const kzg_point_tree *pl, PointTreeView *v) {
    v->device = pl->device;
    v->k = pl->k;
    v->K = pl->K;
    v->distinct = pl->distinct;
    v->product = pl->mtrue;
}
int point_tree_interpolate_run(kzg_ctx *ctx, hipStream_t st, const kzg_point_tree *pl, const Fr *d_ys, size_t units, Fr *d_R, Fr *d_A, Fr *d_out) {
    return pt_combine_core(ctx, st, pl, d_ys, units, pl->dinv, d_R, d_A, d_out);
}

}  // namespace kzg

extern "C" int kzg_point_tree_setup(kzg_ctx *ctx, const void *xs, size_t k, int sfmt, kzg_point_tree **out) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!xs || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_setup: NULL xs or out");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (k == 0 || k > ((size_t)1 << 22)) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_setup: 1 <= k <= 2^22 points");
    const uint32_t lk = (uint32_t)ilog2_ceil(k);
    const size_t K = (size_t)1 << lk;
    std::vector<Fr> xm;
    try {  // (no exception may leave through the C ABI)
        xm.assign(K, Fr::zero());
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the points");
    }
    for (size_t i = 0; i < k; i++) {
        Fr v;
        memcpy(v.v, (const uint8_t *)xs + 32 * i, 32);
        if (!is_canonical(v)) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_setup: a point is not below r");
        xm[i] = sfmt == KZG_FR_CANONICAL_LE_32 ? to_mont(v) : v;
    }
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kzg_point_tree *pl = new (std::nothrow) kzg_point_tree();
    if (!pl) return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    pl->device = ctx->device;
    pl->k = k;
    pl->K = K;
    pl->log_K = lk;
    pl->leaf = ctx->opt_point_tree_leaf ? (size_t)ctx->opt_point_tree_leaf : (size_t)PT_LEAF;
    pl->log_leaf = (uint32_t)ilog2_ceil(pl->leaf);
    const int rc = pt_build(ctx, pl, xm);
    if (rc != KZG_OK) {
        hipStreamSynchronize(ctx->lanes[0].stream);
        delete pl;
        return rc;
    }
    *out = pl;
    return KZG_OK;
}

extern "C" void kzg_point_tree_free(kzg_ctx *ctx, kzg_point_tree *plan) {
    if (!plan) return;
    std::optional<Guard> g;
    if (ctx) g.emplace(ctx);
    hipSetDevice(plan->device);
    hipDeviceSynchronize();
    delete plan;
}

extern "C" int kzg_point_tree_shape(const kzg_point_tree *plan, size_t *k, size_t *padded, size_t *bytes, int *distinct) {
    if (!plan) return KZG_ERR_SHAPE;
    if (k) *k = plan->k;
    if (padded) *padded = plan->K;
    if (bytes) *bytes = plan->bytes;
    if (distinct) *distinct = plan->distinct;
    return KZG_OK;
}

extern "C" int kzg_point_tree_product(kzg_ctx *ctx, const kzg_point_tree *plan, int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    KZG_TRY(pt_check(ctx, plan, sfmt, "kzg_point_tree_product"));
    if (!out) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_product: NULL out");
    const size_t cnt = plan->k + 1;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool out_dev = (flags & KZG_OUT_DEVICE) != 0;
    KZG_TRY(lane_reserve(ctx, lane, align_up(cnt * 32, 256) + 65536));
    Fr *d_m = out_dev ? (Fr *)out : (Fr *)lane_alloc(ctx, lane, cnt * 32);
    if (!d_m) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_m, plan->mtrue, cnt * 32, hipMemcpyDeviceToDevice, st));
    if (sfmt == KZG_FR_CANONICAL_LE_32) KZG_TRY(fr_convert(ctx, st, d_m, cnt, 0));
    if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, d_m, cnt * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_point_tree_eval(kzg_ctx *ctx, const kzg_point_tree *plan, const void *coeffs, size_t n, size_t batch, int sfmt, int flags,
                                   void *ys_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    KZG_TRY(pt_check(ctx, plan, sfmt, "kzg_point_tree_eval"));
    if (!coeffs || !ys_out) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_eval: NULL coeffs or ys_out");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, "empty polynomial");
    if (n > ((size_t)1 << 28)) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_eval: polynomials of up to 2^28 coefficients");
    if (batch > ((size_t)1 << 40) / n || batch > ((size_t)1 << 50) / plan->k) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_eval: batch x n or batch x k too large");
    if (batch == 0) return KZG_OK;
    const size_t k = plan->k, K = plan->K, nblocks = (n + K - 1) / K;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    // a chunk: P whole polynomials, or nb blocks of one polynomial (highest first, combined with carry); P nb K <= PT_CHUNK_ELEMS
    const bool whole = nblocks * K <= PT_CHUNK_ELEMS;
    const size_t P = whole ? std::min(batch, PT_CHUNK_ELEMS / (nblocks * K)) : 1, nb = whole ? nblocks : std::max<size_t>(1, PT_CHUNK_ELEMS / K);
    const size_t units = P * nb, stage_in = in_dev ? 0 : (whole ? P * n : nb * K);
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_TRY(lane_reserve(ctx, lane, align_up(units * 2 * K * 32, 256) + align_up(units * K * 32, 256) + align_up(stage_in * 32, 256) +
                                        (out_dev ? 0 : align_up(P * k * 32, 256)) + 65536));
    Fr *d_R = (Fr *)lane_alloc(ctx, lane, units * 2 * K * 32), *d_A = (Fr *)lane_alloc(ctx, lane, units * K * 32);
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, stage_in * 32), *d_y = out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, P * k * 32);
    if (!d_R || !d_A || (!in_dev && !d_in) || (!out_dev && !d_y)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    for (size_t b0 = 0; b0 < batch; b0 += P) {
        const size_t B = std::min(P, batch - b0);
        Fr *dst = out_dev ? (Fr *)ys_out + b0 * k : d_y;
        if (whole) {
            const Fr *src = (const Fr *)coeffs + b0 * n;
            if (!in_dev) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * n * 32, hipMemcpyHostToDevice, st));
                src = d_in;
            }
            KZG_TRY(pt_eval_core(ctx, st, plan, src, n, n, B, 0, nblocks, 0, d_R, d_A, dst, k));
        } else {
            for (size_t hi = nblocks; hi > 0;) {  // blocks [lo, hi) of polynomial b0
                const size_t lo = hi > nb ? hi - nb : 0, first = lo * K, len = std::min(n, hi * K) - first;
                const Fr *src = (const Fr *)coeffs + b0 * n + first;
                if (!in_dev) {
                    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, len * 32, hipMemcpyHostToDevice, st));
                    src = d_in;
                }
                KZG_TRY(pt_eval_core(ctx, st, plan, src, len, 0, 1, 0, hi - lo, hi != nblocks, d_R, d_A, dst, k));
                hi = lo;
            }
        }
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)ys_out + b0 * k, d_y, B * k * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_point_tree_combine(kzg_ctx *ctx, const kzg_point_tree *plan, const void *cs, size_t batch, int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    KZG_TRY(pt_check(ctx, plan, sfmt, "kzg_point_tree_combine"));
    if (!cs || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_combine: NULL cs or out");
    if (batch > ((size_t)1 << 50) / plan->k) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_combine: batch x k too large");
    if (batch == 0) return KZG_OK;
    return pt_combine(ctx, plan, cs, batch, flags, nullptr, out);
}

extern "C" int kzg_point_tree_interpolate(kzg_ctx *ctx, const kzg_point_tree *plan, const void *ys, size_t batch, int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    KZG_TRY(pt_check(ctx, plan, sfmt, "kzg_point_tree_interpolate"));
    if (!ys || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_interpolate: NULL ys or out");
    if (!plan->distinct) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_interpolate: two points of the plan coincide (the reference panics in invert().unwrap())");
    if (batch > ((size_t)1 << 50) / plan->k) return fail(ctx, KZG_ERR_SHAPE, "kzg_point_tree_interpolate: batch x k too large");
    if (batch == 0) return KZG_OK;
    return pt_combine(ctx, plan, ys, batch, flags, plan->dinv, out);
}
