// poly_divide.hip -- quotient and remainder of `batch` dividends by ONE divisor of any degree (kzg_poly_divide): Polynomial::long_division
// (src/polynomial.rs:193-227) without its sequential O((n - m) m) loop.  DESIGN.md section 3.4f; tests/poly_divide_model.py is the
// big-int model of exactly these steps.
//
// With m = na - nb + 1 quotient coefficients and f = rev(b) (f_0 = b[nb - 1] != 0):
//   1. g = 1 / f mod X^m, once per call.  k_pd_inv_base makes the first min(base, m) coefficients in LDS by the schoolbook recurrence
//      g_i = -g_0 sum_{j >= 1} f_j g_(i-j), the sum spread over the lanes of one wave.  Each Newton level k -> hi = min(2k, m) is
//      g(2 - f g) through ntt_run: two forward transforms of T points, k_pd_newton (G (2 - F G) pointwise) and one inverse; the
//      coefficients [k, hi) are new, the ones below k do not change.  f g g has fl + 2k - 2 coefficients (fl = min(hi, nb)); modulo
//      X^T - 1 the ones from T on wrap to positions below fl + 2k - 2 - T, so T = pow2(max(hi, fl + k - 2)) keeps [k, hi) clean: 2k for
//      a divisor of up to k + 2 coefficients, 4k otherwise.  A short f takes the transform's short-input path.
//   2. q = rev((rev(a) mod X^m) g mod X^m) per dividend: Tq = pow2(2m - 1) points; the transform of g is made once.  k_pd_load
//      reverses and truncates on the way in, k_pd_emit_rev reverses on the way out.
//   3. r = a - q b has fewer than nb - 1 <= N = pow2(nb - 1) coefficients, so it equals (a - q b) mod (X^N - 1): k_pd_fold streams a and
//      q once each into N sums, the product with the once-transformed folded b is one pointwise pass between two N-point transforms.
//      k_pd_rem subtracts, writes r and clears the dividend's `exact` flag at a non-zero coefficient.
//
// Forms: the divisor goes to Montgomery form in its load kernels (f, g and the transforms of g and b are Montgomery); every step is
// linear in the dividend, whose Montgomery products with those leave it in the form it came in, so a, q and r are never converted.
// Raw inputs may be any 256-bit value: every kernel that reads caller memory reduces (two conditional subtractions: 2^256 < 3r).
#include <algorithm>

#include "common.h"

namespace kzg {

constexpr int PD_T = 256;         // threads per workgroup of the streaming kernels
constexpr int PD_BASE = 64;       // default (and largest) precision of the base kernel: one wave, 6 KiB of LDS
constexpr int PD_FOLD_TERMS = 16; // terms a lane of k_pd_fold adds at most
constexpr size_t PD_CHUNK_COEFFS = (size_t)1 << 20, PD_CHUNK_MAX = 256;  // dividends per chunk: min(batch, clamp(2^20 / na, 1, 256))

__device__ __forceinline__ Fr pd_reduced(Fr v) {
    reduce_once(v);
    reduce_once(v);
    return v;
}

// dst[i] = src[rev ? top - i : i] mod r for i < cnt (in Montgomery form if to_m), zero for cnt <= i < total
__global__ __launch_bounds__(PD_T) void k_pd_load(const Fr *src, size_t top, int rev, size_t cnt, Fr *dst, size_t total, int to_m) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i >= total) return;
    Fr v = Fr::zero();
    if (i < cnt) {
        v = pd_reduced(src[rev ? top - i : i]);
        if (to_m) v = to_mont(v);
    }
    dst[i] = v;
}

// dst[j] = b[j] + b[j + N] mod r in Montgomery form, j < N (nb <= N + 1 coefficients: b mod (X^N - 1))
__global__ __launch_bounds__(PD_T) void k_pd_fold_b(const Fr *b, size_t nb, Fr *dst, size_t N, int to_m) {
    const size_t j = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (j >= N) return;
    Fr v = j < nb ? pd_reduced(b[j]) : Fr::zero();
    if (j + N < nb) v = add(v, pd_reduced(b[j + N]));
    dst[j] = to_m ? to_mont(v) : v;
}

// g[0, k0) = 1 / f mod X^k0 for k0 <= PD_BASE, f of fl coefficients with f[0] != 0.  One wave: lane t holds the term j = t + 1 of
// g_i = -g_0 sum_{1 <= j <= i} f_j g_(i-j); the terms are summed by a tree in LDS.
__global__ __launch_bounds__(PD_BASE) void k_pd_inv_base(const Fr *f, uint32_t fl, uint32_t k0, Fr *g) {
    __shared__ Fr sf[PD_BASE], sg[PD_BASE], red[PD_BASE];
    const uint32_t t = threadIdx.x;
    sf[t] = t < fl ? f[t] : Fr::zero();
    sg[t] = Fr::zero();
    __syncthreads();
    if (t == 0) sg[0] = inv(sf[0]);
    __syncthreads();
    const Fr ng0 = neg(sg[0]);
    for (uint32_t i = 1; i < k0; i++) {
        red[t] = t + 1 <= i ? mul(sf[t + 1], sg[i - t - 1]) : Fr::zero();  // (t + 1 <= i < PD_BASE)
        __syncthreads();
        for (uint32_t off = PD_BASE / 2; off > 0; off >>= 1) {
            if (t < off) red[t] = add(red[t], red[t + off]);
            __syncthreads();
        }
        if (t == 0) sg[i] = mul(ng0, red[0]);
        __syncthreads();
    }
    if (t < k0) g[t] = sg[t];
}

// G[i] = G[i] (2 - F[i] G[i]): the Newton step on the transformed values
__global__ __launch_bounds__(PD_T) void k_pd_newton(const Fr *F, Fr *G, size_t T) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i >= T) return;
    const Fr gi = G[i], two = dbl(Fr::one());
    G[i] = mul(gi, sub(two, mul(F[i], gi)));
}

// a[i] *= b[i] (b Montgomery: a keeps its form)
__global__ __launch_bounds__(PD_T) void k_pd_mul(Fr *a, const Fr *b, size_t n) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i < n) a[i] = mul(a[i], b[i]);
}

// q[i] = c a[i] (nb == 1: c = 1 / b[0], Montgomery)
__global__ __launch_bounds__(PD_T) void k_pd_scale(const Fr *a, const Fr *c, Fr *q, size_t n) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i < n) q[i] = mul(pd_reduced(a[i]), c[0]);
}

// q[i] = v[m - 1 - i], i < m: the quotient from the low m coefficients of rev(a) g
__global__ __launch_bounds__(PD_T) void k_pd_emit_rev(const Fr *v, size_t m, Fr *q) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i < m) q[i] = pd_reduced(v[m - 1 - i]);
}

// dst[t] = sum_s v(t + W s) for t < W, where v(i) = src[rev ? top - i : i] mod r for i < len: src mod (X^W - 1).  Lanes read
// neighbouring addresses; W is chosen by the host so that a lane adds at most PD_FOLD_TERMS terms.
__global__ __launch_bounds__(PD_T) void k_pd_fold(const Fr *src, size_t len, size_t top, int rev, size_t W, Fr *dst) {
    const size_t t = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (t >= W) return;
    Fr acc = Fr::zero();
    for (size_t i = t; i < len; i += 4 * W) {  // four loads in flight per lane
        Fr v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const size_t iu = i + (size_t)u * W;
            v[u] = iu < len ? src[rev ? top - iu : iu] : Fr::zero();
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = add(acc, pd_reduced(v[u]));
    }
    dst[t] = acc;
}

// r[j] = af[j] - qb[j] for j < nr (qb null: r = af); *exact = 0 if one of them is non-zero.  r may be null.  The flag is cleared by
// a plain store: every writer writes the same 0, and a wave's stores to the one address merge (an atomic per non-zero coefficient
// measured 6 ms at 2^19 coefficients).
__global__ __launch_bounds__(PD_T) void k_pd_rem(const Fr *af, const Fr *qb, size_t nr, Fr *r, int *exact) {
    const size_t j = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (j >= nr) return;
    const Fr v = qb ? sub(af[j], pd_reduced(qb[j])) : af[j];
    if (r) r[j] = v;
    if (!v.is_zero()) *exact = 0;
}

__global__ __launch_bounds__(PD_T) void k_pd_fill_int(int *p, size_t n, int v) {
    const size_t i = (size_t)blockIdx.x * PD_T + threadIdx.x;
    if (i < n) p[i] = v;
}

static inline unsigned pd_grid(size_t n) { return (unsigned)((n + PD_T - 1) / PD_T); }
static inline size_t pd_pow2(size_t x) { return (size_t)1 << ilog2_ceil(x); }

// one transform whose scratch goes back to the arena (the kernels of a call follow one another on the lane's stream)
static int pd_ntt(kzg_ctx *ctx, int lane, Fr *d, uint32_t log_n, int inverse, size_t nnz = (size_t)-1) {
    if (log_n == 0) return KZG_OK;  // one point: the identity
    const size_t mark = ctx->lanes[lane].arena_used;
    KZG_TRY(ntt_run(ctx, lane, d, log_n, inverse, nnz));
    ctx->lanes[lane].arena_used = mark;
    return KZG_OK;
}

// elements of the two ping-pong buffers pd_fold_run needs for `len` coefficients folded to N
static inline size_t pd_fold_tmp0(size_t len, size_t N) { return len / PD_FOLD_TERMS + 2 * N + 64; }
static inline size_t pd_fold_tmp1(size_t len, size_t N) { return len / PD_FOLD_TERMS / PD_FOLD_TERMS + 2 * N + 64; }

// dst[0, N) = src mod (X^N - 1) in stages of at most PD_FOLD_TERMS terms per lane; the widths are multiples of N
static int pd_fold_run(kzg_ctx *ctx, hipStream_t st, const Fr *src, size_t len, int rev, size_t N, Fr *tmp0, Fr *tmp1, Fr *dst) {
    const size_t top = len - 1;
    for (int stage = 0;; stage++) {
        const size_t terms = (len + N - 1) / N;
        const bool last = terms <= (size_t)PD_FOLD_TERMS;
        const size_t W = last ? N : N * ((terms + PD_FOLD_TERMS - 1) / PD_FOLD_TERMS);
        Fr *out = last ? dst : ((stage & 1) ? tmp1 : tmp0);
        KZG_LAUNCH(ctx, st, "k_pd_fold", k_pd_fold, pd_grid(W), PD_T, 0, src, len, rev ? top : 0, rev, W, out);
        if (last) return KZG_OK;
        src = out;
        len = W;
        rev = 0;
    }
}

// transform size of the Newton level k -> hi for a divisor with fl coefficients below X^hi
static inline size_t pd_newton_size(size_t k, size_t hi, size_t fl) { return pd_pow2(std::max(hi, fl + k - 2)); }

// g[0, m) = 1 / f mod X^m for f of fl_all <= m coefficients, f[0] != 0 (f, g Montgomery): the first min(base, m) coefficients by
// k_pd_inv_base (base <= PD_BASE), then Newton doubling.  d_A, d_G: scratch of pow2(2 m - 1) elements each; the lane's arena must
// have ntt_workspace_bytes(ilog2_ceil(2 m - 1)) left.  Shared by kzg_poly_divide and kzg_point_tree_setup.
int series_inverse_run(kzg_ctx *ctx, int lane, const Fr *d_f, size_t fl_all, size_t m, size_t base, Fr *d_g, Fr *d_A, Fr *d_G) {
    hipStream_t st = ctx->lanes[lane].stream;
    size_t k = std::min(std::min(base, (size_t)PD_BASE), m);
    KZG_LAUNCH(ctx, st, "k_pd_inv_base", k_pd_inv_base, 1, PD_BASE, 0, d_f, (uint32_t)std::min<size_t>(fl_all, PD_BASE), (uint32_t)k, d_g);
    while (k < m) {  // Newton: F in d_A, G in d_G
        const size_t hi = std::min(2 * k, m), fl = std::min(hi, fl_all), T = pd_newton_size(k, hi, fl);
        const uint32_t log_T = (uint32_t)ilog2_ceil(T);
        const bool sf = ntt_short_input_ok(log_T, fl);
        KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(sf ? fl : T), PD_T, 0, d_f, 0, 0, fl, d_A, sf ? fl : T, 0);
        KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(T), PD_T, 0, d_g, 0, 0, k, d_G, T, 0);
        KZG_TRY(pd_ntt(ctx, lane, d_A, log_T, 0, sf ? fl : (size_t)-1));
        KZG_TRY(pd_ntt(ctx, lane, d_G, log_T, 0));
        KZG_LAUNCH(ctx, st, "k_pd_newton", k_pd_newton, pd_grid(T), PD_T, 0, d_A, d_G, T);
        KZG_TRY(pd_ntt(ctx, lane, d_G, log_T, 1));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_g + k, d_G + k, (hi - k) * 32, hipMemcpyDeviceToDevice, st));  // the truncation to hi
        k = hi;
    }
    return KZG_OK;
}

// ---- the division by ONE divisor as device-level stages (common.h, PolyDivisor): behind kzg_poly_divide and kzg_witness_coeff_tree ----
void poly_divisor_shape(size_t na, size_t nb, PolyDivisor *d) {
    d->na = na;
    d->nb = nb;
    d->m = na >= nb ? na - nb + 1 : 0;
    d->nr = nb - 1;
    d->log_tq = d->m ? (uint32_t)ilog2_ceil(2 * d->m - 1) : 0;
    d->log_N = d->nr ? (uint32_t)ilog2_ceil(d->nr) : 0;
    d->Tq = (size_t)1 << d->log_tq;
    d->N = (size_t)1 << d->log_N;
    d->fl_all = std::min(nb, std::max<size_t>(d->m, 1));
    d->t0 = pd_fold_tmp0(std::max(na, d->m), d->N);
    d->t1 = pd_fold_tmp1(std::max(na, d->m), d->N);
}

// what depends on the divisor alone (m >= 1, nb >= 2): f = rev(b) mod X^m, g = 1 / f, the transform of g and, with want_r, of b folded
int poly_divisor_run(kzg_ctx *ctx, int lane, const Fr *bd, int to_m, bool want_r, const PolyDivisor &d) {
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(d.fl_all), PD_T, 0, bd, d.nb - 1, 1, d.fl_all, d.f, d.fl_all, to_m);
    const size_t base = ctx->opt_poly_divide_base ? (size_t)ctx->opt_poly_divide_base : (size_t)PD_BASE;
    KZG_TRY(series_inverse_run(ctx, lane, d.f, d.fl_all, d.m, base, d.g, d.A, d.G));  // (A, G: free until the quotient stage)
    KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(d.Tq), PD_T, 0, d.g, 0, 0, d.m, d.G, d.Tq, 0);
    KZG_TRY(pd_ntt(ctx, lane, d.G, d.log_tq, 0));
    if (want_r) {
        KZG_LAUNCH(ctx, st, "k_pd_fold_b", k_pd_fold_b, pd_grid(d.N), PD_T, 0, bd, d.nb, d.B, d.N, to_m);
        KZG_TRY(pd_ntt(ctx, lane, d.B, d.log_N, 0));
    }
    return KZG_OK;
}

// one dividend ai (na coefficients, device): qi (m coefficients, may be null) and, with want_r, ri (nr coefficients, may be null) with
// *flag cleared at a non-zero remainder coefficient
int poly_dividend_run(kzg_ctx *ctx, int lane, const PolyDivisor &d, const Fr *ai, Fr *qi, bool want_r, Fr *ri, int *flag) {
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(d.Tq), PD_T, 0, ai, d.na - 1, 1, d.m, d.A, d.Tq, 0);  // rev(a) mod X^m
    KZG_TRY(pd_ntt(ctx, lane, d.A, d.log_tq, 0));
    KZG_LAUNCH(ctx, st, "k_pd_mul", k_pd_mul, pd_grid(d.Tq), PD_T, 0, d.A, d.G, d.Tq);
    KZG_TRY(pd_ntt(ctx, lane, d.A, d.log_tq, 1));
    if (qi) KZG_LAUNCH(ctx, st, "k_pd_emit_rev", k_pd_emit_rev, pd_grid(d.m), PD_T, 0, d.A, d.m, qi);
    if (!want_r) return KZG_OK;
    KZG_TRY(pd_fold_run(ctx, st, ai, d.na, 0, d.N, d.tmp0, d.tmp1, d.af));
    KZG_TRY(pd_fold_run(ctx, st, d.A, d.m, 1, d.N, d.tmp0, d.tmp1, d.qf));
    KZG_TRY(pd_ntt(ctx, lane, d.qf, d.log_N, 0));
    KZG_LAUNCH(ctx, st, "k_pd_mul", k_pd_mul, pd_grid(d.N), PD_T, 0, d.qf, d.B, d.N);
    KZG_TRY(pd_ntt(ctx, lane, d.qf, d.log_N, 1));
    KZG_LAUNCH(ctx, st, "k_pd_rem", k_pd_rem, pd_grid(d.nr), PD_T, 0, d.af, d.qf, d.nr, ri, flag);
    return KZG_OK;
}

// dst[i] = src[i] mod r for i < cnt, zero for cnt <= i < total: a dividend shorter than the divisor is its own remainder
int poly_pad_run(kzg_ctx *ctx, hipStream_t st, const Fr *src, size_t cnt, Fr *dst, size_t total) {
    KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(total), PD_T, 0, src, 0, 0, cnt, dst, total, 0);
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_poly_divide(kzg_ctx *ctx, const void *a, size_t na, size_t batch, const void *b, size_t nb, int sfmt, int flags, void *q_out,
                               void *r_out, int *exact) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (na == 0 || nb == 0) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: empty dividend or divisor");
    if (na > ((size_t)1 << 27)) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: dividends of up to 2^27 coefficients");
    if (batch > (~(size_t)0 / 32) / na) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: batch x na too large");
    if (batch == 0) return KZG_OK;
    if (!a || !b) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: NULL a or b");
    const size_t m = na >= nb ? na - nb + 1 : 0, nr = nb - 1;  // quotient / remainder coefficients per dividend
    if (!q_out && !r_out && (m || nr)) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: NULL q_out and r_out");
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const int to_m = sfmt == KZG_FR_CANONICAL_LE_32;

    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    {  // the top coefficient: 32 bytes, wherever the divisor lives
        Fr top;
        const uint8_t *p = (const uint8_t *)b + (nb - 1) * 32;
        if (in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(top.v, p, 32, hipMemcpyDeviceToHost, st));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
        } else {
            memcpy(top.v, p, 32);
        }
        reduce_once(top);
        reduce_once(top);
        if (top.is_zero()) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_divide: the divisor's top coefficient is zero (divisor must not be zero; pass slice_coeffs())");
    }

    const bool want_q = q_out && m, want_r = (r_out || exact) && nr && m;  // (m == 0: the remainder is the dividend itself)
    const size_t C = std::min(batch, std::min(PD_CHUNK_MAX, std::max<size_t>(1, PD_CHUNK_COEFFS / na)));
    PolyDivisor dv;
    poly_divisor_shape(na, nb, &dv);
    const uint32_t log_tq = dv.log_tq, log_N = dv.log_N;
    const size_t Tq = dv.Tq, N = dv.N, fl_all = dv.fl_all, t0 = dv.t0, t1 = dv.t1;
    const bool general = m && nb > 1;
    size_t need = 65536 + align_up(C * sizeof(int), 256) + align_up(nb * 32, 256) + align_up(fl_all * 32, 256);
    if (!in_dev) need += align_up(C * na * 32, 256);
    const bool stage_q = !out_dev && want_q, stage_r = !out_dev && r_out && nr;  // host outputs: a chunk's results are staged
    if (stage_q) need += align_up(C * m * 32, 256);
    if (stage_r) need += align_up(C * nr * 32, 256);
    if (!m && !r_out) need += align_up(nr * 32, 256);
    if (general) need += align_up(m * 32, 256) + 2 * align_up(Tq * 32, 256) + ntt_workspace_bytes(log_tq);
    if (general && want_r) need += 3 * align_up(N * 32, 256) + align_up(t0 * 32, 256) + align_up(t1 * 32, 256) + ntt_workspace_bytes(log_N);
    KZG_TRY(lane_reserve(ctx, lane, need));
    int *d_exact = (int *)lane_alloc(ctx, lane, C * sizeof(int));
    Fr *d_b = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, nb * 32);
    Fr *d_f = (Fr *)lane_alloc(ctx, lane, fl_all * 32);
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, C * na * 32);
    Fr *d_q = stage_q ? (Fr *)lane_alloc(ctx, lane, C * m * 32) : nullptr;
    Fr *d_r = stage_r ? (Fr *)lane_alloc(ctx, lane, C * nr * 32) : nullptr;
    if (!d_exact || !d_f || (!in_dev && (!d_b || !d_in)) || (stage_q && !d_q) || (stage_r && !d_r)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    Fr *d_g = nullptr, *d_G = nullptr, *d_A = nullptr, *d_B = nullptr, *d_af = nullptr, *d_qf = nullptr, *d_t0 = nullptr, *d_t1 = nullptr;
    Fr *d_pad = nullptr;  // na < nb, exact without r_out: where a dividend is reduced
    if (!m && !r_out && exact && !(d_pad = (Fr *)lane_alloc(ctx, lane, nr * 32))) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    if (general) {
        d_g = (Fr *)lane_alloc(ctx, lane, m * 32);
        d_G = (Fr *)lane_alloc(ctx, lane, Tq * 32);
        d_A = (Fr *)lane_alloc(ctx, lane, Tq * 32);
        if (!d_g || !d_G || !d_A) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        if (want_r) {
            d_B = (Fr *)lane_alloc(ctx, lane, N * 32);
            d_af = (Fr *)lane_alloc(ctx, lane, N * 32);
            d_qf = (Fr *)lane_alloc(ctx, lane, N * 32);
            d_t0 = (Fr *)lane_alloc(ctx, lane, t0 * 32);
            d_t1 = (Fr *)lane_alloc(ctx, lane, t1 * 32);
            if (!d_B || !d_af || !d_qf || !d_t0 || !d_t1) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        }
    }

    // ---- what depends on the divisor alone ----
    const Fr *bd = (const Fr *)b;
    if (!in_dev) {
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_b, b, nb * 32, hipMemcpyHostToDevice, st));
        bd = d_b;
    }
    dv.f = d_f, dv.g = d_g, dv.G = d_G, dv.A = d_A, dv.B = d_B, dv.af = d_af, dv.qf = d_qf, dv.tmp0 = d_t0, dv.tmp1 = d_t1;
    if (m && nb == 1) {
        // f = b[0], Montgomery
        KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(fl_all), PD_T, 0, bd, nb - 1, 1, fl_all, d_f, fl_all, to_m);
        KZG_LAUNCH(ctx, st, "k_pd_inv_base", k_pd_inv_base, 1, PD_BASE, 0, d_f, 1u, 1u, d_f);  // d_f[0] = 1 / b[0]
    } else if (general) {
        KZG_TRY(poly_divisor_run(ctx, lane, bd, to_m, want_r, dv));
    }

    // ---- the dividends, a chunk at a time ----
    for (size_t b0 = 0; b0 < batch; b0 += C) {
        const size_t B = std::min(C, batch - b0);
        const Fr *src = (const Fr *)a + b0 * na;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * na * 32, hipMemcpyHostToDevice, st));
            src = d_in;
        }
        if (exact) KZG_LAUNCH(ctx, st, "k_pd_fill_int", k_pd_fill_int, pd_grid(B), PD_T, 0, d_exact, B, 1);
        Fr *qc = !want_q ? nullptr : (out_dev ? (Fr *)q_out + b0 * m : d_q);
        Fr *rc = !(r_out && nr) ? nullptr : (out_dev ? (Fr *)r_out + b0 * nr : d_r);
        for (size_t bi = 0; bi < B; bi++) {
            const Fr *ai = src + bi * na;
            Fr *qi = qc ? qc + bi * m : nullptr, *ri = rc ? rc + bi * nr : nullptr;
            int *ei = exact ? d_exact + bi : nullptr;
            if (!m) {  // na < nb: the remainder is the dividend
                Fr *dst = ri ? ri : d_pad;  // (without r_out the reduced dividend is only looked at for `exact`)
                if (!dst) continue;
                KZG_LAUNCH(ctx, st, "k_pd_load", k_pd_load, pd_grid(nr), PD_T, 0, ai, 0, 0, na, dst, nr, 0);
                if (ei) KZG_LAUNCH(ctx, st, "k_pd_rem", k_pd_rem, pd_grid(nr), PD_T, 0, dst, (const Fr *)nullptr, nr, (Fr *)nullptr, ei);
                continue;
            }
            if (nb == 1) {  // q = a / b[0]; no remainder
                if (want_q) KZG_LAUNCH(ctx, st, "k_pd_scale", k_pd_scale, pd_grid(na), PD_T, 0, ai, d_f, qi, na);
                continue;
            }
            KZG_TRY(poly_dividend_run(ctx, lane, dv, ai, want_q ? qi : nullptr, want_r, ri, ei ? ei : d_exact));
        }
        if (!out_dev) {
            if (stage_q) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)q_out + b0 * m, d_q, B * m * 32, hipMemcpyDeviceToHost, st));
            if (stage_r) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)r_out + b0 * nr, d_r, B * nr * 32, hipMemcpyDeviceToHost, st));
        }
        if (exact) KZG_HIP_CHECK(ctx, hipMemcpyAsync(exact + b0, d_exact, B * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}
