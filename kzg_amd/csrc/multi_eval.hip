// multi_eval.hip -- coefficient-form polynomials at many points in one call (kzg_poly_multi_eval): ys[b k + i] = p_b(xs[i]), the
// Vandermonde matrix-vector product of Polynomial::multi_eval (src/polynomial.rs:229-233).  DESIGN.md section 3.4e.
//
// n k field products per polynomial, no dependency between points, every coefficient shared by all of them.  The coefficients are cut
// into segments of L = 2^l; stage A (k_me_partials) is Horner per (point, segment), S[s][i] = sum_j a_(s L + j) x_i^j, highest index
// first; stage B (k_me_combine) is Horner over the segments in x^L, y_i = sum_s S[s][i] (x_i^L)^s.  In stage A the point lives in the
// lane's registers and the coefficients come from an LDS tile the workgroup loads once with whole-line loads: with 64 or more points
// a wave's lanes are 64 points on ONE segment and read the same LDS address (a broadcast: no bank conflicts); with fewer points a
// workgroup's lanes are (point, segment) pairs over 256 / k neighbouring segments, so the parallelism comes from the segments and a k
// of 1..63 still fills waves (the tile rows of the segments are one word apart in their bank).
//
// Arithmetic (A/B in profiles/multi_eval_ab_*.json): stage A multiplies by a constant of the lane, so it is the Shoup
// product of fr29.h -- (w, wp) per point prepared on the host -- on 9 x 29-bit limbs with the sum left unreduced between products; the
// data keeps the form it has.  -DKZG_ME_MONT builds stage A on the library's Montgomery mul / add instead.  Stage B is Montgomery:
// its multiplier x^L is made by the lane (l squarings).  Coefficients may be any 256-bit value and count as their residue; what
// leaves either kernel is the canonical residue.
#include <algorithm>

#include "common.h"
#include "fr29.h"

namespace kzg {

constexpr int ME_T = 256;          // threads per workgroup, both kernels
constexpr int ME_TILE = 512;       // coefficients in an LDS tile at most: 18 KiB of nine-limb values, eight workgroups per CU
constexpr int ME_BLOCKS = 1024;    // workgroups stage A is planned for: 256 CUs x four waves per SIMD (the dependent multiply-add
                                   // chain of one wave leaves issue slots to the next; beyond four nothing is gained)
constexpr size_t ME_POINTS = 4096; // points per pass at most (the partial sums of a pass are segments x points)
constexpr int MEB_P = 16, MEB_R = 16;  // stage B: points x parts of the segment range per workgroup

struct MePoint {                   // a point as stage A's Shoup multiplier
    Fr29 w, wp;
};

// stage A on 29-bit limbs: acc (limbs below 2^30, value below 2^256 + 2r) -> acc x + a
struct MeShoup {
    typedef Fr29 Acc;
    typedef MePoint Point;
    static constexpr int W = 9, PAD = 1;  // words per tile entry; words between the tile rows of neighbouring segments
    static __device__ __forceinline__ Point point(const Fr *, const MePoint *pts, uint32_t i) { return pts[i]; }
    static __device__ __forceinline__ Acc zero() { return fr29_zero(); }
    static __device__ __forceinline__ void put(uint32_t *slot, const Fr &raw) {
        const Fr29 v = fr29_unpack(raw);
#pragma unroll
        for (int i = 0; i < W; i++) slot[i] = v.v[i];
    }
    static __device__ __forceinline__ Acc step(const Acc &acc, const Point &x, const uint32_t *slot) {
        Fr29 a;
#pragma unroll
        for (int i = 0; i < W; i++) a.v[i] = slot[i];
        return fr29_add_lazy(mulshoup29(acc, x.w, x.wp), a);
    }
    static __device__ __forceinline__ Fr finish(const Acc &acc) { return fr29_canonical(fr29_normalize(acc)); }
};

// stage A on the saturated Montgomery form: residues below r throughout
struct MeMont {
    typedef Fr Acc;
    typedef Fr Point;
    static constexpr int W = 8, PAD = 4;
    static __device__ __forceinline__ Point point(const Fr *xs, const MePoint *, uint32_t i) { return xs[i]; }
    static __device__ __forceinline__ Acc zero() { return Fr::zero(); }
    static __device__ __forceinline__ void put(uint32_t *slot, Fr raw) {
        raw = fr_residue(raw);  // any value below 2^256 < 3r (field.h)
#pragma unroll
        for (int i = 0; i < W; i++) slot[i] = raw.v[i];
    }
    static __device__ __forceinline__ Acc step(const Acc &acc, const Point &x, const uint32_t *slot) {
        Fr a;
#pragma unroll
        for (int i = 0; i < W; i++) a.v[i] = slot[i];
        return add(mul(acc, x), a);
    }
    static __device__ __forceinline__ Fr finish(const Acc &acc) { return acc; }
};

#ifdef KZG_ME_MONT
typedef MeMont MeArith;
#else
typedef MeShoup MeArith;
#endif

// S[(b nseg + s) kc + i] = sum_{j < L} coeffs[b pstride + s L + j] x_i^j (coefficients beyond n are zero).
// grid (ceil(nseg / Q), ceil(kc / P), polynomials); a workgroup is P points x Q neighbouring segments: P = 256, Q = 1 (kc >= 64) or
// P = kc, Q = 256 / kc.  A segment goes through LDS in tiles of TC = 2^log_tc coefficients, the last tile first.
template <class A>
__global__ __launch_bounds__(ME_T) void k_me_partials(const Fr *coeffs, size_t n, size_t pstride, const Fr *xs, const MePoint *pts, uint32_t kc,
                                                      uint32_t P, uint32_t Q, uint32_t log_L, uint32_t log_tc, uint32_t nseg, Fr *S) {
    extern __shared__ uint32_t me_lds[];
    const uint32_t t = threadIdx.x, q = t / P, p = blockIdx.y * P + (t - q * P);
    const uint32_t seg0 = blockIdx.x * Q, seg = seg0 + q;
    const bool active = q < Q && p < kc && seg < nseg;
    const Fr *poly = coeffs + (size_t)blockIdx.z * pstride;
    const size_t L = (size_t)1 << log_L, base = (size_t)seg0 * L;     // base < n: seg0 < nseg
    const uint32_t TC = 1u << log_tc, RS = TC * A::W + A::PAD;
    const size_t len0 = n - base < L ? n - base : L;                       // the workgroup's first segment is its longest
    const uint32_t ntile = (uint32_t)((len0 + TC - 1) >> log_tc);
    const typename A::Point x = A::point(xs, pts, p < kc ? p : 0);
    typename A::Acc acc = A::zero();
    for (uint32_t c = ntile; c-- > 0;) {
        __syncthreads();  // the tile before this one is consumed
        for (uint32_t e = t; e < (Q << log_tc); e += ME_T) {
            const uint32_t r = e >> log_tc, j = e & (TC - 1);
            const size_t idx = base + (size_t)r * L + ((size_t)c << log_tc) + j;
            A::put(me_lds + r * RS + j * A::W, idx < n ? poly[idx] : Fr::zero());
        }
        __syncthreads();
        if (active) {
            const uint32_t *row = me_lds + q * RS;
#pragma unroll 1
            for (uint32_t j = TC; j-- > 0;) acc = A::step(acc, x, row + j * A::W);
        }
    }
    if (active) S[((size_t)blockIdx.z * nseg + seg) * kc + p] = A::finish(acc);
}

// out[b ostride + i] = sum_{s < nseg} S[(b nseg + s) kc + i] X_i^s, X_i = x_i^(2^log_L).  grid (ceil(kc / MEB_P), polynomials); a
// workgroup is MEB_P points x MEB_R parts of G = 2^log_G segments each (MEB_R G >= nseg): Horner over a part, then over the parts in
// X^G by the lanes of part 0 -- depth G + MEB_R + log_L + log_G products instead of nseg.
__global__ __launch_bounds__(ME_T) void k_me_combine(const Fr *S, const Fr *xs, uint32_t kc, uint32_t nseg, uint32_t log_L, uint32_t log_G, Fr *out,
                                                     size_t ostride) {
    __shared__ Fr sh[ME_T];
    const uint32_t t = threadIdx.x, r = t / MEB_P, p = blockIdx.x * MEB_P + t % MEB_P;
    const bool active = p < kc;
    Fr X = xs[active ? p : 0];
    for (uint32_t i = 0; i < log_L; i++) X = sqr(X);
    const Fr *Sb = S + (size_t)blockIdx.y * nseg * kc + p;
    const uint64_t lo = (uint64_t)r << log_G, top = lo + ((uint64_t)1 << log_G), hi = top < nseg ? top : nseg;
    Fr acc = Fr::zero();
    if (active)
        for (uint64_t s = hi; s > lo; s--) acc = add(mul(acc, X), Sb[(size_t)(s - 1) * kc]);
    sh[t] = acc;
    __syncthreads();
    if (r == 0 && active) {
        Fr XG = X;
        for (uint32_t i = 0; i < log_G; i++) XG = sqr(XG);
        Fr y = sh[(MEB_R - 1) * MEB_P + t];
        for (int rr = MEB_R - 2; rr >= 0; rr--) y = add(mul(y, XG), sh[rr * MEB_P + t]);
        out[(size_t)blockIdx.y * ostride + p] = y;
    }
}

// ---------------------------------------------------------------------------------------------
// the plan of a call: points and polynomials per pass, the segment length, the tile
// ---------------------------------------------------------------------------------------------
struct MePlan {
    size_t kc, bc;                          // points / polynomials per pass
    uint32_t P, Q, pblocks;                 // workgroup shape (k_me_partials) and workgroups per segment range
    uint32_t log_L, log_tc, nseg, log_G;
    size_t lds_bytes, partial_bytes;
};

static uint32_t log2_ceil64(size_t x) {
    uint32_t l = 0;
    while (((size_t)1 << l) < x) l++;
    return l;
}

// The grid of stage A is (segments / Q) x pblocks x polynomials workgroups; the segment length is the power of two that brings it
// to ME_BLOCKS.  Polynomials per pass: as many as fill the grid without cutting segments (and, staged from the host, as fit 256 MiB).
// The partial sums of a pass are nseg x kc x bc <= 256 (ME_BLOCKS + pblocks bc) scalars: 17 MiB at most under automatic planning.
static MePlan me_plan(size_t n, size_t k, size_t batch, int opt_segment, int opt_chunk, bool in_dev) {
    MePlan pl;
    pl.kc = std::min(k, opt_chunk ? std::min<size_t>((size_t)opt_chunk, ME_POINTS) : ME_POINTS);
    const bool wide = pl.kc >= 64;
    pl.P = wide ? ME_T : (uint32_t)pl.kc;
    pl.Q = wide ? 1 : ME_T / (uint32_t)pl.kc;
    pl.pblocks = wide ? (uint32_t)((pl.kc + ME_T - 1) / ME_T) : 1;
    pl.bc = std::min<size_t>(batch, std::max<size_t>(1, ME_BLOCKS / pl.pblocks));
    if (!in_dev) pl.bc = std::min<size_t>(pl.bc, std::max<size_t>(1, ((size_t)256 << 20) / (n * 32)));
    if (opt_segment) {
        pl.log_L = log2_ceil64((size_t)opt_segment);
    } else {
        const size_t want = std::max<size_t>(1, (size_t)ME_BLOCKS * pl.Q / (pl.pblocks * pl.bc));  // segments
        pl.log_L = std::max<uint32_t>(log2_ceil64((n + want - 1) / want), wide ? 6 : 3);
        // Few points cannot fill the grid however short the segments: there the call is as long as one lane's L steps of stage A
        // (0.43 us each, measured) plus its nseg / MEB_R steps of stage B (1.1 us each), least near L = sqrt(n / 6).
        if (!wide)
            while (((size_t)6 << (2 * pl.log_L)) < n) pl.log_L++;
    }
    pl.nseg = (uint32_t)((n + ((size_t)1 << pl.log_L) - 1) >> pl.log_L);
    uint32_t log_tc = 0;
    while ((2u << log_tc) * pl.Q <= (uint32_t)ME_TILE) log_tc++;  // the largest power of two with TC Q <= ME_TILE (Q <= 256: TC >= 2)
    pl.log_tc = std::min(log_tc, pl.log_L);
    pl.log_G = log2_ceil64((pl.nseg + MEB_R - 1) / MEB_R);
    pl.lds_bytes = (size_t)pl.Q * (((size_t)MeArith::W << pl.log_tc) + MeArith::PAD) * 4;
    pl.partial_bytes = align_up((size_t)pl.nseg * pl.kc * pl.bc * 32, 256);
    return pl;
}

// Up to this many values (points x polynomials) the driver takes one poly_eval_run scan per value instead (the bytes are the same).
// Measured at 2^20 (profiles/multi_eval_small.json): a scan costs 0.061 ms; the two kernels 0.44-0.49 ms from 4 points on whatever
// the batch (their lanes are not full before ~64 values), 0.85 / 0.75 ms at one / two points (tiles of two / four coefficients).  A
// forced segment or points chunk (the two options) always takes the kernels.
static size_t me_loop_values(size_t k) { return k <= 2 ? 12 : 7; }

static int me_host_point(kzg_ctx *ctx, const void *s, int sfmt, Fr *mont) {
    Fr v;
    memcpy(v.v, s, 32);
    if (!is_canonical(v)) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_multi_eval: a point is not below r");
    *mont = sfmt == KZG_FR_CANONICAL_LE_32 ? to_mont(v) : v;
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_poly_multi_eval(kzg_ctx *ctx, const void *coeffs, size_t n, size_t batch, const void *xs, size_t k, int sfmt, int flags,
                                   void *ys_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    if (!coeffs || !xs || !ys_out) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_multi_eval: NULL coeffs, xs or ys_out");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, "empty polynomial");
    if (n > ((size_t)1 << 28)) return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_multi_eval: polynomials of up to 2^28 coefficients");
    if (k > ((size_t)1 << 40) || batch > ((size_t)1 << 40) / n || (k && batch > ((size_t)1 << 50) / k))
        return fail(ctx, KZG_ERR_SHAPE, "kzg_poly_multi_eval: batch x n or batch x k too large");
    std::vector<Fr> xm;
    std::vector<MePoint> hp;
    try {  // (no exception may leave through the C ABI)
        xm.resize(k);
#ifndef KZG_ME_MONT
        hp.resize(k);
#endif
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the points");
    }
    for (size_t i = 0; i < k; i++) {
        KZG_TRY(me_host_point(ctx, (const uint8_t *)xs + 32 * i, sfmt, &xm[i]));
#ifndef KZG_ME_MONT
        fr29_shoup_from_twiddle(fr29_twiddle_from_mont(xm[i]), hp[i].w, hp[i].wp);
#endif
    }
    if (k == 0 || batch == 0) return KZG_OK;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const int opt_segment = ctx->opt_multi_eval_segment, opt_chunk = ctx->opt_multi_eval_points_chunk;

    if (k * batch <= me_loop_values(k) && !opt_segment && !opt_chunk) {  // few values: one Horner scan each
        const size_t horner = (n / 2048 + 4) * 64 + 4096;
        KZG_TRY(lane_reserve(ctx, lane, (in_dev ? 0 : align_up(n * 32, 256)) + align_up(k * 32, 256) + horner + 65536));
        Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, n * 32);
        Fr *d_y = (Fr *)lane_alloc(ctx, lane, k * 32);
        if ((!in_dev && !d_in) || !d_y) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        const size_t mark = ctx->lanes[lane].arena_used;
        for (size_t b = 0; b < batch; b++) {
            const Fr *src = (const Fr *)coeffs + b * n;
            if (!in_dev) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, n * 32, hipMemcpyHostToDevice, st));
                src = d_in;
            }
            Fr *dst = out_dev ? (Fr *)ys_out + b * k : d_y;
            for (size_t i = 0; i < k; i++) {
                ctx->lanes[lane].arena_used = mark;  // the scans follow one another on the stream: they share their scratch
                KZG_TRY(poly_eval_run(ctx, lane, src, n, xm[i], dst + i));
            }
            if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((Fr *)ys_out + b * k, d_y, k * 32, hipMemcpyDeviceToHost, st));
        }
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
        if (ctx->prof) prof_collect(ctx);
        return KZG_OK;
    }

    const MePlan pl = me_plan(n, k, batch, opt_segment, opt_chunk, in_dev);
    KZG_TRY(lane_reserve(ctx, lane, (in_dev ? 0 : align_up(pl.bc * n * 32, 256)) + pl.partial_bytes + align_up(pl.kc * sizeof(MePoint), 256) +
                                        align_up(pl.kc * 32, 256) + (out_dev ? 0 : align_up(pl.bc * pl.kc * 32, 256)) + 65536));
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, pl.bc * n * 32);
    Fr *d_S = (Fr *)lane_alloc(ctx, lane, pl.partial_bytes);
    MePoint *d_pts = (MePoint *)lane_alloc(ctx, lane, pl.kc * sizeof(MePoint));
    Fr *d_xs = (Fr *)lane_alloc(ctx, lane, pl.kc * 32);
    Fr *d_y = out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, pl.bc * pl.kc * 32);
    if ((!in_dev && !d_in) || !d_S || !d_pts || !d_xs || (!out_dev && !d_y)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const uint32_t gx = (pl.nseg + pl.Q - 1) / pl.Q;
    for (size_t b0 = 0; b0 < batch; b0 += pl.bc) {
        const size_t B = std::min(pl.bc, batch - b0);
        const Fr *src = (const Fr *)coeffs + b0 * n;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, src, B * n * 32, hipMemcpyHostToDevice, st));
            src = d_in;
        }
        for (size_t p0 = 0; p0 < k; p0 += pl.kc) {
            const size_t K = std::min(pl.kc, k - p0);
            if (b0 == 0 || k > pl.kc) {  // (one pass of points: they are resident after the first chunk of polynomials)
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_xs, xm.data() + p0, K * 32, hipMemcpyHostToDevice, st));
                if (!hp.empty()) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_pts, hp.data() + p0, K * sizeof(MePoint), hipMemcpyHostToDevice, st));
            }
            // a short last pass keeps the workgroup shape of the plan: lanes beyond K idle
            const uint32_t gy = pl.pblocks == 1 ? 1 : (uint32_t)((K + ME_T - 1) / ME_T);
            KZG_LAUNCH(ctx, st, "k_me_partials", k_me_partials<MeArith>, dim3(gx, gy, (unsigned)B), ME_T, pl.lds_bytes, src, n, n, d_xs, d_pts, (uint32_t)K,
                       pl.P, pl.Q, pl.log_L, pl.log_tc, pl.nseg, d_S);
            Fr *dst = out_dev ? (Fr *)ys_out + b0 * k + p0 : d_y;
            const size_t ostride = out_dev ? k : K;
            KZG_LAUNCH(ctx, st, "k_me_combine", k_me_combine, dim3((unsigned)((K + MEB_P - 1) / MEB_P), (unsigned)B), ME_T, 0, d_S, d_xs, (uint32_t)K, pl.nseg,
                       pl.log_L, pl.log_G, dst, ostride);
            if (!out_dev) {
                uint8_t *h = (uint8_t *)ys_out + (b0 * k + p0) * 32;
                if (K == k) KZG_HIP_CHECK(ctx, hipMemcpyAsync(h, d_y, B * K * 32, hipMemcpyDeviceToHost, st));
                else KZG_HIP_CHECK(ctx, hipMemcpy2DAsync(h, k * 32, d_y, K * 32, K * 32, B, hipMemcpyDeviceToHost, st));
            }
        }
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}
