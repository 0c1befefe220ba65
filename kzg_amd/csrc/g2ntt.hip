// g2ntt.hip -- the G2 DFT: kzg_ntt_g2 (forward and scaled inverse transforms of arrays of G2 points, batched) and the transform
// behind kzg_srs_lagrange_from_monomial_g2 past the sizes its row-by-row sums handle.  The shape is the one of the G1 DFT
// (g1ntt.hip) on the Fq2 arithmetic of tower.h (G2Jacobian, 288 B a point):
//   k_g2ntt_load     affine in -> Jacobian, natural order for the DIF, bit-reversed for the DIT
//   k_g2ntt_dif      natural in -> bit-reversed out, half-size m = d/2 .. 2:  (x, y) -> (x + y, [w^e](x - y))
//   k_g2ntt_dit      bit-reversed in -> natural out, half-size m = 2 .. d/2:  t = [w^e] y, (x, y) -> (x + t, x - t)
//   k_g2ntt_trivial  half-size 1 (the twiddle is 1): two additions per butterfly
//   k_g2ntt_finish   the read-out: bit-reversed after a DIF, the [1/d] product of an inverse transform, affine (one inversion a point)
// `batch` arrays of d points sit one after the other and the array index is folded into the grid; every launch is a grid-stride
// loop over at most T threads; no point is permuted in memory.  Structured input (equal points, P and -P, identities) reaches
// every degenerate branch of g2_add / g2_dbl at the first stage, so all of them stay in the code path.
//
// Twiddle products.  psi, the untwist-Frobenius-twist endomorphism (x, y) -> (c_x conj x, c_y conj y) (Jacobian: Z -> conj Z),
// acts on the r-torsion as [z], z = -u the curve parameter (q = z mod r).  r = u^4 - u^2 + 1, so every k < r is
// k0 + k1 u + k2 u^2 + k3 u^3 with k_i < u < 2^64 by three divisions by u, and
//     [k]Q = [k0]Q - [k1]psi Q + [k2]psi^2 Q - [k3]psi^3 Q.
// Each k_i is recoded into 17 signed 4-bit digits in [-8, 7] (add 0x88..8, read nibbles, subtract 8; the carry out of bit 63 is
// the 17th).  One joint chain costs 64 doublings and at most 68 additions plus 7 operations for the table Q..8Q, against 256 and 64
// for signed digits over the whole scalar (option "g2_ntt_mul" = 1, kept for comparison): about 2.3 times fewer point operations
// (counted, not timed).  psi^i and the sign are applied to a table entry on the fly (psi^2: x times a constant of Fq, y negated).
// The twiddles are fixed per transform size and are split and recoded once per call (k_g2_twiddles).
//
// The table lives in an HBM scratch slot per thread, entries strided by the thread count.  T <= 2^17 threads (G2NTT_MAX_THREADS):
// 2^17 x 8 x 288 B = 302 MB of scratch at most.  kzg_ntt_g2 runs its batch in chunks of at most 2^20 points (option
// "group_ntt_chunk_points"), so its workspace -- points, affine results, staged input and output, scratch -- does not grow with
// `batch`.
#include <algorithm>

#include "glv.h"  // recode_add
#include "pairing_shared.h"

namespace kzg {

constexpr size_t G2NTT_MAX_THREADS = (size_t)1 << 17;   // scratch slots: 2^17 x 8 x 288 B = 302 MB
constexpr size_t G2NTT_CHUNK_POINTS = (size_t)1 << 20;  // points per chunk of kzg_ntt_g2
constexpr int G2NTT_TAB = 8;                            // Q, 2Q, .., 8Q

// a recoded scalar.  Split (route 0): w[2i], w[2i + 1] = k_i + 0x88..8 mod 2^64, bit i of top = its carry out.  Plain (route 1):
// w = k + 0x88..8 (< 2^256 for k < r), top = 0.
struct alignas(16) G2Tw {
    uint32_t w[8];
    uint32_t top, pad[3];
};

struct G2PsiConsts {
    Fq2 cx, cy, cx3;  // psi: x -> cx conj x, y -> cy conj y; psi^3: x -> cx3 conj x, y -> -cy conj y
    Fq cx2;           // psi^2: x -> cx2 x, y -> -y
};

static G2PsiConsts g2_psi_consts() {
    G2PsiConsts c;
    c.cx = Fq2{g2_psi_limb(0), g2_psi_limb(1)};
    c.cy = Fq2{g2_psi_limb(2), g2_psi_limb(3)};
    c.cx2 = g2_psi_limb(4);
    c.cx3 = Fq2{g2_psi_limb(5), g2_psi_limb(6)};
    return c;
}

// k (canonical, 8 limbs, < r) -> the four base-u digits, least significant first: restoring division, one bit per step
KZG_HD void g2_split_u(const uint32_t k[8], uint64_t out[4]) {
    uint32_t n[8];
    for (int i = 0; i < 8; i++) n[i] = k[i];
    for (int s = 0; s < 3; s++) {
        uint64_t rem = 0;
        uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int bit = 255; bit >= 0; bit--) {
            const uint64_t carry = rem >> 63;
            rem = (rem << 1) | ((n[bit >> 5] >> (bit & 31)) & 1u);
            if (carry || rem >= BLS_Z_ABS) {
                rem -= BLS_Z_ABS;
                q[bit >> 5] |= 1u << (bit & 31);
            }
        }
        out[s] = rem;
        for (int i = 0; i < 8; i++) n[i] = q[i];
    }
    out[3] = (uint64_t)n[0] | ((uint64_t)n[1] << 32);  // k < u^4: the third quotient is below u
}

KZG_HD G2Tw g2_recode(const uint32_t k[8], int route) {
    G2Tw t;
    t.top = 0;
    t.pad[0] = t.pad[1] = t.pad[2] = 0;
    if (route == 1) {
        for (int i = 0; i < 8; i++) t.w[i] = k[i];
        recode_add(t.w, 8);
        return t;
    }
    uint64_t ks[4];
    g2_split_u(k, ks);
    for (int i = 0; i < 4; i++) {
        t.w[2 * i] = (uint32_t)ks[i];
        t.w[2 * i + 1] = (uint32_t)(ks[i] >> 32);
        t.top |= recode_add(t.w + 2 * i, 2) << i;
    }
    return t;
}

// T <- (+-) psi^i(T) for the term of power i and a digit of sign `neg`: the odd powers carry a minus in the split, psi^2 and psi^3
// negate y themselves
static __device__ __noinline__ void g2_psi_term(G2Jacobian &T, int i, bool neg, const G2PsiConsts &c) {
    if (i == 1 || i == 3) {
        Fq2 t;
        f2_conj(t, T.x);
        f2_mul(T.x, t, i == 1 ? c.cx : c.cx3);
        f2_conj(t, T.y);
        f2_mul(T.y, t, c.cy);
        f2_conj(T.z, T.z);
    } else if (i == 2) {
        f2_mul_fq(T.x, T.x, c.cx2);
    }
    if (neg != (i == 1 || i == 2)) f2_neg(T.y, T.y);
}

// tab[e * st] = (e + 1) P, e < 8
static __device__ __noinline__ void g2_build_tab8(const G2Jacobian &P, G2Jacobian *tab, size_t st) {
    G2Jacobian p2, p3, p4, t;
    tab[0] = P;
    g2_dbl(p2, P);
    tab[st] = p2;
    g2_add(p3, p2, P);
    tab[2 * st] = p3;
    g2_dbl(p4, p2);
    tab[3 * st] = p4;
    g2_add(t, p4, P);
    tab[4 * st] = t;
    g2_dbl(t, p3);
    tab[5 * st] = t;
    g2_add(t, t, P);
    tab[6 * st] = t;
    g2_dbl(t, p4);
    tab[7 * st] = t;
}

// r = [k] P for the recoded k; r may be P
static __device__ __noinline__ void g2_tw_mul(G2Jacobian &r, const G2Jacobian &P, const G2Tw &w, int route, G2Jacobian *tab, size_t st,
                                              const G2PsiConsts &c) {
    g2_build_tab8(P, tab, st);
    G2Jacobian acc, T;
    g2_set_inf(acc);
    if (route == 1) {
#pragma nounroll
        for (int nib = 63; nib >= 0; nib--) {
#pragma nounroll
            for (int j = 0; j < 4; j++) g2_dbl(acc, acc);
            const int d = (int)((w.w[nib >> 3] >> (4 * (nib & 7))) & 15u) - 8;
            if (d) {
                T = tab[(size_t)((d < 0 ? -d : d) - 1) * st];
                if (d < 0) f2_neg(T.y, T.y);
                g2_add(acc, acc, T);
            }
        }
        r = acc;
        return;
    }
#pragma nounroll
    for (int i = 0; i < 4; i++)
        if ((w.top >> i) & 1u) {
            T = tab[0];
            g2_psi_term(T, i, false, c);
            g2_add(acc, acc, T);
        }
#pragma nounroll
    for (int nib = 15; nib >= 0; nib--) {
#pragma nounroll
        for (int j = 0; j < 4; j++) g2_dbl(acc, acc);
#pragma nounroll
        for (int i = 0; i < 4; i++) {
            const int d = (int)((w.w[2 * i + (nib >> 3)] >> (4 * (nib & 7))) & 15u) - 8;
            if (d) {
                T = tab[(size_t)((d < 0 ? -d : d) - 1) * st];
                g2_psi_term(T, i, d < 0, c);
                g2_add(acc, acc, T);
            }
        }
    }
    r = acc;
}

__device__ __forceinline__ size_t g2_brev(size_t i, uint32_t bits) {
    return bits ? (size_t)(__brevll((unsigned long long)i) >> (64 - bits)) : 0;
}

// recoded twiddles from a Montgomery power table
__global__ __launch_bounds__(64) void k_g2_twiddles(const Fr *pw, size_t count, int route, G2Tw *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Fr k = from_mont(pw[i]);
    out[i] = g2_recode(k.v, route);
}

// P[b d + i] = in[b d + (rev ? brev(i) : i)] as Jacobian points, b < batch
__global__ __launch_bounds__(64) void k_g2ntt_load(const G2Affine *in, size_t d, uint32_t bits, int rev, size_t batch, G2Jacobian *P) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < batch * d; u += nt) {
        const size_t b = u / d, i = u % d;
        G2Affine a = in[b * d + (rev ? g2_brev(i, bits) : i)];
        G2Jacobian j;
        g2_from_affine(j, a);
        P[u] = j;
    }
}

// tw: recoded w_d^e, e < d / 2.  `scratch` has gridDim.x * blockDim.x * 8 points; thread t owns the entries scratch[t + e nt].
__global__ __launch_bounds__(64) void k_g2ntt_dif(G2Jacobian *P, size_t d, size_t m, const G2Tw *tw, size_t batch, G2Jacobian *scratch,
                                                  int route, G2PsiConsts c) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t half = d / 2, work = batch * half;
    for (size_t u = tid; u < work; u += nt) {
        const size_t b = u / half, t = u % half;
        const size_t j = t / m, i = t % m;
        G2Jacobian *A = P + b * d;
        const size_t i0 = j * 2 * m + i, i1 = i0 + m;
        G2Jacobian x = A[i0], y = A[i1], s;
        g2_add(s, x, y);
        A[i0] = s;
        f2_neg(y.y, y.y);
        g2_add(s, x, y);
        const G2Tw w = tw[i * (d / (2 * m))];
        g2_tw_mul(s, s, w, route, scratch + tid, nt, c);
        A[i1] = s;
    }
}

__global__ __launch_bounds__(64) void k_g2ntt_dit(G2Jacobian *P, size_t d, size_t m, const G2Tw *tw, size_t batch, G2Jacobian *scratch,
                                                  int route, G2PsiConsts c) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t half = d / 2, work = batch * half;
    for (size_t u = tid; u < work; u += nt) {
        const size_t b = u / half, t = u % half;
        const size_t j = t / m, i = t % m;
        G2Jacobian *A = P + b * d;
        const size_t i0 = j * 2 * m + i, i1 = i0 + m;
        G2Jacobian x = A[i0], T = A[i1], s;
        const G2Tw w = tw[i * (d / (2 * m))];
        g2_tw_mul(T, T, w, route, scratch + tid, nt, c);
        g2_add(s, x, T);
        A[i0] = s;
        f2_neg(T.y, T.y);
        g2_add(s, x, T);
        A[i1] = s;
    }
}

// half-size 1, both directions: (x, y) -> (x + y, x - y)
__global__ __launch_bounds__(64) void k_g2ntt_trivial(G2Jacobian *P, size_t d, size_t batch) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t work = batch * (d / 2);  // the arrays are contiguous: pair t of all of them is P[2t], P[2t + 1]
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < work; t += nt) {
        G2Jacobian x = P[2 * t], y = P[2 * t + 1], s;
        g2_add(s, x, y);
        P[2 * t] = s;
        f2_neg(y.y, y.y);
        g2_add(s, x, y);
        P[2 * t + 1] = s;
    }
}

// out[b d + i] = [s] P[b d + (rev ? brev(i) : i)], affine; scale = 0: no product
__global__ __launch_bounds__(64) void k_g2ntt_finish(const G2Jacobian *P, size_t d, uint32_t bits, int rev, size_t batch, int scale, G2Tw s,
                                                     G2Jacobian *scratch, int route, G2PsiConsts c, G2Affine *out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t u = tid; u < batch * d; u += nt) {
        const size_t b = u / d, i = u % d;
        G2Jacobian Q = P[b * d + (rev ? g2_brev(i, bits) : i)];
        if (scale) g2_tw_mul(Q, Q, s, route, scratch + tid, nt, c);
        G2Affine a;
        g2_to_affine(a, Q);
        out[u] = a;
    }
}

// threads of one launch over `work` items: at most the cap (option "group_ntt_threads"), whole workgroups of 64
static size_t g2ntt_threads(const kzg_ctx *ctx, size_t work) {
    const size_t cap = ctx->opt_group_ntt_threads ? (size_t)ctx->opt_group_ntt_threads : G2NTT_MAX_THREADS;
    const size_t t = std::min(std::max<size_t>(work, 1), cap);
    return (t + 63) / 64 * 64;
}

// the workspace of transforms over `pts` = batch x d points
struct G2NttWork {
    G2Jacobian *P = nullptr, *scratch = nullptr;
    Fr *pw = nullptr;
    G2Tw *tw = nullptr;
    size_t threads = 0;
};
static size_t g2ntt_work_bytes(const kzg_ctx *ctx, size_t pts, size_t d) {
    const size_t half = d > 1 ? d / 2 : 1;
    return align_up(pts * sizeof(G2Jacobian), 256) + align_up(g2ntt_threads(ctx, pts) * G2NTT_TAB * sizeof(G2Jacobian), 256) +
           align_up(half * sizeof(Fr), 256) + align_up(half * sizeof(G2Tw), 256);
}
static int g2ntt_work_alloc(kzg_ctx *ctx, size_t pts, size_t d, G2NttWork *w) {
    const size_t half = d > 1 ? d / 2 : 1;
    w->threads = g2ntt_threads(ctx, pts);
    w->P = (G2Jacobian *)lane_alloc(ctx, 0, pts * sizeof(G2Jacobian));
    w->scratch = (G2Jacobian *)lane_alloc(ctx, 0, w->threads * G2NTT_TAB * sizeof(G2Jacobian));
    w->pw = (Fr *)lane_alloc(ctx, 0, half * sizeof(Fr));
    w->tw = (G2Tw *)lane_alloc(ctx, 0, half * sizeof(G2Tw));
    if (!w->P || !w->scratch || !w->pw || !w->tw) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    return KZG_OK;
}

// the recoded twiddles w^(+-e), e < d / 2, of the call's transform size
static int g2ntt_twiddles(kzg_ctx *ctx, hipStream_t st, uint32_t logd, bool inverse, int route, const G2NttWork &w) {
    if (logd < 2) return KZG_OK;  // sizes 1 and 2 have the trivial stage only
    const size_t half = (size_t)1 << (logd - 1);
    const Fr om = host_omega(logd);
    KZG_TRY(pow_table(ctx, st, inverse ? inv(om) : om, Fr::one(), half, w.pw));
    KZG_LAUNCH(ctx, st, "k_g2_twiddles", k_g2_twiddles, (unsigned)((half + 63) / 64), 64, 0, (const Fr *)w.pw, half, route, w.tw);
    return KZG_OK;
}

// d_in: B arrays of d affine points -> d_out: their transforms, affine, natural order.  Forward: DIF, read out bit-reversed;
// inverse: loaded bit-reversed, DIT over w^-1, the [1/d] product in the read-out.
static int g2ntt_transform(kzg_ctx *ctx, hipStream_t st, const G2Affine *d_in, uint32_t logd, size_t B, bool inverse, int route,
                           const G2NttWork &w, G2Affine *d_out) {
    const size_t d = (size_t)1 << logd, pts = B * d;
    const G2PsiConsts c = g2_psi_consts();
    const unsigned gp = (unsigned)(g2ntt_threads(ctx, pts) / 64), gb = (unsigned)(g2ntt_threads(ctx, pts / 2) / 64);
    KZG_LAUNCH(ctx, st, "k_g2ntt_load", k_g2ntt_load, gp, 64, 0, d_in, d, logd, inverse ? 1 : 0, B, w.P);
    if (d >= 2 && !inverse) {
        for (size_t m = d / 2; m >= 2; m /= 2)
            KZG_LAUNCH(ctx, st, "k_g2ntt_dif", k_g2ntt_dif, gb, 64, 0, w.P, d, m, (const G2Tw *)w.tw, B, w.scratch, route, c);
        KZG_LAUNCH(ctx, st, "k_g2ntt_trivial", k_g2ntt_trivial, gb, 64, 0, w.P, d, B);
    } else if (d >= 2) {
        KZG_LAUNCH(ctx, st, "k_g2ntt_trivial", k_g2ntt_trivial, gb, 64, 0, w.P, d, B);
        for (size_t m = 2; m <= d / 2; m *= 2)
            KZG_LAUNCH(ctx, st, "k_g2ntt_dit", k_g2ntt_dit, gb, 64, 0, w.P, d, m, (const G2Tw *)w.tw, B, w.scratch, route, c);
    }
    G2Tw s = {};
    const int scale = inverse && d > 1;
    if (scale) {
        const Fr dinv = from_mont(inv(from_u64<FrParams>((uint64_t)d)));
        s = g2_recode(dinv.v, route);
    }
    KZG_LAUNCH(ctx, st, "k_g2ntt_finish", k_g2ntt_finish, gp, 64, 0, (const G2Jacobian *)w.P, d, logd, inverse ? 0 : 1, B, scale, s,
               w.scratch, route, c, d_out);
    return KZG_OK;
}

int g2_lagrange_dft(kzg_ctx *ctx, const G2Affine *d_in, uint32_t log_d, G2Affine *d_out) {
    if (log_d > G2NTT_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, "G2 DFT: log_n <= 20 (documented limit)");
    const size_t d = (size_t)1 << log_d;
    hipStream_t st = ctx->lanes[0].stream;
    KZG_TRY(lane_reserve(ctx, 0, g2ntt_work_bytes(ctx, d, d) + 65536));
    G2NttWork w;
    KZG_TRY(g2ntt_work_alloc(ctx, d, d, &w));
    const int route = ctx->opt_g2_ntt_mul;
    KZG_TRY(g2ntt_twiddles(ctx, st, log_d, true, route, w));
    KZG_TRY(g2ntt_transform(ctx, st, d_in, log_d, 1, true, route, w, d_out));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_ntt_g2(kzg_ctx *ctx, const void *points, uint32_t log_n, size_t batch, int inverse, int pfmt, int flags, void *out,
                          int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t psz = g2_point_bytes(pfmt), osz = g2_point_bytes(ofmt);
    if (!psz || !osz) return fail(ctx, KZG_ERR_SHAPE, "unknown G2 point format");
    if (log_n > G2NTT_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g2: log_n <= 20 (documented limit)");
    if (batch == 0) return KZG_OK;
    if (!points || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g2: NULL buffer");
    const size_t d = (size_t)1 << log_n;
    if (batch > (SIZE_MAX / 288) >> log_n) return fail(ctx, KZG_ERR_SHAPE, "batch too large");
    if (out == points && psz != osz) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g2: in place needs formats of equal size");
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t cpts = ctx->opt_group_ntt_chunk_points ? (size_t)ctx->opt_group_ntt_chunk_points : G2NTT_CHUNK_POINTS;
    const size_t chunk = std::max<size_t>(1, cpts / d), B0 = std::min(chunk, batch), pts0 = B0 * d;
    KZG_TRY(lane_reserve(ctx, 0, g2ntt_work_bytes(ctx, pts0, d) + 2 * align_up(pts0 * sizeof(G2Affine), 256) + align_up(pts0 * osz, 256) +
                                     (in_dev ? 0 : align_up(pts0 * psz, 256)) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    G2NttWork w;
    KZG_TRY(g2ntt_work_alloc(ctx, pts0, d, &w));
    G2Affine *dec = (G2Affine *)lane_alloc(ctx, 0, pts0 * sizeof(G2Affine)), *res = (G2Affine *)lane_alloc(ctx, 0, pts0 * sizeof(G2Affine));
    uint8_t *enc = (uint8_t *)lane_alloc(ctx, 0, pts0 * osz);  // also with KZG_OUT_DEVICE: `out` may be `points`, which the next pass reads
    uint8_t *d_raw = in_dev ? nullptr : (uint8_t *)lane_alloc(ctx, 0, pts0 * psz);
    int *bad = (int *)lane_alloc(ctx, 0, 256);
    if (!dec || !res || !enc || (!in_dev && !d_raw) || !bad) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const int route = ctx->opt_g2_ntt_mul;
    const uint8_t *src = (const uint8_t *)points;
    uint8_t *dst = (uint8_t *)out;
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    KZG_TRY(g2ntt_twiddles(ctx, st, log_n, inverse != 0, route, w));
    // Nothing is written before every point has passed the check.  One chunk: decoded once, checked, transformed.  Several: a pass
    // that only checks, then the transforms on points decoded again without the checks.
    const bool two_pass = batch > chunk;
    int hbad = 0;
    for (int pass = two_pass ? 0 : 1; pass < 2; pass++) {
        const int level = (two_pass && pass == 1) ? (int)POINTS_TRUSTED : untrusted_level(ctx);
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t B = std::min(chunk, batch - b0), n = B * d;
            const uint8_t *raw = src + b0 * d * psz;
            if (!in_dev) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_raw, raw, n * psz, hipMemcpyHostToDevice, st));
                raw = d_raw;
            }
            KZG_TRY(g2_decode_run(ctx, st, raw, n, pfmt, dec, bad, level));
            if (pass == 0) continue;
            if (!two_pass) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
                KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
                if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, "a G2 point failed to decode, is not on the twist or not in the r-torsion subgroup");
            }
            KZG_TRY(g2ntt_transform(ctx, st, dec, log_n, B, inverse != 0, route, w, res));
            KZG_TRY(g2_encode_run(ctx, st, res, n, ofmt, enc));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(dst + b0 * d * osz, enc, n * osz, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        }
        if (pass == 0) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
            if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, "a G2 point failed to decode, is not on the twist or not in the r-torsion subgroup");
        }
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

#ifdef KZG_TEST_HOOKS
#include "../../include/kzg_mi355x_test.h"

namespace kzg {
__global__ __launch_bounds__(64) void k_test_g2_mul_gls(const G2Affine *p, const Fr *k, size_t n, int route, G2Jacobian *scratch, G2PsiConsts c,
                                                        G2Affine *o) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid; i < n; i += nt) {
        G2Jacobian P;
        g2_from_affine(P, p[i]);
        const G2Tw w = g2_recode(k[i].v, route);
        g2_tw_mul(P, P, w, route, scratch + tid, nt, c);
        G2Affine a;
        g2_to_affine(a, P);
        o[i] = a;
    }
}
}  // namespace kzg

extern "C" int kzg_test_g2_mul_gls(kzg_ctx *ctx, const void *pts_affine, const void *k_canonical, size_t n, int route, void *out_affine) {
    if (!ctx || !pts_affine || !k_canonical || !out_affine || !n || n > 65536 || (route != 0 && route != 1)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t threads = g2ntt_threads(ctx, n);
    KZG_TRY(lane_reserve(ctx, 0, n * (2 * sizeof(G2Affine) + 32) + threads * G2NTT_TAB * sizeof(G2Jacobian) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    G2Affine *dp = (G2Affine *)lane_alloc(ctx, 0, n * sizeof(G2Affine)), *dout = (G2Affine *)lane_alloc(ctx, 0, n * sizeof(G2Affine));
    Fr *dk = (Fr *)lane_alloc(ctx, 0, n * 32);
    G2Jacobian *scratch = (G2Jacobian *)lane_alloc(ctx, 0, threads * G2NTT_TAB * sizeof(G2Jacobian));
    if (!dp || !dout || !dk || !scratch) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dp, pts_affine, n * sizeof(G2Affine), hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dk, k_canonical, n * 32, hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_test_g2_mul_gls", k_test_g2_mul_gls, (unsigned)(threads / 64), 64, 0, (const G2Affine *)dp, (const Fr *)dk, n, route,
               scratch, g2_psi_consts(), dout);
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out_affine, dout, n * sizeof(G2Affine), hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    return KZG_OK;
}

// the recoding of one canonical scalar below r, on the calling thread: words[0..3] = k_0..k_3 (k = sum k_i u^i), digits[17 i + j] = digit
// j of k_i (least significant first, the 17th is the carry)
extern "C" int kzg_test_g2_gls_recode(const void *k_canonical, uint64_t *words, int8_t *digits) {
    if (!k_canonical || !words || !digits) return KZG_ERR_SHAPE;
    uint32_t k[8];
    memcpy(k, k_canonical, 32);
    g2_split_u(k, words);
    const G2Tw t = g2_recode(k, 0);
    for (int i = 0; i < 4; i++) {
        for (int j = 0; j < 16; j++) digits[17 * i + j] = (int8_t)((int)((t.w[2 * i + (j >> 3)] >> (4 * (j & 7))) & 15u) - 8);
        digits[17 * i + 16] = (int8_t)((t.top >> i) & 1u);
    }
    return KZG_OK;
}
#endif  // KZG_TEST_HOOKS
