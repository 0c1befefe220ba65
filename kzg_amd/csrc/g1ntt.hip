// g1ntt.hip -- the G1 DFT and its callers: FK20 (Feist-Khovratovich), every opening of one polynomial over its whole evaluation
// domain in O(N log N) group operations, at single points (described first) and at cosets (further down), both through one plan
// representation, one setup and one chunked run function; and compute_lagrange_basis from the monomial SRS (at the end).
//
// Domain N = 2^k, w = compute_omega(N).omega, coefficients c_0..c_{N-1} (zero-padded from n <= N), s_i = [tau^i]G.  The witness
// at w^m is pi_m = [q_m(tau)] with q_m = (p - p(w^m)) / (X - w^m), and pi = DFT_N(H) with H_k = sum_{i <= N-2-k} c_{i+k+1} s_i
// (H_{N-1} = O).  H is the first half of the length-2N cyclic convolution of
//     x_j = s_{N-2-j} (j <= N-2), O (j >= N-1)          (per plan: Xh = DFT_2N(x) over G1, stored bit-reversed)
//     y_0 = c_{N-1}, y_1..y_N = 0, y_t = c_{t-N-1}        (per polynomial, in Fr: yh = DFT_2N(y) / 2N, permuted bit-reversed)
// so per polynomial:  Hh_j = yh_j Xh_j (bit-reversed),  H = iDFT_2N(Hh) as DIT (bit-reversed in, natural out, first half only),
// pi = DFT_N(H) as DIF (natural in, bit-reversed out), read out bit-reversed by the emit kernel.  No 224-byte point is permuted
// and no G1 stage carries a scale factor (the 1/2N is folded into yh).  s_i beyond the SRS is the identity: exact for every
// polynomial with n - 1 <= len(srs), because c_{i+k+1} s_i is non-zero only for i <= n - 2.
//
// Butterflies multiply by a fixed twiddle, so each twiddle is split once per plan by the GLV endomorphism of BLS12-381 G1:
// lambda = z^2 - 1 (r = lambda^2 + lambda + 1), phi(x, y) = (beta x, y) = [lambda](x, y); k = k2 lambda + k1 with k1, k2 < 2^128
// by plain division.  Both halves are recoded into signed 4-bit digits in [-8, 7] (add 0x88..8, read nibbles, subtract 8): one
// joint double-and-add over P and phi(P) costs 128 doublings and <= 64 additions against 256 and 64 for a 4-bit window over the
// full scalar, and the eight multiples P..8P are the whole per-thread table (phi and the sign are applied on the fly: one Fq
// product per phi digit).  The table lives in an HBM scratch slot per thread of a grid-stride launch, entries strided by the
// thread count so that a wave's reads and writes are coalesced.  The stage with half-size 1 has trivial twiddles only and its own
// kernel of two additions per butterfly.  The point-wise products (varying scalars) use the same signed digits over 256 bits.
#include <algorithm>
#include <optional>
#include <string>

#include "common.h"
#include "emit.h"
#include "glv.h"

namespace kzg {

constexpr size_t G1NTT_MAX_THREADS = (size_t)1 << 18;  // grid-stride launches: bounds the scratch table (2^18 x 8 x 224 B = 470 MB)
constexpr size_t FK20_CHUNK_POINTS = (size_t)1 << 21;  // polynomials per chunk: chunk x 2N points of workspace at most (470 MB)
constexpr size_t FK20_MAX_CHUNK = 4096;
constexpr uint32_t FK20_MAX_LOG = 22;

__device__ __forceinline__ size_t brev(size_t i, uint32_t bits) {
    return bits ? (size_t)(__brevll((unsigned long long)i) >> (64 - bits)) : 0;
}

// ---- G1 DFT stages over `batch` arrays of d points (array b at P + b * pstride) -------------------------------------------
// tw: recoded w_D^e, e < D / 2, for a transform of size D >= d; tws = D / d (so w_d^e = tw[e * tws]).
// DIF, natural in -> bit-reversed out, half-size m = d/2 .. 2:  (x, y) -> (x + y, [w^e](x - y)),  e = i d / 2m
__global__ __launch_bounds__(256) void k_g1ntt_dif(MsmPoint *P, size_t pstride, size_t d, size_t m, const GlvTw *tw, size_t tws,
                                                   size_t batch, MsmPoint *scratch, Fq30 beta) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t half = d / 2, work = batch * half;
    for (size_t u = tid; u < work; u += nt) {
        const size_t b = u / half, t = u % half;
        const size_t j = t / m, i = t % m;
        MsmPoint *A = P + b * pstride;
        const size_t i0 = j * 2 * m + i, i1 = i0 + m;
        const MsmPoint x = A[i0], y = A[i1];
        A[i0] = g1_add30(x, y);
        MsmPoint D = y;
        D.y = neg30(D.y);
        D = g1_add30(x, D);
        A[i1] = glv_mul(D, tw[i * (d / (2 * m)) * tws], scratch + tid, nt, beta);
    }
}

// DIT, bit-reversed in -> natural out, half-size m = 2 .. d/2:  t = [w^e] y, (x, y) -> (x + t, x - t).  half_out: the last stage
// of a transform of which only the first half is wanted (x + t only).
__global__ __launch_bounds__(256) void k_g1ntt_dit(MsmPoint *P, size_t pstride, size_t d, size_t m, const GlvTw *tw, size_t tws,
                                                   size_t batch, MsmPoint *scratch, Fq30 beta, int half_out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t half = d / 2, work = batch * half;
    for (size_t u = tid; u < work; u += nt) {
        const size_t b = u / half, t = u % half;
        const size_t j = t / m, i = t % m;
        MsmPoint *A = P + b * pstride;
        const size_t i0 = j * 2 * m + i, i1 = i0 + m;
        const MsmPoint x = A[i0];
        MsmPoint T = glv_mul(A[i1], tw[i * (d / (2 * m)) * tws], scratch + tid, nt, beta);
        A[i0] = g1_add30(x, T);
        if (!half_out) {
            T.y = neg30(T.y);
            A[i1] = g1_add30(x, T);
        }
    }
}

// half-size 1, both directions (the twiddle is 1): (x, y) -> (x + y, x - y)
__global__ __launch_bounds__(256) void k_g1ntt_trivial(MsmPoint *P, size_t pstride, size_t d, size_t batch, int half_out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t half = d / 2, work = batch * half;
    for (size_t u = tid; u < work; u += nt) {
        const size_t b = u / half, t = u % half;
        MsmPoint *A = P + b * pstride;
        const MsmPoint x = A[2 * t], y = A[2 * t + 1];
        A[2 * t] = g1_add30(x, y);
        if (!half_out) {
            MsmPoint D = y;
            D.y = neg30(D.y);
            A[2 * t + 1] = g1_add30(x, D);
        }
    }
}

// recoded twiddles from a Montgomery power table
__global__ __launch_bounds__(256) void k_glv_twiddles(const Fr *pw, size_t count, GlvTw *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Fr k = from_mont(pw[i]);
    out[i] = glv_recode(k.v);
}

// The two kernels below take the coset size l of the multi-point case (further down); l = 1, K = N is the layout above.
// X[r][j] = x^(r)_j = s_{r + (K-2-j) l} (j <= K-2 and inside the SRS), O otherwise; r < l, j < 2K
__global__ __launch_bounds__(256) void k_fk20_load_x(const G1Affine *srs, size_t srs_n, size_t K, size_t l, MsmPoint *X) {
    const size_t two = 2 * K, u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= l * two) return;
    const size_t r = u / two, j = u % two;
    const bool in = j + 2 <= K && r + (K - 2 - j) * l < srs_n;
    X[u] = in ? g1_from_affine30(g1_affine_to30(srs[r + (K - 2 - j) * l]), false) : MsmPoint::infinity();
}

// y[(b l + r) 2K + t] = y^(r)_t of polynomial b, from n coefficients per polynomial (stride n) in sfmt; Montgomery out
__global__ __launch_bounds__(256) void k_fk20_build_y(const Fr *c, size_t n, size_t K, size_t l, size_t batch, int sfmt, Fr *y) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t two = 2 * K, work = batch * l * two;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t a = u / two, t = u % two, b = a / l, r = a % l;
        const bool has = t == 0 || t > K;
        const size_t ci = r + (t == 0 ? K - 1 : t - K - 1) * l;
        Fr v = Fr::zero();
        if (has && ci < n) {
            v = c[b * n + ci];
            if (sfmt == KZG_FR_CANONICAL_LE_32) v = to_mont(v);
        }
        y[u] = v;
    }
}

// yh (natural, Montgomery) -> canonical yh / 2N, bit-reversed
__global__ __launch_bounds__(256) void k_fk20_scale_brev(const Fr *yn, uint32_t log2n, Fr scale, size_t batch, Fr *out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t two = (size_t)1 << log2n, work = batch * two;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t b = u / two, j = u % two;
        out[u] = from_mont(mul(yn[b * two + brev(j, log2n)], scale));
    }
}

// P[b][j] = [yh[b][j]] Xh[j]
__global__ __launch_bounds__(256) void k_fk20_pointwise(MsmPoint *P, const MsmPoint *Xh, const Fr *yh, size_t two, size_t batch,
                                                        MsmPoint *scratch, Fq30 beta) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t work = batch * two;
    for (size_t u = tid; u < work; u += nt) P[u] = mul256(Xh[u % two], yh[u], scratch + tid, nt, beta);
}

// out[b][m] = P[b][brev(m)] in fmt (P == nullptr: the identity)
__global__ __launch_bounds__(64) void k_fk20_emit(const MsmPoint *P, size_t pstride, uint32_t logn, size_t batch, uint8_t *out,
                                                  int fmt, size_t psz) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t N = (size_t)1 << logn, work = batch * N;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t b = u / N, m = u % N;
        emit_one(P ? P[b * pstride + brev(m, logn)] : MsmPoint::infinity(), out + u * psz, fmt);
    }
}

static unsigned grid_for(size_t work, size_t block, size_t max_threads = G1NTT_MAX_THREADS) {
    size_t t = std::min(work, max_threads);
    size_t g = (t + block - 1) / block;
    return (unsigned)(g ? g : 1);
}
static size_t scratch_points(size_t work) { return (size_t)grid_for(work, 256) * 256 * G1NTT_TAB; }

static Fq30 beta30() {
    Fq b;
    for (int i = 0; i < 12; i++) b.v[i] = GLV_BETA[i];
    return to30(to_mont(b));
}

// recoded twiddles base^e (Montgomery base), e < count, into d_out; d_pw: count Fr of scratch
static int glv_table(kzg_ctx *ctx, hipStream_t st, const Fr &base, size_t count, Fr *d_pw, GlvTw *d_out) {
    KZG_TRY(pow_table(ctx, st, base, Fr::one(), count, d_pw));
    KZG_LAUNCH(ctx, st, "k_glv_twiddles", k_glv_twiddles, (unsigned)((count + 255) / 256), 256, 0, d_pw, count, d_out);
    return KZG_OK;
}

// one G1 DFT of size d = 2^logd over `batch` arrays.  forward: DIF (natural -> bit-reversed); else DIT with inverse twiddles
// (bit-reversed -> natural), half_out: only the first half of the last stage.  tw: recoded twiddles of a size-D table, tws = D / d.
// max_threads: the threads of a launch = the slots `scratch` has (kzg_ntt_g1's option; everyone else has scratch_points)
static int g1_dft(kzg_ctx *ctx, hipStream_t st, MsmPoint *P, size_t pstride, uint32_t logd, size_t batch, const GlvTw *tw, size_t tws,
                  bool forward, bool half_out, MsmPoint *scratch, const Fq30 &beta, size_t max_threads = G1NTT_MAX_THREADS) {
    const size_t d = (size_t)1 << logd;
    if (d < 2) return KZG_OK;
    const unsigned g = grid_for(batch * d / 2, 256, max_threads);
    if (forward) {
        for (size_t m = d / 2; m >= 2; m /= 2)
            KZG_LAUNCH(ctx, st, "k_g1ntt_dif", k_g1ntt_dif, g, 256, 0, P, pstride, d, m, tw, tws, batch, scratch, beta);
        KZG_LAUNCH(ctx, st, "k_g1ntt_trivial", k_g1ntt_trivial, g, 256, 0, P, pstride, d, batch, 0);
    } else {
        KZG_LAUNCH(ctx, st, "k_g1ntt_trivial", k_g1ntt_trivial, g, 256, 0, P, pstride, d, batch, (half_out && d == 2) ? 1 : 0);
        for (size_t m = 2; m <= d / 2; m *= 2)
            KZG_LAUNCH(ctx, st, "k_g1ntt_dit", k_g1ntt_dit, g, 256, 0, P, pstride, d, m, tw, tws, batch, scratch, beta,
                       (half_out && m == d / 2) ? 1 : 0);
    }
    return KZG_OK;
}

// ---- multi-point FK20: every coset opening ------------------------------------------------------------------------------
// Coset size l = 2^j, K = N / l cosets, C_i = { w^(i + tK) : t < l }, Z_i = X^l - w^(il) (w^l = w_K).  With the residue split
// c^(r)_t = c_{r + tl}, s^(r)_v = s_{r + vl} (r < l), the witness of coset i is pi_i = DFT_K(h)_i with h = sum_r h^(r) and
// h^(r)_u = sum_{v <= K-2-u} c^(r)_{u+1+v} s^(r)_v: the single-point layout above with N -> K, once per residue, the l products
// summed in the frequency domain before the one inverse transform:
//     x^(r)_j = s_{r + (K-2-j) l} (j <= K-2), O otherwise      (per plan: Xh^(r) = DFT_2K(x^(r)), bit-reversed, l arrays)
//     y^(r) = (c^(r)_{K-1}, 0 x K, c^(r)_0 .. c^(r)_{K-2})       (per polynomial: yh^(r) = DFT_2K(y^(r)) / 2K, bit-reversed)
//     hh_j = sum_r yh^(r)_j Xh^(r)_j,   h = iDFT_2K(hh) first half (DIT),   pi = DFT_K(h) (DIF), read out bit-reversed.
// The interpolant I_i = p mod Z_i has coefficient r = sum_t c^(r)_t w_K^(it) = DFT_K(c^(r))_i: Fr only.  SRS points past len(srs)
// count as the identity, exact whenever n <= l or n - l <= len(srs) (q_i has n - l coefficients).
//
// The combination (2N scalar multiplications per polynomial) is the hot kernel.  The bases are fixed per plan, so the plan keeps
// their multiples 1..8 in affine 30-bit form (G1Affine30, one 128-byte row each), and one thread runs ONE doubling chain per
// frequency over the signed 4-bit digits of all its terms (Straus): 256 doublings for the whole sum plus ~60 mixed additions per
// term.  The per-term route (option "fk20_cosets_combine" = 1) runs mul256 on every term -- 256 doublings, the table build and
// ~60 additions each -- and is kept for comparison.  Both split the residues into S slices whose partial sums k_coset_reduce adds.

constexpr size_t COSET_TARGET_THREADS = (size_t)1 << 17;  // combination threads per chunk the slicing aims for

// tab[e * count + u] = (e + 1) X[u] in affine 30-bit form, e < 8 (the identity: all limbs zero)
__global__ __launch_bounds__(256) void k_coset_table(const MsmPoint *X, size_t count, G1Affine30 *tab) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < count; u += nt) {
        const MsmPoint P = X[u];
        MsmPoint Q = P;
#pragma nounroll
        for (int e = 0; e < G1NTT_TAB; e++) {
            if (e == 1) Q = g1_dbl30(P);
            else if (e > 1) Q = g1_add30(Q, P);  // (e + 1) P != e P: the group has prime order
            tab[(size_t)e * count + u] = g1_affine_to30(g1_to_affine(g1_xyzz_from30(Q)));
        }
    }
}

// z[(b l + r) K + t] = c^(r)_t of polynomial b (Montgomery), the input of the interpolants' NTTs
__global__ __launch_bounds__(256) void k_coset_gather_r(const Fr *c, size_t n, size_t K, size_t l, size_t batch, int sfmt, Fr *z) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t work = batch * l * K;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t a = u / K, t = u % K, b = a / l, r = a % l;
        const size_t ci = r + t * l;
        Fr v = Fr::zero();
        if (ci < n) {
            v = c[b * n + ci];
            if (sfmt == KZG_FR_CANONICAL_LE_32) v = to_mont(v);
        }
        z[u] = v;
    }
}

// out[(b K + i) l + r] = DFT_K(c^(r))_i of polynomial b, in sfmt: coset i's interpolant coefficients r_0 .. r_{l-1}
__global__ __launch_bounds__(256) void k_coset_emit_r(const Fr *z, size_t K, size_t l, size_t batch, int sfmt, Fr *out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t work = batch * K * l;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t r = u % l, i = (u / l) % K, b = u / (l * K);
        const Fr v = z[(b * l + r) * K + i];
        out[u] = sfmt == KZG_FR_CANONICAL_LE_32 ? from_mont(v) : v;
    }
}

// canonical scalars (arrays of `two`) -> k + 0x88..8 (< 2^256: 64 signed digits, no carry out), word q of array a at
// rec[(a 8 + q) two + j] so that a wave's reads of one digit are coalesced
__global__ __launch_bounds__(256) void k_coset_recode(const Fr *k, size_t arrays, size_t two, uint32_t *rec) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t work = arrays * two;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t a = u / two, j = u % two;
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = k[u].v[q];
        recode_add(v, 8);
#pragma unroll
        for (int q = 0; q < 8; q++) rec[(a * 8 + q) * two + j] = v[q];
    }
}

// Straus: P[(b S + s) two + j] = sum over the l / S residues r of slice s of [k_{b,r,j}] T_{r,j}.  tab: the multiples 1..8 of T_{r,j}
// at tab[(e l + r) two + j]; rec: the recoded scalars of the (b, r) arrays (k_coset_recode).  One doubling chain per thread.
__global__ __launch_bounds__(256) void k_coset_straus(const G1Affine30 *tab, size_t l, size_t two, const uint32_t *rec, size_t batch,
                                                      size_t S, MsmPoint *P) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    const size_t work = batch * S * two, rs = l / S;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < work; u += nt) {
        const size_t j = u % two, s = (u / two) % S, b = u / (two * S);
        const uint32_t *rw = rec + (b * l + s * rs) * 8 * two + j;
        const G1Affine30 *tb = tab + s * rs * two + j;
        MsmPoint acc = MsmPoint::infinity();
#pragma nounroll
        for (int nib = 63; nib >= 0; nib--) {
#pragma nounroll
            for (int i = 0; i < 4; i++) acc = g1_dbl30(acc);
            const int q = nib >> 3, sh = 4 * (nib & 7);
#pragma nounroll
            for (size_t rr = 0; rr < rs; rr++) {
                const int d = (int)((rw[(rr * 8 + q) * two] >> sh) & 15u) - 8;
                if (d) acc = g1_madd30(acc, tb[((size_t)((d < 0 ? -d : d) - 1) * l + rr) * two], d < 0);
            }
        }
        P[u] = acc;
    }
}

// per-term route, same contract: mul256 on every term (the multiple 1 of the table is the base itself)
__global__ __launch_bounds__(256) void k_coset_perterm(const G1Affine30 *tab, size_t l, size_t two, const uint32_t *rec, size_t batch,
                                                       size_t S, MsmPoint *P, MsmPoint *scratch, Fq30 beta) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t work = batch * S * two, rs = l / S;
    for (size_t u = tid; u < work; u += nt) {
        const size_t j = u % two, s = (u / two) % S, b = u / (two * S);
        MsmPoint acc = MsmPoint::infinity();
#pragma nounroll
        for (size_t rr = 0; rr < rs; rr++) {
            const size_t r = s * rs + rr;
            Fr k;  // undo the recoding: k = rec - 0x88..8
            uint64_t br = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint64_t d = (uint64_t)rec[((b * l + r) * 8 + q) * two + j] - 0x88888888u - br;
                k.v[q] = (uint32_t)d;
                br = (d >> 32) & 1u;
            }
            acc = g1_add30(acc, mul256(g1_from_affine30(tab[r * two + j], false), k, scratch + tid, nt, beta));
        }
        P[u] = acc;
    }
}

// P[b S two + j] = sum_s P[(b S + s) two + j]
__global__ __launch_bounds__(256) void k_coset_reduce(MsmPoint *P, size_t two, size_t S, size_t batch) {
    const size_t nt = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < batch * two; u += nt) {
        MsmPoint *base = P + (u / two) * S * two + u % two;
        MsmPoint acc = base[0];
        for (size_t s = 1; s < S; s++) acc = g1_add30(acc, base[s * two]);
        base[0] = acc;
    }
}

// residue slices of a combination over `batch` x two frequencies: enough threads to fill the chip, at most l
static size_t coset_slices(size_t l, size_t two, size_t batch) {
    size_t S = 1;
    while (S < l && batch * S * two < COSET_TARGET_THREADS) S *= 2;
    return S;
}

// the combination and its slice reduction; route 0 Straus, 1 per-term (scratch: scratch_points(batch * S * two) points)
static int coset_combine(kzg_ctx *ctx, hipStream_t st, int route, const G1Affine30 *tab, size_t l, size_t two, const uint32_t *rec,
                         size_t batch, size_t S, MsmPoint *P, MsmPoint *scratch, const Fq30 &beta) {
    const unsigned g = grid_for(batch * S * two, 256);
    if (route == 1)
        KZG_LAUNCH(ctx, st, "k_coset_perterm", k_coset_perterm, g, 256, 0, tab, l, two, rec, batch, S, P, scratch, beta);
    else
        KZG_LAUNCH(ctx, st, "k_coset_straus", k_coset_straus, g, 256, 0, tab, l, two, rec, batch, S, P);
    if (S > 1) KZG_LAUNCH(ctx, st, "k_coset_reduce", k_coset_reduce, grid_for(batch * two, 256), 256, 0, P, two, S, batch);
    return KZG_OK;
}

}  // namespace kzg

using namespace kzg;

// ---- plans -------------------------------------------------------------------------------------------------------------------
// One representation for both plan kinds: a single-point plan is the l = 1, K = N case and keeps the DFT output Xh itself
// (k_fk20_pointwise); a coset plan keeps the affine multiples of Xh (k_coset_straus / k_coset_perterm).  `device` stays the first
// field.  The two public types are distinct and opaque (include/kzg_mi355x.h).
struct Fk20Plan {
    int device = 0;
    uint32_t log_n = 0, log_l = 0;
    size_t N = 0, l = 0, K = 0;
    size_t srs_n = 0;               // length of the monomial SRS the plan was built from
    MsmPoint *xhat = nullptr;       // single-point: DFT_2N(x), bit-reversed (2N points)
    G1Affine30 *tab = nullptr;      // cosets: (e + 1) Xh^(r)_j at tab[(e l + r) 2K + j], e < 8: 8 x 2N rows of 128 B
    GlvTw *tw_fwd = nullptr;        // w_2K^e, e < K
    GlvTw *tw_inv = nullptr;        // w_2K^-e, e < K
    Fr inv2k;                       // 1 / 2K, Montgomery
    Fq30 beta;
    ~Fk20Plan() {  // on the plan's device, with nothing of the plan in flight
        if (xhat) hipFree(xhat);
        if (tab) hipFree(tab);
        if (tw_fwd) hipFree(tw_fwd);
        if (tw_inv) hipFree(tw_inv);
    }
};
struct kzg_fk20 : Fk20Plan {};
struct kzg_fk20_cosets : Fk20Plan {};

namespace kzg {

// fills *p for `who` (the entry point, named in its error texts); table: a coset plan (log_l >= 1), else log_l = 0
static int fk20_build(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, uint32_t log_l, bool table, const std::string &who,
                      Fk20Plan *p) {
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (monomial->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, "SRS resident on another GPU");
    if (log_n + 1 >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    if (log_n > FK20_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, who + ": log_n <= 22 (documented limit)");
    if (table && log_l == 0) return fail(ctx, KZG_ERR_SHAPE, who + ": log_l >= 1 (single points: kzg_fk20_setup)");
    if (log_l > log_n) return fail(ctx, KZG_ERR_SHAPE, who + ": coset larger than the domain");
    const std::string what = table ? "FK20 coset plan" : "FK20 plan";
    p->device = ctx->device;
    p->log_n = log_n;
    p->log_l = log_l;
    p->N = (size_t)1 << log_n;
    p->l = (size_t)1 << log_l;
    p->K = p->N >> log_l;
    p->srs_n = monomial->n;
    p->beta = beta30();
    const size_t K = p->K, two = 2 * K, rows = 2 * p->N;  // l arrays of 2K
    const uint32_t logk = log_n - log_l;
    const Fr w = host_omega(logk + 1);  // w_2K, w_2K^2 = w_K = w_N^l (l = 1: compute_omega(N).omega)
    p->inv2k = inv(from_u64<FrParams>((uint64_t)two));
    hipStream_t st = ctx->lanes[0].stream;
    int rc = KZG_OK;
    Fr *pw = nullptr;
    MsmPoint *X = nullptr, *scratch = nullptr;
    const size_t scr = scratch_points(p->l * K);
    if ((table && hipMalloc((void **)&p->tab, G1NTT_TAB * rows * sizeof(G1Affine30)) != hipSuccess) ||
        hipMalloc((void **)&p->tw_fwd, K * sizeof(GlvTw)) != hipSuccess || hipMalloc((void **)&p->tw_inv, K * sizeof(GlvTw)) != hipSuccess ||
        hipMalloc((void **)&pw, K * sizeof(Fr)) != hipSuccess || hipMalloc((void **)&X, rows * sizeof(MsmPoint)) != hipSuccess ||
        hipMalloc((void **)&scratch, scr * sizeof(MsmPoint)) != hipSuccess)
        rc = fail(ctx, KZG_ERR_ALLOC, "hipMalloc(" + what + ")");
    if (rc == KZG_OK) rc = glv_table(ctx, st, w, K, pw, p->tw_fwd);
    if (rc == KZG_OK) rc = glv_table(ctx, st, inv(w), K, pw, p->tw_inv);
    if (rc == KZG_OK) {
        KZG_LAUNCH(ctx, st, "k_fk20_load_x", k_fk20_load_x, (unsigned)((rows + 255) / 256), 256, 0, monomial->table, monomial->n, K, p->l, X);
        rc = g1_dft(ctx, st, X, two, logk + 1, p->l, p->tw_fwd, 1, true, false, scratch, p->beta);
    }
    if (rc == KZG_OK && table)
        KZG_LAUNCH(ctx, st, "k_coset_table", k_coset_table, grid_for(rows, 256), 256, 0, (const MsmPoint *)X, rows, p->tab);
    if (hipStreamSynchronize(st) != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, what + " kernels failed");
    if (hipGetLastError() != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, what + " kernels failed");
    if (!table && rc == KZG_OK) std::swap(p->xhat, X);  // the DFT output is the single-point plan
    if (pw) hipFree(pw);
    if (X) hipFree(X);
    if (scratch) hipFree(scratch);
    if (ctx->prof) prof_collect(ctx);
    return rc;
}

template <class Plan>
static int fk20_setup(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, uint32_t log_l, bool table, const char *who, Plan **out) {
    if (!ctx || !monomial || !out) return KZG_ERR_SHAPE;
    Plan *p = new Plan();
    const int rc = fk20_build(ctx, monomial, log_n, log_l, table, who, p);
    if (rc != KZG_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return KZG_OK;
}

template <class Plan>
static void fk20_free(kzg_ctx *ctx, Plan *plan) {
    if (!plan) return;
    std::optional<Guard> g;
    if (ctx) g.emplace(ctx);
    hipSetDevice(plan->device);
    hipDeviceSynchronize();
    delete plan;
}

// `count` Fr transforms of 2^logd points, transform i at d + i * stride.  Each ntt_run takes its scratch from the arena mark again:
// the transforms are ordered on the lane's stream, so the next one may reuse what the previous one was given
static int ntt_each(kzg_ctx *ctx, int lane, size_t mark, Fr *d, size_t stride, size_t count, uint32_t logd, int inverse) {
    for (size_t i = 0; i < count; i++) {
        ctx->lanes[lane].arena_used = mark;
        KZG_TRY(ntt_run(ctx, lane, d + i * stride, logd, inverse));
    }
    return KZG_OK;
}

// every witness (and, for a coset plan, optionally every interpolant: out_r) of `batch` polynomials of n coefficients (eval: N
// evaluations each), in chunks.  Behind kzg_witness_all_* (l = 1, out_r null) and kzg_witness_cosets_*.
static int fk20_run(kzg_ctx *ctx, const Fk20Plan *p, const void *in, size_t n, size_t batch, int sfmt, int flags, void *out_w, int ofmt,
                    void *out_r, bool eval) {
    if (!ctx || !p) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    const size_t psz = point_format_bytes(ofmt);
    if (!psz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 output format");
    if (p->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, p->tab ? "FK20 coset plan resident on another GPU" : "FK20 plan resident on another GPU");
    const size_t N = p->N, l = p->l, K = p->K, two = 2 * K;
    if (eval && n != N) return fail(ctx, KZG_ERR_SHAPE, "assert!(self.d == evals.d): evaluations must cover the plan's domain");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, "empty polynomial");
    if (n > N) return fail(ctx, KZG_ERR_SHAPE, "polynomial longer than the plan's domain");
    if (n > l && n - l > p->srs_n) return fail(ctx, KZG_ERR_SHAPE, "quotient longer than the SRS (reference: slice index panic)");
    if (batch == 0) return KZG_OK;
    if (batch > SIZE_MAX / (N * 144)) return fail(ctx, KZG_ERR_SHAPE, "batch too large");
    if (!in || !out_w) return KZG_ERR_SHAPE;
    const int lane = 0;
    hipStream_t st = ctx->lanes[lane].stream;
    const bool out_dev = (flags & KZG_OUT_DEVICE) != 0, in_dev = (flags & KZG_IN_DEVICE) != 0, want_r = out_r != nullptr;
    const uint8_t *src = (const uint8_t *)in;
    uint8_t *dst = (uint8_t *)out_w;
    if (N == 1) {  // every quotient is zero: the identity, as kzg_witness_eval / kzg_witness_coeff_many write it (single-point plans only)
        const size_t chunk = std::min(batch, FK20_CHUNK_POINTS);
        KZG_TRY(lane_reserve(ctx, lane, out_dev ? 4096 : chunk * psz + 4096));
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const size_t B = std::min(chunk, batch - b0);
            uint8_t *d_out = out_dev ? dst + b0 * psz : (uint8_t *)ctx->lanes[lane].arena;
            KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)std::min<size_t>((B + 63) / 64, 4096), 64, 0, (const MsmPoint *)nullptr,
                       (size_t)0, 0u, B, d_out, ofmt, psz);
            if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(dst + b0 * psz, d_out, B * psz, hipMemcpyDeviceToHost, st));
        }
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
        KZG_HIP_CHECK(ctx, hipGetLastError());
        return KZG_OK;
    }
    const uint32_t logn = p->log_n, logk = logn - p->log_l;
    const size_t chunk = std::max<size_t>(1, std::min(FK20_MAX_CHUNK, FK20_CHUNK_POINTS / (2 * N)));
    const size_t B0 = std::min(chunk, batch);
    const size_t S = coset_slices(l, two, B0);  // from the first chunk, kept for the ragged last one
    const int route = ctx->opt_fk20_cosets_combine;
    const size_t in_bytes = B0 * n * 32;
    const size_t scr = scratch_points(B0 * S * two);
    size_t need = align_up(B0 * S * two * sizeof(MsmPoint), 256) + 2 * align_up(B0 * 2 * N * 32, 256) + align_up(scr * sizeof(MsmPoint), 256) +
                  (want_r ? align_up(B0 * N * 32, 256) : 0) + (in_dev ? 0 : align_up(in_bytes, 256)) +
                  (out_dev ? 0 : align_up(B0 * K * psz, 256) + (want_r ? align_up(B0 * N * 32, 256) : 0)) +
                  ntt_workspace_bytes(std::max(logk + 1, logn)) + 65536;
    KZG_TRY(lane_reserve(ctx, lane, need));
    MsmPoint *P = (MsmPoint *)lane_alloc(ctx, lane, B0 * S * two * sizeof(MsmPoint));
    Fr *y = (Fr *)lane_alloc(ctx, lane, B0 * 2 * N * 32);
    Fr *yh = (Fr *)lane_alloc(ctx, lane, B0 * 2 * N * 32);
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, lane, scr * sizeof(MsmPoint));
    Fr *z = want_r ? (Fr *)lane_alloc(ctx, lane, B0 * N * 32) : nullptr;
    uint8_t *d_in = in_dev ? nullptr : (uint8_t *)lane_alloc(ctx, lane, in_bytes);
    uint8_t *d_stage = out_dev ? nullptr : (uint8_t *)lane_alloc(ctx, lane, B0 * K * psz);
    uint8_t *d_stage_r = (out_dev || !want_r) ? nullptr : (uint8_t *)lane_alloc(ctx, lane, B0 * N * 32);
    if (!P || !y || !yh || !scratch || (want_r && !z) || (!in_dev && !d_in) || (!out_dev && !d_stage) || (!out_dev && want_r && !d_stage_r))
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const size_t ntt_mark = ctx->lanes[lane].arena_used;  // the scratch of every ntt_each below
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const size_t B = std::min(chunk, batch - b0);
        const uint8_t *d_src = src + b0 * n * 32;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, d_src, B * n * 32, hipMemcpyHostToDevice, st));
            d_src = d_in;
        }
        const Fr *coeffs = (const Fr *)d_src;
        int csfmt = sfmt;
        if (eval) {  // iNTT_N of each evaluation vector (Montgomery) into yh, which the coefficients' only readers precede
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(yh, d_src, B * N * 32, hipMemcpyDeviceToDevice, st));
            if (sfmt == KZG_FR_CANONICAL_LE_32) KZG_TRY(fr_convert(ctx, st, yh, B * N, 1));
            KZG_TRY(ntt_each(ctx, lane, ntt_mark, yh, N, B, logn, 1));
            coeffs = yh;
            csfmt = KZG_FR_MONT_LE_32;
        }
        const unsigned gw = (unsigned)std::min<size_t>((B * 2 * N + 255) / 256, 8192);
        if (want_r) {  // interpolants: DFT_K of every residue class, then transposed into coset-major order
            KZG_LAUNCH(ctx, st, "k_coset_gather_r", k_coset_gather_r, gw, 256, 0, coeffs, n, K, l, B, csfmt, z);
            if (logk) KZG_TRY(ntt_each(ctx, lane, ntt_mark, z, K, B * l, logk, 0));
            Fr *d_r = out_dev ? (Fr *)((uint8_t *)out_r + b0 * N * 32) : (Fr *)d_stage_r;
            KZG_LAUNCH(ctx, st, "k_coset_emit_r", k_coset_emit_r, gw, 256, 0, (const Fr *)z, K, l, B, sfmt, d_r);
            if (!out_dev)
                KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out_r + b0 * N * 32, d_stage_r, B * N * 32, hipMemcpyDeviceToHost, st));
        }
        KZG_LAUNCH(ctx, st, "k_fk20_build_y", k_fk20_build_y, gw, 256, 0, coeffs, n, K, l, B, csfmt, y);
        KZG_TRY(ntt_each(ctx, lane, ntt_mark, y, two, B * l, logk + 1, 0));
        KZG_LAUNCH(ctx, st, "k_fk20_scale_brev", k_fk20_scale_brev, gw, 256, 0, y, logk + 1, p->inv2k, B * l, yh);
        if (p->tab) {  // hh_j = sum_r yh^(r)_j Xh^(r)_j over the plan's table
            KZG_LAUNCH(ctx, st, "k_coset_recode", k_coset_recode, gw, 256, 0, (const Fr *)yh, B * l, two, (uint32_t *)y);
            KZG_TRY(coset_combine(ctx, st, route, p->tab, l, two, (const uint32_t *)y, B, S, P, scratch, p->beta));
        } else {  // Hh_j = yh_j Xh_j
            KZG_LAUNCH(ctx, st, "k_fk20_pointwise", k_fk20_pointwise, grid_for(B * two, 256), 256, 0, P, p->xhat, yh, two, B, scratch, p->beta);
        }
        KZG_TRY(g1_dft(ctx, st, P, S * two, logk + 1, B, p->tw_inv, 1, false, true, scratch, p->beta));  // h = iDFT_2K, first half
        KZG_TRY(g1_dft(ctx, st, P, S * two, logk, B, p->tw_fwd, 2, true, false, scratch, p->beta));      // pi = DFT_K(h), bit-reversed
        uint8_t *d_out = out_dev ? dst + b0 * K * psz : d_stage;
        KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)std::min<size_t>((B * K + 63) / 64, 16384), 64, 0, (const MsmPoint *)P,
                   S * two, logk, B, d_out, ofmt, psz);
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(dst + b0 * K * psz, d_stage, B * K * psz, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

}  // namespace kzg

extern "C" int kzg_fk20_setup(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, kzg_fk20 **out) {
    return fk20_setup(ctx, monomial, log_n, 0, false, "kzg_fk20_setup", out);
}

extern "C" int kzg_fk20_cosets_setup(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, uint32_t log_l, kzg_fk20_cosets **out) {
    return fk20_setup(ctx, monomial, log_n, log_l, true, "kzg_fk20_cosets_setup", out);
}

extern "C" void kzg_fk20_free(kzg_ctx *ctx, kzg_fk20 *plan) { fk20_free(ctx, plan); }

extern "C" void kzg_fk20_cosets_free(kzg_ctx *ctx, kzg_fk20_cosets *plan) { fk20_free(ctx, plan); }

extern "C" size_t kzg_fk20_domain(const kzg_fk20 *plan) { return plan ? plan->N : 0; }

extern "C" int kzg_fk20_cosets_shape(const kzg_fk20_cosets *plan, size_t *domain, size_t *coset_size) {
    if (!plan) return KZG_ERR_SHAPE;
    if (domain) *domain = plan->N;
    if (coset_size) *coset_size = plan->l;
    return KZG_OK;
}

extern "C" int kzg_witness_all_coeff(kzg_ctx *ctx, const kzg_fk20 *plan, const void *coeffs, size_t n, size_t batch, int sfmt,
                                     int flags, void *out, int ofmt) {
    return fk20_run(ctx, plan, coeffs, n, batch, sfmt, flags, out, ofmt, nullptr, false);
}

extern "C" int kzg_witness_all_eval(kzg_ctx *ctx, const kzg_fk20 *plan, const void *evals, size_t d, size_t batch, int sfmt,
                                    int flags, void *out, int ofmt) {
    return fk20_run(ctx, plan, evals, d, batch, sfmt, flags, out, ofmt, nullptr, true);
}

extern "C" int kzg_witness_cosets_coeff(kzg_ctx *ctx, const kzg_fk20_cosets *plan, const void *coeffs, size_t n, size_t batch, int sfmt,
                                        int flags, void *out_w, int ofmt, void *out_r) {
    return fk20_run(ctx, plan, coeffs, n, batch, sfmt, flags, out_w, ofmt, out_r, false);
}

extern "C" int kzg_witness_cosets_eval(kzg_ctx *ctx, const kzg_fk20_cosets *plan, const void *evals, size_t d, size_t batch, int sfmt,
                                       int flags, void *out_w, int ofmt, void *out_r) {
    return fk20_run(ctx, plan, evals, d, batch, sfmt, flags, out_w, ofmt, out_r, true);
}

// ---- compute_lagrange_basis (src/eval_form.rs:254-280), G1 half, from the monomial SRS alone (no secret) ------------------------
// lagrange_basis_g[i] = commit(l_i) with l_i(X) = (1/d) sum_j w^(-ij) X^j: L = (1/d) DFT_d(gs) with the inverse twiddles, i.e.
// g1_dft as a DIF over w^-1 (natural in, bit-reversed out) and the 1/d product in the kernel that reads it out.  The reference
// builds every l_i by d - 1 polynomial multiplications and commits to it (O(d^3) field work); a ceremony SRS has no tau, so the
// eval-form path at 2^20 needs this transform.  Untimed input generation.
namespace kzg {

__global__ __launch_bounds__(256) void k_affine_to_msm_points(const G1Affine *in, MsmPoint *out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = g1_from_affine30(g1_affine_to30(in[i]), false);
}

// out[i] = [dinv] P[brev(i)] in the canonical XYZZ form (dinv: canonical 1 / d; d == 1: L_0 = gs[0], no product)
__global__ __launch_bounds__(256) void k_lagrange_finish(const MsmPoint *P, size_t d, uint32_t bits, Fr dinv, MsmPoint *scratch,
                                                         Fq30 beta, G1Xyzz *out) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid; i < d; i += nt) {
        MsmPoint Q = P[brev(i, bits)];
        if (d > 1) Q = mul256(Q, dinv, scratch + tid, nt, beta);
        out[i] = g1_xyzz_from30(Q);
    }
}

}  // namespace kzg

extern "C" int kzg_srs_lagrange_from_monomial_g1(kzg_ctx *ctx, const kzg_srs *mono, kzg_srs **out) {
    if (!ctx || !mono || !out) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t d = mono->n;
    if (d == 0 || (d & (d - 1))) return fail(ctx, KZG_ERR_SHAPE, "assert!(d & (d - 1) == 0) (src/eval_form.rs:255-256)");
    const uint32_t exp = (uint32_t)ilog2_ceil(d);
    if (exp >= FR_TWO_ADICITY) return fail(ctx, KZG_ERR_DEGREE_TOO_LARGE, "domain too large");
    if (exp > 24) return fail(ctx, KZG_ERR_SHAPE, "compute_lagrange_basis on the GPU is limited to d <= 2^24 (documented limit)");
    hipStream_t st = ctx->lanes[0].stream;
    kzg_srs *s = nullptr;
    KZG_TRY(srs_alloc(ctx, d, &s));
    MsmPoint *P = nullptr, *scratch = nullptr;
    G1Xyzz *rows = nullptr;
    Fr *pw = nullptr;
    GlvTw *tw = nullptr;
    int rc = KZG_OK;
    const size_t half = d > 1 ? d / 2 : 1;
    const size_t scr = scratch_points(d);  // the read-out's d threads; the stages have d / 2 butterflies
    if (hipMalloc((void **)&P, d * sizeof(MsmPoint)) != hipSuccess || hipMalloc((void **)&rows, d * sizeof(G1Xyzz)) != hipSuccess ||
        hipMalloc((void **)&scratch, scr * sizeof(MsmPoint)) != hipSuccess || hipMalloc((void **)&pw, half * sizeof(Fr)) != hipSuccess ||
        hipMalloc((void **)&tw, half * sizeof(GlvTw)) != hipSuccess)
        rc = fail(ctx, KZG_ERR_ALLOC, "hipMalloc(group-FFT workspace)");
    if (rc == KZG_OK) {
        const Fq30 beta = beta30();
        const Fr dinv = from_mont(inv(from_u64<FrParams>((uint64_t)d)));  // canonical
        KZG_LAUNCH(ctx, st, "k_affine_to_msm_points", k_affine_to_msm_points, (unsigned)((d + 255) / 256), 256, 0, mono->table, P, d);
        rc = glv_table(ctx, st, inv(host_omega(exp)), half, pw, tw);
        if (rc == KZG_OK) rc = g1_dft(ctx, st, P, d, exp, 1, tw, 1, true, false, scratch, beta);
        if (rc == KZG_OK) {
            KZG_LAUNCH(ctx, st, "k_lagrange_finish", k_lagrange_finish, grid_for(d, 256), 256, 0, (const MsmPoint *)P, d, exp, dinv, scratch,
                       beta, rows);
            rc = srs_finish_from_xyzz(ctx, s, rows);
        }
    }
    hipStreamSynchronize(st);
    if (hipGetLastError() != hipSuccess && rc == KZG_OK) rc = fail(ctx, KZG_ERR_HIP, "group FFT kernels failed");
    if (P) hipFree(P);
    if (rows) hipFree(rows);
    if (scratch) hipFree(scratch);
    if (pw) hipFree(pw);
    if (tw) hipFree(tw);
    if (rc != KZG_OK) {
        kzg_srs_free(nullptr, s);
        return rc;
    }
    *out = s;
    return KZG_OK;
}

// ---- kzg_ntt_g1: the DFT above as a call of its own ------------------------------------------------------------------------------
// Both directions run g1_dft as a DIF (natural in, bit-reversed out; the inverse over w^-1, as compute_lagrange_basis above), so the
// decoded points are taken as they come and k_fk20_emit reads the result out bit-reversed; the inverse's 1/d is one mul256 per
// point in between.  `batch` arrays in chunks of at most 2^21 points (option "group_ntt_chunk_points").
namespace kzg {

constexpr size_t G1NTT_CHUNK_POINTS = (size_t)1 << 21;

// P[u] = [k] P[u], k canonical
__global__ __launch_bounds__(256) void k_g1ntt_scale(MsmPoint *P, size_t count, Fr k, MsmPoint *scratch, Fq30 beta) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t u = tid; u < count; u += nt) P[u] = mul256(P[u], k, scratch + tid, nt, beta);
}

}  // namespace kzg

extern "C" int kzg_ntt_g1(kzg_ctx *ctx, const void *points, uint32_t log_n, size_t batch, int inverse, int pfmt, int flags, void *out,
                          int ofmt) {
    if (!ctx) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t psz = point_format_bytes(pfmt), osz = point_format_bytes(ofmt);
    if (!psz || !osz) return fail(ctx, KZG_ERR_SHAPE, "unknown G1 point format");
    if (log_n > FK20_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g1: log_n <= 22 (documented limit)");
    if (batch == 0) return KZG_OK;
    if (!points || !out) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g1: NULL buffer");
    const size_t d = (size_t)1 << log_n, half = d > 1 ? d / 2 : 1;
    if (batch > (SIZE_MAX / 224) >> log_n) return fail(ctx, KZG_ERR_SHAPE, "batch too large");
    if (out == points && psz != osz) return fail(ctx, KZG_ERR_SHAPE, "kzg_ntt_g1: in place needs formats of equal size");
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t cpts = ctx->opt_group_ntt_chunk_points ? (size_t)ctx->opt_group_ntt_chunk_points : G1NTT_CHUNK_POINTS;
    const size_t chunk = std::max<size_t>(1, cpts / d), B0 = std::min(chunk, batch), pts0 = B0 * d;
    const size_t cap = ctx->opt_group_ntt_threads ? (size_t)ctx->opt_group_ntt_threads : G1NTT_MAX_THREADS;
    const size_t scr = (size_t)grid_for(pts0, 256, cap) * 256 * G1NTT_TAB;  // the scaling's pts0 threads; the stages have half as many
    KZG_TRY(lane_reserve(ctx, 0, align_up(pts0 * sizeof(MsmPoint), 256) + align_up(pts0 * sizeof(G1Xyzz), 256) + align_up(scr * sizeof(MsmPoint), 256) +
                                     align_up(half * 32, 256) + align_up(half * sizeof(GlvTw), 256) + align_up(pts0 * osz, 256) +
                                     (in_dev ? 0 : align_up(pts0 * psz, 256)) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    MsmPoint *P = (MsmPoint *)lane_alloc(ctx, 0, pts0 * sizeof(MsmPoint));
    G1Xyzz *dec = (G1Xyzz *)lane_alloc(ctx, 0, pts0 * sizeof(G1Xyzz));
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, 0, scr * sizeof(MsmPoint));
    Fr *pw = (Fr *)lane_alloc(ctx, 0, half * 32);
    GlvTw *tw = (GlvTw *)lane_alloc(ctx, 0, half * sizeof(GlvTw));
    uint8_t *enc = (uint8_t *)lane_alloc(ctx, 0, pts0 * osz);  // also with KZG_OUT_DEVICE: `out` may be `points`
    uint8_t *d_raw = in_dev ? nullptr : (uint8_t *)lane_alloc(ctx, 0, pts0 * psz);
    int *bad = (int *)lane_alloc(ctx, 0, 256);
    if (!P || !dec || !scratch || !pw || !tw || !enc || (!in_dev && !d_raw) || !bad) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const Fq30 beta = beta30();
    const Fr w = host_omega(log_n);
    const Fr dinv = from_mont(inv(from_u64<FrParams>((uint64_t)d)));  // canonical
    const uint8_t *src = (const uint8_t *)points;
    uint8_t *dst = (uint8_t *)out;
    const char *bad_msg = "a G1 point failed to decode, is not on the curve or not in the r-torsion subgroup";
    KZG_HIP_CHECK(ctx, hipMemsetAsync(bad, 0, sizeof(int), st));
    if (log_n >= 2) KZG_TRY(glv_table(ctx, st, inverse ? inv(w) : w, half, pw, tw));
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
            KZG_TRY(decode_points(ctx, st, raw, n, pfmt, dec, bad, level));
            if (pass == 0) continue;
            if (!two_pass) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
                KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
                if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, bad_msg);
            }
            KZG_TRY(points_to30(ctx, st, dec, P, n));
            KZG_TRY(g1_dft(ctx, st, P, d, log_n, B, tw, 1, true, false, scratch, beta, cap));
            if (inverse && d > 1) KZG_LAUNCH(ctx, st, "k_g1ntt_scale", k_g1ntt_scale, grid_for(n, 256, cap), 256, 0, P, n, dinv, scratch, beta);
            KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)std::min<size_t>((n + 63) / 64, 16384), 64, 0, (const MsmPoint *)P, d,
                       log_n, B, enc, ofmt, osz);
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(dst + b0 * d * osz, enc, n * osz, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        }
        if (pass == 0) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
            KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
            if (hbad) return fail(ctx, KZG_ERR_BAD_POINT, bad_msg);
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
__global__ __launch_bounds__(256) void k_test_g1_mul_glv(const G1Affine *p, const Fr *k, size_t n, MsmPoint *scratch, Fq30 beta,
                                                         G1Affine *o) {
    const size_t nt = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = tid; i < n; i += nt) {
        const MsmPoint P = g1_from_affine30(g1_affine_to30(p[i]), false);
        const GlvTw w = glv_recode(k[i].v);
        emit_one(glv_mul(P, w, scratch + tid, nt, beta), (uint8_t *)(o + i), KZG_G1_AFFINE_MONT_96);
    }
}

// affine in, natural order (inverse: loaded bit-reversed for the DIT)
__global__ __launch_bounds__(256) void k_test_g1ntt_load(const G1Affine *in, size_t d, uint32_t bits, int rev, MsmPoint *P) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d) return;
    P[i] = g1_from_affine30(g1_affine_to30(in[rev ? brev(i, bits) : i]), false);
}
}  // namespace kzg

extern "C" int kzg_test_g1_mul_glv(kzg_ctx *ctx, const void *p, const void *k_canonical, size_t n, void *out) {
    if (!ctx || !p || !k_canonical || !out || !n) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t scr = scratch_points(n);
    KZG_TRY(lane_reserve(ctx, 0, n * (96 + 32 + 96) + scr * sizeof(MsmPoint) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *dp = lane_alloc(ctx, 0, n * 96), *dk = lane_alloc(ctx, 0, n * 32), *dout = lane_alloc(ctx, 0, n * 96);
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, 0, scr * sizeof(MsmPoint));
    if (!dp || !dk || !dout || !scratch) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dp, p, n * 96, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dk, k_canonical, n * 32, hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_test_g1_mul_glv", k_test_g1_mul_glv, grid_for(n, 256), 256, 0, (const G1Affine *)dp, (const Fr *)dk, n,
               scratch, beta30(), (G1Affine *)dout);
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, n * 96, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    return KZG_OK;
}

// out_m = sum_j w^(+-jm) P_j over the size-2^log_n domain (the inverse is NOT scaled by 1 / d)
extern "C" int kzg_test_g1_ntt(kzg_ctx *ctx, const void *pts, uint32_t log_n, int inverse, void *out) {
    if (!ctx || !pts || !out || log_n > FK20_MAX_LOG) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t d = (size_t)1 << log_n, half = d > 1 ? d / 2 : 1;
    const size_t scr = scratch_points(half);
    KZG_TRY(lane_reserve(ctx, 0, d * (96 + 96 + sizeof(MsmPoint)) + half * (32 + sizeof(GlvTw)) + scr * sizeof(MsmPoint) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *din = lane_alloc(ctx, 0, d * 96), *dout = lane_alloc(ctx, 0, d * 96);
    MsmPoint *P = (MsmPoint *)lane_alloc(ctx, 0, d * sizeof(MsmPoint));
    Fr *pw = (Fr *)lane_alloc(ctx, 0, half * 32);
    GlvTw *tw = (GlvTw *)lane_alloc(ctx, 0, half * sizeof(GlvTw));
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, 0, scr * sizeof(MsmPoint));
    if (!din || !dout || !P || !pw || !tw || !scratch) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(din, pts, d * 96, hipMemcpyHostToDevice, st));
    const Fr w = host_omega(log_n);
    KZG_TRY(glv_table(ctx, st, inverse ? inv(w) : w, half, pw, tw));
    KZG_LAUNCH(ctx, st, "k_test_g1ntt_load", k_test_g1ntt_load, (unsigned)((d + 255) / 256), 256, 0, (const G1Affine *)din, d, log_n,
               inverse ? 1 : 0, P);
    KZG_TRY(g1_dft(ctx, st, P, d, log_n, 1, tw, 1, !inverse, false, scratch, beta30()));
    if (inverse) {  // natural order out: d "polynomials" of one point each
        KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)((d + 63) / 64), 64, 0, (const MsmPoint *)P, (size_t)1, 0u, d,
                   (uint8_t *)dout, (int)KZG_G1_AFFINE_MONT_96, (size_t)96);
    } else {
        KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)((d + 63) / 64), 64, 0, (const MsmPoint *)P, d, log_n, (size_t)1,
                   (uint8_t *)dout, (int)KZG_G1_AFFINE_MONT_96, (size_t)96);
    }
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, d * 96, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    return KZG_OK;
}

// out_j = sum_r k_{r,j} B_{r,j}: the coset combination alone (tables, recoding, route, slices, reduction) on caller-given points
extern "C" int kzg_test_fk20_cosets_combine(kzg_ctx *ctx, const void *bases, const void *k_canonical, size_t l, size_t m, int route,
                                            size_t slices, void *out) {
    if (!ctx || !bases || !k_canonical || !out || !l || !m || (l & (l - 1)) || (route != 0 && route != 1)) return KZG_ERR_SHAPE;
    if (slices && (slices > l || (slices & (slices - 1)))) return KZG_ERR_SHAPE;
    if (l * m > ((size_t)1 << 22)) return KZG_ERR_SHAPE;
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t cnt = l * m, S = slices ? slices : coset_slices(l, m, 1);
    const size_t scr = scratch_points(S * m);
    KZG_TRY(lane_reserve(ctx, 0, cnt * (96 + 32 + 32 + sizeof(MsmPoint) + G1NTT_TAB * sizeof(G1Affine30)) + S * m * sizeof(MsmPoint) +
                                     m * 96 + scr * sizeof(MsmPoint) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *db = lane_alloc(ctx, 0, cnt * 96), *dout = lane_alloc(ctx, 0, m * 96);
    Fr *dk = (Fr *)lane_alloc(ctx, 0, cnt * 32);
    uint32_t *rec = (uint32_t *)lane_alloc(ctx, 0, cnt * 32);
    MsmPoint *X = (MsmPoint *)lane_alloc(ctx, 0, cnt * sizeof(MsmPoint));
    G1Affine30 *tab = (G1Affine30 *)lane_alloc(ctx, 0, G1NTT_TAB * cnt * sizeof(G1Affine30));
    MsmPoint *P = (MsmPoint *)lane_alloc(ctx, 0, S * m * sizeof(MsmPoint));
    MsmPoint *scratch = (MsmPoint *)lane_alloc(ctx, 0, scr * sizeof(MsmPoint));
    if (!db || !dout || !dk || !rec || !X || !tab || !P || !scratch) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(db, bases, cnt * 96, hipMemcpyHostToDevice, st));
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(dk, k_canonical, cnt * 32, hipMemcpyHostToDevice, st));
    KZG_LAUNCH(ctx, st, "k_test_g1ntt_load", k_test_g1ntt_load, (unsigned)((cnt + 255) / 256), 256, 0, (const G1Affine *)db, cnt, 0u, 0,
               X);
    KZG_LAUNCH(ctx, st, "k_coset_table", k_coset_table, grid_for(cnt, 256), 256, 0, (const MsmPoint *)X, cnt, tab);
    KZG_LAUNCH(ctx, st, "k_coset_recode", k_coset_recode, grid_for(cnt, 256), 256, 0, (const Fr *)dk, l, m, rec);
    KZG_TRY(coset_combine(ctx, st, route, tab, l, m, rec, 1, S, P, scratch, beta30()));
    KZG_LAUNCH(ctx, st, "k_fk20_emit", k_fk20_emit, (unsigned)((m + 63) / 64), 64, 0, (const MsmPoint *)P, (size_t)1, 0u, m,
               (uint8_t *)dout, (int)KZG_G1_AFFINE_MONT_96, (size_t)96);
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, m * 96, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    return KZG_OK;
}
#endif  // KZG_TEST_HOOKS
