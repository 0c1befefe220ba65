// glv.h -- [k]P by the GLV endomorphism of BLS12-381 G1 and signed 4-bit digits, on the signed 30-bit XYZZ form (curve30.h): the
// scalar multiplications of the FK20 butterflies and point-wise products (g1ntt.hip).  Host and device: the CPU suite compiles it
// with g++ (tests/host_glv.cpp) and checks it against the oracle without a GPU.
//
// lambda = z^2 - 1 with r = lambda^2 + lambda + 1, phi(x, y) = (beta x, y) = [lambda](x, y); k = k2 lambda + k1 with k1, k2 < 2^128 by
// plain division.  A value v is recoded as v + 0x88..8 read by nibbles minus 8: digits in [-8, 7] plus a carry out, so the table
// holds P..8P only (sign and phi applied on the fly: one Fq product per phi digit).  Table entry e sits at tab[e * st] (a scratch
// slot strided by the thread count on the GPU: coalesced).
#pragma once
#include "curve30.h"

namespace kzg {

// lambda = 0xac45a4010001a40200000000ffffffff (little-endian u32 limb i)
KZG_HD constexpr uint32_t glv_lambda(int i) { return i == 0 ? 0xffffffffu : i == 1 ? 0u : i == 2 ? 0x0001a402u : i == 3 ? 0xac45a401u : 0u; }
// beta (canonical), a primitive cube root of unity in Fq with phi(P) = [lambda]P
constexpr uint32_t GLV_BETA[12] = {0x0000aaacu, 0x8bfd0000u, 0x4f49fffdu, 0x409427ebu, 0x0fb85f9bu, 0x897d2965u,
                                   0x89759ad4u, 0xaa0d857du, 0x63d4de85u, 0xec024086u, 0x397fe699u, 0x1a0111eau};
constexpr int G1NTT_TAB = 8;  // P, 2P, .., 8P

// a twiddle k = k2 lambda + k1, recoded: a = k1 + 0x88..8, b = k2 + 0x88..8 (mod 2^128); top bit 0 / 1 = the carries out
struct alignas(16) GlvTw {
    uint32_t a[4], b[4];
    uint32_t top, pad[3];
};

KZG_HD uint32_t limb_sel(const uint32_t *v, int n, int q) {  // v[q] without a dynamically indexed array
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < n) r = (i == q) ? v[i] : r;
    return r;
}

// k (canonical, 8 limbs) = k2 lambda + k1, k1 < lambda, k2 <= lambda + 1 (< 2^128): restoring division, one bit per step (every
// array index static: no scratch memory)
KZG_HD void glv_split(const uint32_t k[8], uint32_t k1[4], uint32_t k2[4]) {
    uint32_t rem[5] = {0, 0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
#pragma nounroll
    for (int bit = 255; bit >= 0; bit--) {
#pragma unroll
        for (int i = 4; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 31);
        rem[0] = (rem[0] << 1) | ((limb_sel(k, 8, bit >> 5) >> (bit & 31)) & 1u);
        // rem >= lambda: borrow-free subtraction
        uint32_t t[5];
        uint64_t br = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            uint64_t d = (uint64_t)rem[i] - glv_lambda(i) - br;
            t[i] = (uint32_t)d;
            br = (d >> 32) & 1u;
        }
        const bool ge = br == 0;
#pragma unroll
        for (int i = 0; i < 5; i++) rem[i] = ge ? t[i] : rem[i];
        // quotient bits arrive most significant first; only the low 128 can be set
#pragma unroll
        for (int i = 3; i > 0; i--) q[i] = (q[i] << 1) | (q[i - 1] >> 31);
        q[0] = (q[0] << 1) | (ge ? 1u : 0u);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        k1[i] = rem[i];
        k2[i] = q[i];
    }
}

// v + 0x88..8 over n limbs; returns the carry out
KZG_HD uint32_t recode_add(uint32_t *v, int n) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < n; i++) {
        uint64_t t = (uint64_t)v[i] + 0x88888888u + c;
        v[i] = (uint32_t)t;
        c = t >> 32;
    }
    return (uint32_t)c;
}

KZG_HD GlvTw glv_recode(const uint32_t k[8]) {
    GlvTw w;
    glv_split(k, w.a, w.b);
    uint32_t ta = recode_add(w.a, 4), tb = recode_add(w.b, 4);
    w.top = ta | (tb << 1);
    w.pad[0] = w.pad[1] = w.pad[2] = 0;
    return w;
}

// tab[e * st] = (e + 1) P, e < 8
KZG_HD void build_tab8(const G1Xyzz30 &P, G1Xyzz30 *tab, size_t st) {
    tab[0] = P;
    G1Xyzz30 p2 = g1_dbl30(P);
    tab[st] = p2;
    G1Xyzz30 p3 = g1_add30(p2, P);
    tab[2 * st] = p3;
    G1Xyzz30 p4 = g1_dbl30(p2);
    tab[3 * st] = p4;
    tab[4 * st] = g1_add30(p4, P);
    G1Xyzz30 p6 = g1_dbl30(p3);
    tab[5 * st] = p6;
    tab[6 * st] = g1_add30(p6, P);
    tab[7 * st] = g1_dbl30(p4);
}

// acc + [nib - 8] T (T = P, or phi(P) with `phi`), T's multiples in the table
KZG_HD G1Xyzz30 add_digit(const G1Xyzz30 &acc, const G1Xyzz30 *tab, size_t st, uint32_t nib, bool phi,
                                              const Fq30 &beta) {
    const int d = (int)nib - 8;
    if (d == 0) return acc;
    G1Xyzz30 T = tab[(size_t)((d < 0 ? -d : d) - 1) * st];
    if (d < 0) T.y = neg30(T.y);
    if (phi) T.x = mul30(T.x, beta);
    return g1_add30(acc, T);
}

// [k1 + k2 lambda] P from a recoded twiddle
KZG_HD G1Xyzz30 glv_mul(const G1Xyzz30 &P, const GlvTw &w, G1Xyzz30 *tab, size_t st, const Fq30 &beta) {
    build_tab8(P, tab, st);
    G1Xyzz30 acc = (w.top & 1u) ? P : G1Xyzz30::infinity();
    if (w.top & 2u) {
        G1Xyzz30 T = P;
        T.x = mul30(T.x, beta);
        acc = g1_add30(acc, T);
    }
#pragma nounroll
    for (int nib = 31; nib >= 0; nib--) {
#pragma nounroll
        for (int j = 0; j < 4; j++) acc = g1_dbl30(acc);
        const int q = nib >> 3, sh = 4 * (nib & 7);
        acc = add_digit(acc, tab, st, (limb_sel(w.a, 4, q) >> sh) & 15u, false, beta);
        acc = add_digit(acc, tab, st, (limb_sel(w.b, 4, q) >> sh) & 15u, true, beta);
    }
    return acc;
}

// [k] P for a canonical k < r: k + 0x88..8 < 2^256, 64 signed digits, no carry out
KZG_HD G1Xyzz30 mul256(const G1Xyzz30 &P, const Fr &k, G1Xyzz30 *tab, size_t st, const Fq30 &beta) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = k.v[i];
    recode_add(v, 8);
    build_tab8(P, tab, st);
    G1Xyzz30 acc = G1Xyzz30::infinity();
#pragma nounroll
    for (int nib = 63; nib >= 0; nib--) {
#pragma nounroll
        for (int j = 0; j < 4; j++) acc = g1_dbl30(acc);
        acc = add_digit(acc, tab, st, (limb_sel(v, 8, nib >> 3) >> (4 * (nib & 7))) & 15u, false, beta);
    }
    return acc;
}

}  // namespace kzg
