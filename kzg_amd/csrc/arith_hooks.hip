// arith_hooks.hip -- kzg_test_arith (include/kzg_mi355x_test.h): the device twin of the arithmetic shims of tests/host_math.cpp.
// Linked into libkzg_mi355x_hooks.so only, and built through the same device-assembly post-processing as msm.hip / ntt.hip
// (kzg_amd/build.py: strip_asm_nops), so the tests check the generated inline asm in the form the hot kernels run it.
//
// Each d_* function below has the body of the host shim of the same name (hm_*), line for line: the same functions in the same
// order.  On the host they resolve to the portable C (mul30_inline, mulshoup29_inline, ...); here to mul_gfx950.inc,
// mul30_gfx950.inc and mul29r_gfx950.inc.  One thread per record; a record is the shim's arguments back to back.
#include "common.h"
#include "emit.h"
#include "fr29.h"
#include "../../include/kzg_mi355x_test.h"

namespace kzg {
namespace {

__device__ void d_fq_mul(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fq x, y; memcpy(x.v, a, 48); memcpy(y.v, b, 48); Fq z = mul(x, y); memcpy(o, z.v, 48); }
__device__ void d_fq_add(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fq x, y; memcpy(x.v, a, 48); memcpy(y.v, b, 48); Fq z = add(x, y); memcpy(o, z.v, 48); }
__device__ void d_fq_sub(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fq x, y; memcpy(x.v, a, 48); memcpy(y.v, b, 48); Fq z = sub(x, y); memcpy(o, z.v, 48); }
__device__ void d_fr_mul(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fr x, y; memcpy(x.v, a, 32); memcpy(y.v, b, 32); Fr z = mul(x, y); memcpy(o, z.v, 32); }
__device__ void d_fr_add(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fr x, y; memcpy(x.v, a, 32); memcpy(y.v, b, 32); Fr z = add(x, y); memcpy(o, z.v, 32); }
__device__ void d_fr_sub(const uint32_t *a, const uint32_t *b, uint32_t *o) { Fr x, y; memcpy(x.v, a, 32); memcpy(y.v, b, 32); Fr z = sub(x, y); memcpy(o, z.v, 32); }

__device__ void d_mul30_raw(const int32_t *a, const int32_t *b, int32_t *o) { Fq30 x, y; memcpy(x.v, a, 52); memcpy(y.v, b, 52);
    Fq30 z = mul30(x, y); memcpy(o, z.v, 52); }
__device__ void d_sqr30_raw(const int32_t *a, int32_t *o) { Fq30 x; memcpy(x.v, a, 52); Fq30 z = sqr30(x); memcpy(o, z.v, 52); }
// the host shim calls muladd30_inline explicitly (the portable function); the device twin calls what the kernels call
__device__ void d_muladd30_raw(const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int32_t *o) {
    Fq30 x, y, u, w; memcpy(x.v, a, 52); memcpy(y.v, b, 52); memcpy(u.v, c, 52); memcpy(w.v, d, 52);
    Fq30 z = muladd30(x, y, u, w); memcpy(o, z.v, 52); }
__device__ void d_mul30_sub_raw(const int32_t *a, const int32_t *b, const int32_t *c, int32_t *o) { Fq30 x, y, u; memcpy(x.v, a, 52); memcpy(y.v, b, 52);
    memcpy(u.v, c, 52); Fq30 z = mul30_sub(x, y, u); memcpy(o, z.v, 52); }
__device__ void d_sqr30_sub2_raw(const int32_t *a, const int32_t *c, const int32_t *e, int32_t *o) { Fq30 x, u, w; memcpy(x.v, a, 52); memcpy(u.v, c, 52);
    memcpy(w.v, e, 52); Fq30 z = sqr30_sub2(x, u, w); memcpy(o, z.v, 52); }
__device__ void d_mul30u_raw(const int32_t *a, const int32_t *b, int32_t *o) { Fq30 x, y; memcpy(x.v, a, 52); memcpy(y.v, b, 52);
    Fq30 z = mul30u(x, y); memcpy(o, z.v, 52); }
__device__ void d_sqr30_sub2u_raw(const int32_t *a, const int32_t *c, const int32_t *e, int32_t *o) { Fq30 x, u, w; memcpy(x.v, a, 52); memcpy(u.v, c, 52);
    memcpy(w.v, e, 52); Fq30 z = sqr30_sub2u(x, u, w); memcpy(o, z.v, 52); }
__device__ void d_normalize30_raw(const int32_t *a, int32_t *o) { Fq30 x; memcpy(x.v, a, 52); Fq30 z = normalize30(x); memcpy(o, z.v, 52); }
__device__ void d_from30_raw(const int32_t *a, uint32_t *o) { Fq30 x; memcpy(x.v, a, 52); Fq z = from30(x); memcpy(o, z.v, 48); }

__device__ void d_madd30_chain_kernel_form(const uint32_t *pts, int n, uint64_t signs, uint32_t *o) {
    const G1Affine *p = (const G1Affine *)pts;
    G1Affine30 first = g1_affine_to30(p[0]);
    G1Xyzz30 acc = g1_from_affine30(first, signs & 1);
    for (int i = 1; i < n; i++) {
        const G1Affine30 cur = g1_affine_to30(p[i]);
        const bool neg = (signs >> i) & 1;
        if (cur.is_inf()) continue;
        if (acc.inf) { acc = g1_from_affine30(cur, neg); continue; }
        Madd30Mid mid = g1_madd30_phase1(acc, cur, neg);
        acc = g1_madd30_phase2(acc, mid, neg, [&]() { return cur; });
    }
    G1Affine r = g1_to_affine(g1_xyzz_from30(g1_normalize30(acc))); memcpy(o, &r, 96); }
__device__ void d_add30(const uint32_t *a, const uint32_t *b, uint32_t *o) { G1Affine x, y; memcpy(&x, a, 96); memcpy(&y, b, 96);
    G1Affine30 x30 = g1_affine_to30(x), y30 = g1_affine_to30(y);
    G1Xyzz30 p = g1_madd30(g1_dbl30(g1_from_affine30(x30, false)), x30, true);
    G1Xyzz30 q = g1_madd30(g1_madd30(g1_from_affine30(y30, false), y30, false), y30, true);
    G1Affine r = g1_to_affine(g1_xyzz_from30(g1_add30(p, q))); memcpy(o, &r, 96); }
__device__ void d_mul30_scalar(const uint32_t *a, const uint32_t *k, uint32_t *o) { G1Affine x; memcpy(&x, a, 96);
    G1Xyzz30 base = g1_from_affine30(g1_affine_to30(x), false), acc = G1Xyzz30::infinity();
    for (int i = 255; i >= 0; i--) { acc = g1_dbl30(acc); if ((k[i >> 5] >> (i & 31)) & 1) acc = g1_add30(acc, base); }
    G1Affine r = g1_to_affine(g1_xyzz_from30(acc)); memcpy(o, &r, 96); }

__device__ void d_fr29_mul(const uint32_t *x, const uint32_t *w_mont, uint32_t *o) { Fr a, w; memcpy(a.v, x, 32); memcpy(w.v, w_mont, 32);
    Fr z = fr29_pack_canonical(mul29r(fr29_unpack(a), fr29_twiddle_from_mont(w))); memcpy(o, z.v, 32); }
__device__ void d_fr29_butterflies(const uint32_t *u, const uint32_t *v, const uint32_t *w_mont, int stages, uint32_t *ou, uint32_t *ov) {
    Fr a, b, w; memcpy(a.v, u, 32); memcpy(b.v, v, 32); memcpy(w.v, w_mont, 32);
    Fr29 U = fr29_unpack(a), V = fr29_unpack(b), W = fr29_twiddle_from_mont(w);
    for (int s = 0; s < stages; s++) { Fr29 t = mul29r(V, W); fr29_butterfly(U, V, t); }
    Fr zu = fr29_pack_canonical(mul29r(U, fr29_one())), zv = fr29_pack_canonical(mul29r(V, fr29_one()));
    memcpy(ou, zu.v, 32); memcpy(ov, zv.v, 32); }
__device__ void d_fr29_shoup_raw(const uint32_t *x_limbs, const uint32_t *w_mont, uint32_t *out_limbs, uint32_t *w_out, uint32_t *wp_out) {
    Fr w; memcpy(w.v, w_mont, 32);
    Fr29 x, W, WP; memcpy(x.v, x_limbs, 36);
    fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w), W, WP);
    Fr29 r = mulshoup29(x, W, WP);
    memcpy(out_limbs, r.v, 36); memcpy(w_out, W.v, 36); memcpy(wp_out, WP.v, 36); }
// as the host shim, except that t1 and t3 (the two products that share a twiddle) are ONE mulshoup29x2, as in lds_ntt_stages29
__device__ void d_fr29_radix4_chain(const uint32_t *x0, const uint32_t *xs, const uint32_t *w_mont, int pairs, int which, uint32_t *o) {
    Fr a; memcpy(a.v, x0, 32);
    Fr29 X0 = fr29_unpack(a);
    for (int p = 0; p < pairs; p++) {
        Fr b1, b2, b3, w1, w2, w3;
        memcpy(b1.v, xs + 24 * p, 32); memcpy(b2.v, xs + 24 * p + 8, 32); memcpy(b3.v, xs + 24 * p + 16, 32);
        memcpy(w1.v, w_mont + 24 * p, 32); memcpy(w2.v, w_mont + 24 * p + 8, 32); memcpy(w3.v, w_mont + 24 * p + 16, 32);
        Fr29 A, AP, B, BP, Cw, CP;
        fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w1), A, AP);
        fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w2), B, BP);
        fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w3), Cw, CP);
        Fr29 x1 = fr29_unpack(b1), x2 = fr29_unpack(b2), x3 = fr29_unpack(b3);
        Fr29 t1 = x1, t3 = x3;
        mulshoup29x2(t1, A, AP, t3, A, AP);
        Fr29 s0, y1, s2, y3;
        fr29_butterfly_lazy(X0, t1, s0, y1);
        fr29_butterfly_lazy(x2, t3, s2, y3);
        Fr29 t2 = mulshoup29(s2, B, BP), t3b = mulshoup29(y3, Cw, CP);
        Fr29 z0, z2, z1, z3;
        fr29_butterfly_lazy(s0, t2, z0, z2);
        fr29_butterfly_lazy(y1, t3b, z1, z3);
        X0 = fr29_normalize(which == 0 ? z0 : which == 1 ? z1 : which == 2 ? z2 : z3);
    }
    Fr z = fr29_pack_canonical(fr29_reduce_below_2r(X0)); memcpy(o, z.v, 32); }
__device__ void d_fr29_quotient_thread(const uint32_t *a, const uint32_t *x_mont, const uint32_t *p_mont, const uint32_t *nb, int m, const uint32_t *a_next,
                                       uint32_t *o_scan, uint32_t *o_next, uint32_t *top_limb) {
    Fr xm, pm; memcpy(xm.v, x_mont, 32); memcpy(pm.v, p_mont, 32);
    Fr29 X, XP, P, PP;
    fr29_shoup_from_twiddle(fr29_twiddle_from_mont(xm), X, XP);
    fr29_shoup_from_twiddle(fr29_twiddle_from_mont(pm), P, PP);
    Fr c[8]; memcpy(c, a, 256);
    Fr29 v = fr29_unpack(c[7]);
    for (int k = 6; k >= 0; k--) v = fr29_add_lazy(mulshoup29(v, X, XP), fr29_unpack(c[k]));
    v = fr29_normalize(v);
    for (int i = 0; i < m; i++) {
        Fr29 o; memcpy(o.v, nb + 9 * i, 36);
        v = fr29_normalize(fr29_add_lazy(v, mulshoup29(o, P, PP)));
    }
    *top_limb = v.v[8];
    Fr out = fr29_canonical(v); memcpy(o_scan, out.v, 32);
    Fr an; memcpy(an.v, a_next, 32);
    Fr nx = add(an, fr29_pack_canonical(mulshoup29(fr29_unpack(out), X, XP))); memcpy(o_next, nx.v, 32); }
// device only: two independent Shoup products with different operands through one interleaved mulshoup29x2
__device__ void d_mulshoup29x2(const uint32_t *x_limbs, const uint32_t *w_mont, const uint32_t *y_limbs, const uint32_t *w2_mont,
                               uint32_t *out_x, uint32_t *out_y) {
    Fr w, w2; memcpy(w.v, w_mont, 32); memcpy(w2.v, w2_mont, 32);
    Fr29 x, y, W, WP, W2, WP2; memcpy(x.v, x_limbs, 36); memcpy(y.v, y_limbs, 36);
    fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w), W, WP);
    fr29_shoup_from_twiddle(fr29_twiddle_from_mont(w2), W2, WP2);
    mulshoup29x2(x, W, WP, y, W2, WP2);
    memcpy(out_x, x.v, 36); memcpy(out_y, y.v, 36); }
__device__ void d_emit(const uint32_t *a, const uint32_t *k, int fmt, uint8_t *o) { G1Affine x; memcpy(&x, a, 96);
    G1Xyzz p = g1_scalar_mul(x, k);
    G1Xyzz30 q = g1_xyzz_to30(p);
    alignas(16) uint8_t buf[144];
    for (int i = 0; i < 144; i++) buf[i] = 0;
    emit_one(q, buf, fmt);
    memcpy(o, buf, 144); }

struct OpShape {
    uint32_t in_rec, out_rec;
};
// indexed by the KZG_ARITH_* op (include/kzg_mi355x_test.h)
constexpr OpShape kShapes[KZG_ARITH_NUM_OPS] = {
    {96, 48}, {96, 48}, {96, 48}, {64, 32}, {64, 32}, {64, 32},                        // saturated
    {104, 52}, {52, 52}, {208, 52}, {156, 52}, {104, 52}, {156, 52}, {156, 52}, {52, 52}, {52, 48},   // 30-bit
    {1552, 96}, {192, 96}, {128, 96},                                                  // 30-bit curve
    {64, 32}, {100, 64}, {68, 108}, {1192, 32}, {716, 68}, {136, 72}, {132, 144}};     // 29-bit, emit

template <int OP>
__global__ __launch_bounds__(256) void k_test_arith(const uint8_t *in, size_t n, uint8_t *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr size_t IN = kShapes[OP].in_rec, OUT = kShapes[OP].out_rec;
    const uint32_t *w = (const uint32_t *)(in + i * IN);   // records are multiples of 4 B (of 16 B where points are cast) on a 256-B base
    uint32_t *o = (uint32_t *)(out + i * OUT);
    const int32_t *s = (const int32_t *)w;
    int32_t *so = (int32_t *)o;
    if constexpr (OP == KZG_ARITH_FQ_MUL) d_fq_mul(w, w + 12, o);
    else if constexpr (OP == KZG_ARITH_FQ_ADD) d_fq_add(w, w + 12, o);
    else if constexpr (OP == KZG_ARITH_FQ_SUB) d_fq_sub(w, w + 12, o);
    else if constexpr (OP == KZG_ARITH_FR_MUL) d_fr_mul(w, w + 8, o);
    else if constexpr (OP == KZG_ARITH_FR_ADD) d_fr_add(w, w + 8, o);
    else if constexpr (OP == KZG_ARITH_FR_SUB) d_fr_sub(w, w + 8, o);
    else if constexpr (OP == KZG_ARITH_MUL30) d_mul30_raw(s, s + 13, so);
    else if constexpr (OP == KZG_ARITH_SQR30) d_sqr30_raw(s, so);
    else if constexpr (OP == KZG_ARITH_MULADD30) d_muladd30_raw(s, s + 13, s + 26, s + 39, so);
    else if constexpr (OP == KZG_ARITH_MUL30_SUB) d_mul30_sub_raw(s, s + 13, s + 26, so);
    else if constexpr (OP == KZG_ARITH_MUL30U) d_mul30u_raw(s, s + 13, so);
    else if constexpr (OP == KZG_ARITH_SQR30_SUB2) d_sqr30_sub2_raw(s, s + 13, s + 26, so);
    else if constexpr (OP == KZG_ARITH_SQR30_SUB2U) d_sqr30_sub2u_raw(s, s + 13, s + 26, so);
    else if constexpr (OP == KZG_ARITH_NORMALIZE30) d_normalize30_raw(s, so);
    else if constexpr (OP == KZG_ARITH_FROM30) d_from30_raw(s, o);
    else if constexpr (OP == KZG_ARITH_MADD30_CHAIN) {
        const int cnt = (int)w[0];     // 1..16 (the wrapper has checked every record)
        d_madd30_chain_kernel_form(w + 4, cnt, (uint64_t)w[2] | ((uint64_t)w[3] << 32), o);
    } else if constexpr (OP == KZG_ARITH_ADD30) d_add30(w, w + 24, o);
    else if constexpr (OP == KZG_ARITH_MUL30_SCALAR) d_mul30_scalar(w, w + 24, o);
    else if constexpr (OP == KZG_ARITH_FR29_MUL) d_fr29_mul(w, w + 8, o);
    else if constexpr (OP == KZG_ARITH_FR29_BUTTERFLIES) d_fr29_butterflies(w, w + 8, w + 16, s[24], o, o + 8);
    else if constexpr (OP == KZG_ARITH_FR29_SHOUP_RAW) d_fr29_shoup_raw(w, w + 9, o, o + 9, o + 18);
    else if constexpr (OP == KZG_ARITH_FR29_RADIX4_CHAIN) d_fr29_radix4_chain(w, w + 8, w + 152, s[296], s[297], o);
    else if constexpr (OP == KZG_ARITH_FR29_QUOTIENT_THREAD) d_fr29_quotient_thread(w, w + 64, w + 72, w + 80, s[170], w + 171, o, o + 8, o + 16);
    else if constexpr (OP == KZG_ARITH_MULSHOUP29X2) d_mulshoup29x2(w, w + 9, w + 17, w + 26, o, o + 9);
    else if constexpr (OP == KZG_ARITH_EMIT) d_emit(w, w + 24, s[32], (uint8_t *)o);
}

// the kernel of a run-time op: k_test_arith<op>
template <int OP>
int launch_arith(kzg_ctx *ctx, hipStream_t st, int op, const uint8_t *din, size_t n, uint8_t *dout) {
    if (op == OP) {
        KZG_LAUNCH(ctx, st, "k_test_arith", k_test_arith<OP>, (unsigned)((n + 255) / 256), 256, 0, din, n, dout);
        return KZG_OK;
    }
    if constexpr (OP + 1 < KZG_ARITH_NUM_OPS) return launch_arith<OP + 1>(ctx, st, op, din, n, dout);
    return fail(ctx, KZG_ERR_SHAPE, "kzg_test_arith: unknown op");
}

// the loop counts the kernels take from the records: outside their range a thread would read past its record
bool record_ok(int op, const uint8_t *rec) {
    int32_t v[2];
    switch (op) {
    case KZG_ARITH_MADD30_CHAIN: memcpy(v, rec, 4); return v[0] >= 1 && v[0] <= 16;
    case KZG_ARITH_FR29_BUTTERFLIES: memcpy(v, rec + 96, 4); return v[0] >= 0 && v[0] <= 12;
    case KZG_ARITH_FR29_RADIX4_CHAIN: memcpy(v, rec + 1184, 8); return v[0] >= 0 && v[0] <= 6 && v[1] >= 0 && v[1] <= 3;
    case KZG_ARITH_FR29_QUOTIENT_THREAD: memcpy(v, rec + 680, 4); return v[0] >= 0 && v[0] <= 10;
    case KZG_ARITH_EMIT:
        memcpy(v, rec + 128, 4);
        return v[0] == KZG_G1_AFFINE_MONT_96 || v[0] == KZG_G1_JACOBIAN_MONT_144 || v[0] == KZG_G1_ZCASH_UNCOMPRESSED_96 ||
               v[0] == KZG_G1_ZCASH_COMPRESSED_48;
    default: return true;
    }
}

}  // namespace
}  // namespace kzg

using namespace kzg;

extern "C" int kzg_test_arith(kzg_ctx *ctx, int op, const void *in, size_t in_rec, size_t n, void *out, size_t out_rec) {
    if (!ctx || !in || !out || !n || n > ((size_t)1 << 24)) return KZG_ERR_SHAPE;
    if (op < 0 || op >= KZG_ARITH_NUM_OPS) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_arith: unknown op");
    if (in_rec != kShapes[op].in_rec || out_rec != kShapes[op].out_rec) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_arith: record size");
    for (size_t i = 0; i < n; i++)
        if (!record_ok(op, (const uint8_t *)in + i * in_rec)) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_arith: record out of contract");
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KZG_TRY(lane_reserve(ctx, 0, n * (in_rec + out_rec) + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *din = lane_alloc(ctx, 0, n * in_rec), *dout = lane_alloc(ctx, 0, n * out_rec);
    if (!din || !dout) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(din, in, n * in_rec, hipMemcpyHostToDevice, st));
    KZG_TRY(launch_arith<0>(ctx, st, op, (const uint8_t *)din, n, (uint8_t *)dout));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, n * out_rec, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}
