/*
 * kzg_mi355x_test.h -- unit-test hooks: device arithmetic exercised directly.  NOT part of the product ABI: they exist only in
 * the -DKZG_TEST_HOOKS build of the library (kzg_amd/libkzg_mi355x_hooks.so, built by `python -m kzg_amd.build` next to the
 * product library and loaded by tests/ only).
 *
 * The hooks build also honours two environment variables (read when the library first needs RCCL):
 *   KZG_TEST_NO_RCCL=1        RCCL is "not installed": the load-failure path on a host that has it
 *   KZG_TEST_SHM_TRANSPORT=1  the eight RCCL entry points are replaced by a shared-memory stand-in (kzg_amd/csrc/test_transport.h)
 *                             and kzg_mctx_create accepts the same device several times: device groups of world size > 1 on a
 *                             one-GPU box (RCCL refuses two ranks per GPU).  tests/test_gpu_mgpu_world.py, tools/bench_shared_gpu.sh.
 */
#ifndef KZG_MI355X_TEST_H
#define KZG_MI355X_TEST_H
#include "kzg_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif
int kzg_test_fr_mul(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out);   /* Montgomery */
int kzg_test_fq_mul(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out);   /* Montgomery, 48 B */
int kzg_test_fr_inv(kzg_ctx *ctx, const void *a, size_t n, void *out);
int kzg_test_g1_add(kzg_ctx *ctx, const void *a, const void *b, size_t n, void *out);   /* affine mont 96 */
int kzg_test_g1_mul(kzg_ctx *ctx, const void *p, const void *k_canonical, size_t n, void *out);
/* [k]P through the GLV split of the FK20 butterflies (g1ntt.hip): k = k2 lambda + k1, signed 4-bit digits over P and phi(P) */
int kzg_test_g1_mul_glv(kzg_ctx *ctx, const void *p, const void *k_canonical, size_t n, void *out);
/* one G1 DFT of 2^log_n points over compute_omega(2^log_n): out_m = sum_j w^(jm) P_j, or w^(-jm) with `inverse` (NOT scaled by
 * 1 / 2^log_n); affine Montgomery in and out, natural order */
int kzg_test_g1_ntt(kzg_ctx *ctx, const void *pts, uint32_t log_n, int inverse, void *out);
/* the coset combination of kzg_witness_cosets_* alone: out_j = sum_{r < l} k_{r,j} B_{r,j}, j < m.  bases: l x m affine Montgomery
 * (B_{r,j} at r m + j), k_canonical: l x m scalars < r likewise, out: m affine Montgomery.  route 0 = Straus, 1 = mul256 per term;
 * slices: the residue slices (a power of two <= l), 0 = the rule of the calls.  l a power of two, l x m <= 2^22 */
int kzg_test_fk20_cosets_combine(kzg_ctx *ctx, const void *bases, const void *k_canonical, size_t l, size_t m, int route,
                                 size_t slices, void *out);
/* kzg_test_arith: the device twin of the arithmetic shims of tests/host_math.cpp (kzg_amd/csrc/arith_hooks.hip).  One thread per
 * record runs the same functions in the same order as the host shim, so on gfx950 it exercises the generated inline-asm branch
 * (mul_gfx950.inc, mul30_gfx950.inc, mul29r_gfx950.inc) where the host build runs the portable C.  Record `i` of the input is the
 * shim's arguments laid out back to back (in_rec bytes), record `i` of the output its output buffers (out_rec bytes).  An unknown
 * op, n == 0, or an in_rec / out_rec that is not the op's returns KZG_ERR_SHAPE.  Fq: 12 x u32, Fr: 8 x u32, Fq30: 13 x i32,
 * Fr29: 9 x u32, G1: affine Montgomery 96 B, all little-endian.  The contract of each op is the one its portable version is
 * proven for (tests/test_host_math.py); outside it the result is unspecified.
 *
 *  op                          in_rec  out_rec  record (in -> out)                  contract
 *  FQ_MUL / FQ_ADD / FQ_SUB     96      48      a, b -> a*b/R, a+b, a-b mod q       a, b < q
 *  FR_MUL / FR_ADD / FR_SUB     64      32      a, b -> same mod r                  a, b < r
 *  MUL30, MUL30U                104     52      a, b -> a*b/2^390 (balanced / unsigned digits)
 *                                                                                   limbs 0..11 in [-2^29, 2^29] or one operand's in
 *                                                                                   [0, 2^30); limb 12 below 2^27 (|value| < 80 q)
 *  SQR30                        52      52      a -> a^2/2^390                      limbs 0..11 in [-2^29, 2^29); limb 12 below 2^27
 *  MULADD30                     208     52      a, b, c, d -> (ab + cd)/2^390       as MUL30
 *  MUL30_SUB                    156     52      a, b, c -> ab/2^390 - c             as MUL30; c likewise
 *  SQR30_SUB2, SQR30_SUB2U      156     52      a, c, e -> a^2/2^390 - c - 2e       a as SQR30; c, e as MUL30's operands
 *  NORMALIZE30                  52      52      a -> the balanced digits of a       limbs 0..11 below 3 * 2^29; limb 12 below 2^20
 *  FROM30                       52      48      a -> a/2^390 * R mod q, canonical   normalised, |a| < 256 q
 *  MADD30_CHAIN                 1552    96      u32 n, u32 0, u64 signs, 16 G1 ->   1 <= n <= 16; the points on the curve; the chain of
 *                                               sum +-P_i (hm_madd30_chain_kernel_form, k_accum_affine's lazy accumulator)
 *  ADD30                        192     96      P, Q -> P + Q via dbl30/madd30/add30  points on the curve
 *  MUL30_SCALAR                 128     96      P, k (8 x u32) -> [k]P (dbl30/add30) P on the curve
 *  FR29_MUL                     64      32      x, w*2^256 mod r -> x*w mod r       x < 2^256, w < r
 *  FR29_BUTTERFLIES             100     64      u, v, w_mont, i32 stages -> u', v'  u, v, w < r; 0 <= stages <= 12
 *  FR29_SHOUP_RAW               68      108     x (9 limbs), w_mont -> x*w (9 limbs), w, wp
 *                                                                                   x < 2^261, limbs below 1.5 * 2^30; w < r
 *  FR29_RADIX4_CHAIN            1192    32      x0, 18 x Fr, 18 x Fr w_mont, i32 pairs, i32 which -> chain value
 *                                                                                   0 <= pairs <= 6, 0 <= which <= 3, w < r
 *  FR29_QUOTIENT_THREAD         716     68      a[8], x_mont, p_mont, nb[10] (9 limbs), i32 m, a_next -> o_scan, o_next, u32 top
 *                                                                                   0 <= m <= 10, nb below 25 r normalised, a_next < r
 *  MULSHOUP29X2                 136     72      (x, w_mont) twice -> both products via ONE interleaved mulshoup29x2 (no host twin:
 *                                                                                   each half equals FR29_SHOUP_RAW's product); as FR29_SHOUP_RAW
 *  EMIT                         132     144     P, k (8 x u32), i32 fmt -> emit_one of [k]P in `fmt` (bytes beyond the format's
 *                                                                                   size are zero); P on the curve, fmt a KZG_G1_* format
 */
enum {
    KZG_ARITH_FQ_MUL = 0, KZG_ARITH_FQ_ADD = 1, KZG_ARITH_FQ_SUB = 2, KZG_ARITH_FR_MUL = 3, KZG_ARITH_FR_ADD = 4, KZG_ARITH_FR_SUB = 5,
    KZG_ARITH_MUL30 = 6, KZG_ARITH_SQR30 = 7, KZG_ARITH_MULADD30 = 8, KZG_ARITH_MUL30_SUB = 9, KZG_ARITH_MUL30U = 10,
    KZG_ARITH_SQR30_SUB2 = 11, KZG_ARITH_SQR30_SUB2U = 12, KZG_ARITH_NORMALIZE30 = 13, KZG_ARITH_FROM30 = 14,
    KZG_ARITH_MADD30_CHAIN = 15, KZG_ARITH_ADD30 = 16, KZG_ARITH_MUL30_SCALAR = 17,
    KZG_ARITH_FR29_MUL = 18, KZG_ARITH_FR29_BUTTERFLIES = 19, KZG_ARITH_FR29_SHOUP_RAW = 20, KZG_ARITH_FR29_RADIX4_CHAIN = 21,
    KZG_ARITH_FR29_QUOTIENT_THREAD = 22, KZG_ARITH_MULSHOUP29X2 = 23, KZG_ARITH_EMIT = 24,
    KZG_ARITH_NUM_OPS = 25
};
/* kzg_test_tower: the device twin of ht_tower_op of tests/host_tower.cpp (kzg_amd/csrc/tower_hooks.hip; both compile the record bodies
 * of kzg_amd/csrc/tower_hooks.h).  One thread per record, 64 per block, runs the functions of kzg_amd/csrc/tower.h as the verifier
 * kernels of pairing.hip do: out of line, operands in scratch memory.  Same shape as kzg_test_arith; n <= 4096.  An unknown op, n == 0,
 * a record size that is not the op's, or a record whose alias / power / np / mask word is out of range returns KZG_ERR_SHAPE before
 * anything is launched.  Encoding: canonical little-endian, Fq 48 B, Fq2 96 B (c0, c1), Fq12 576 B (the coefficients of w^0..w^5),
 * G1 affine 96 B, G2 affine 192 B, all zero = the identity; the kernel converts to and from Montgomery form.
 * `alias` (i32) selects how the call r = op(a, b) is made, on the objects themselves and without a copy:
 *   0 r distinct, 1 r is a, 2 r is b, 3 a is b (r distinct; the record's b is unused), 4 r, a, b one object; unary ops take 0 or 1.
 *
 *  op                          in_rec  out_rec  record (in -> out)
 *  F2_MUL                       196     96      a, b, alias -> a b
 *  F2_SQR / F2_INV / F2_MUL_XI  100     96      a, alias -> a^2, 1/a (a != 0), a (1 + u)
 *  F2_MUL_FQ                    148     96      a, k (Fq), alias -> a k
 *  F12_MUL                      1156    576     a, b, alias -> a b
 *  F12_SQR / F12_CYCLOTOMIC_SQR / F12_INV / F12_CONJ / F12_EXP_Z
 *                               580     576     a, alias -> a^2, a^2 (a cyclotomic), 1/a, a^(q^6), a^z (a cyclotomic, z < 0)
 *  F12_FROB                     584     576     a, i32 power (1 or 2), alias -> a^(q^power)
 *  F12_IS_ONE                   576     4       a -> u32 (a == 1)
 *  F12_MUL_LINE                 864     576     f, lam, cst, P (G1) -> f (cst - lam xP w^2 + yP w^3)
 *  G2_ADD                       388     192     P, Q, alias -> P + Q (g2_add on Jacobian operands, Z = 1)
 *  G2_DOUBLE                    196     192     P, alias -> 2 P (g2_dbl)
 *  G2_MUL                       224     192     P, k (8 x u32) -> [k]P
 *  G2_ON_CURVE                  192     4       P -> u32
 *  G2_PRECOMPUTE_LINES          192     13056   Q -> the 68 (lam, cst) pairs of g2_precompute_lines (all zero for the identity)
 *  MILLER_LOOP                  1160    576     u32 np (1..4), u32 mask (< 2^np), 4 x G1, 4 x G2 -> prod f_{z,Q_i}(P_i); pair i uses
 *                                               stored lines (computed in the same thread from Q_i) when bit i of mask is set, else
 *                                               lines on the fly; mask 0 passes no table at all, as k_pairing_check does
 *  FINAL_EXPONENTIATION         576     576     f -> f^(3 (q^12 - 1)/r)
 *  PAIRING_PRODUCT_IS_ONE       1160    4       as MILLER_LOOP -> u32 (prod e(P_i, Q_i) == 1)
 */
enum {
    KZG_TOWER_F2_MUL = 0, KZG_TOWER_F2_SQR = 1, KZG_TOWER_F2_INV = 2, KZG_TOWER_F2_MUL_FQ = 3, KZG_TOWER_F2_MUL_XI = 4,
    KZG_TOWER_F12_MUL = 5, KZG_TOWER_F12_SQR = 6, KZG_TOWER_F12_CYCLOTOMIC_SQR = 7, KZG_TOWER_F12_INV = 8, KZG_TOWER_F12_FROB = 9,
    KZG_TOWER_F12_CONJ = 10, KZG_TOWER_F12_IS_ONE = 11, KZG_TOWER_F12_EXP_Z = 12, KZG_TOWER_F12_MUL_LINE = 13,
    KZG_TOWER_G2_ADD = 14, KZG_TOWER_G2_DOUBLE = 15, KZG_TOWER_G2_MUL = 16, KZG_TOWER_G2_ON_CURVE = 17,
    KZG_TOWER_G2_PRECOMPUTE_LINES = 18, KZG_TOWER_MILLER_LOOP = 19, KZG_TOWER_FINAL_EXPONENTIATION = 20,
    KZG_TOWER_PAIRING_PRODUCT_IS_ONE = 21,
    KZG_TOWER_NUM_OPS = 22
};
int kzg_test_tower(kzg_ctx *ctx, int op, const void *in, size_t in_rec, size_t n, void *out, size_t out_rec);
/* the first two stages of kzg_verify_cosets alone (kzg_amd/csrc/verify_cosets.hip).  stage 0, interpolation: in = count x l cell values
 * (sfmt) of the cosets coset_ids -> out = count x l interpolant coefficients (sfmt).  stage 1, fixed-base sum: in = count x l scalars
 * (sfmt; coset_ids unused) -> out = count points sum_j in[k l + j] gs[j], affine Montgomery */
int kzg_test_verify_cosets_stage(kzg_ctx *ctx, const kzg_cosets_verifier *plan, int stage, const size_t *coset_ids, const void *in,
                                 size_t count, int sfmt, void *out);
/* the variable-base multi-scalar sum of kzg_verify_cosets_batch alone (kzg_amd/csrc/verify_cosets_batch.hip) over row 0 of a resident
 * SRS: out = sum_{i < n} scalars[i] srs[offset + i], affine Montgomery 96 B -- what kzg_msm_g1 gives for the same arguments */
int kzg_test_vb_msm(kzg_ctx *ctx, const struct kzg_srs *srs, size_t offset, const void *scalars, size_t n, int sfmt, void *out_affine_mont_96);
/* kzg_verify_cosets_batch with its intermediate results: out_a = the l scalars a_j, out_cw = the n_commitments scalars c_m (both
 * canonical), out_points = P1, P2, Cagg, Ragg (4 x affine Montgomery 96 B).  count > 0 */
int kzg_test_verify_cosets_batch_parts(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                                       const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs,
                                       size_t count, const void *r, int sfmt, int pfmt, int flags, int *ok, void *out_a, void *out_cw,
                                       void *out_points);
/* kzg_verify_eval_batch with its intermediate results: out_yagg = the scalar sum_k rho_k y_k, out_cw = the n_commitments scalars c_m
 * (both canonical), out_points = the four points the finish consumes (4 x affine Montgomery 96 B): P1, P2, the total of the third
 * bucket set = Cagg - [yagg] gs[0], and the Ragg slot, which this call leaves the identity.  count > 0 */
int kzg_test_verify_eval_batch_parts(kzg_ctx *ctx, const struct kzg_srs *gs, const struct kzg_srs_g2 *hs, const void *xs, const void *ys,
                                     int sfmt, const void *commitments, size_t n_commitments, const uint32_t *commitment_idx,
                                     const void *witnesses, int pfmt, size_t count, const void *r, int *ok, void *out_yagg, void *out_cw,
                                     void *out_points);
int kzg_test_arith(kzg_ctx *ctx, int op, const void *in, size_t in_rec, size_t n, void *out, size_t out_rec);
/* g2_madd of kzg_amd/csrc/tower.h alone (the mixed addition kzg_msm_g2_bucket accumulates with; kzg_amd/csrc/g2_msm.hip), one thread per
 * record, 64 per block: out[i] = acc[i] + pts[i].  acc: Jacobian Montgomery 288 B (any Z; Z = 0 the identity), pts and out: affine
 * Montgomery 192 B (all zero the identity).  1 <= n <= 4096 */
int kzg_test_g2_madd(kzg_ctx *ctx, const void *acc_jacobian, const void *pts_affine, size_t n, void *out_affine);
/* the twiddle multiplier of the G2 DFT alone (kzg_amd/csrc/g2ntt.hip): out[i] = [k_i] P_i.  pts_affine and out_affine: affine
 * Montgomery 192 B (all zero the identity), P_i in the r-torsion; k_canonical: n scalars below r.  route 0 = the psi split and the joint
 * chain, 1 = signed 4-bit digits over the whole scalar.  1 <= n <= 65536 */
int kzg_test_g2_mul_gls(kzg_ctx *ctx, const void *pts_affine, const void *k_canonical, size_t n, int route, void *out_affine);
/* the recoding of that multiplier for one canonical scalar k < r, on the calling thread (no GPU work): words[i] = k_i of
 * k = k_0 + k_1 u + k_2 u^2 + k_3 u^3 (u = 0xd201000000010000), digits[17 i + j] = the signed 4-bit digit j of k_i in [-8, 7], least
 * significant first, digits[17 i + 16] = the carry (0 or 1) */
int kzg_test_g2_gls_recode(const void *k_canonical, uint64_t *words, int8_t *digits);
/* pretend `srs` is resident on GPU `device` (the "SRS of another GPU" error of every MSM entry point, on a one-GPU box) */
int kzg_test_srs_set_device(struct kzg_srs *srs, int device);
/* the same for the G2 points and for a kzg_cosets_verifier (kzg_amd/csrc/verify_cosets.hip) */
int kzg_test_srs_g2_set_device(struct kzg_srs_g2 *srs, int device);
int kzg_test_cosets_verifier_set_device(kzg_cosets_verifier *plan, int device);
/* the next sharded call of this group fails locally on local GPU 0 with `code` (status agreement across ranks, mgpu.hip) */
int kzg_test_mctx_inject_failure(struct kzg_mctx *m, int code);
/* the next growth of the group's exchange buffers fails on local GPU 0 (a rank-local allocation failure BEFORE the exchange: the
 * ranks agree on it through the status-only all-gather instead of leaving the others inside the data all-gather) */
int kzg_test_mctx_inject_alloc_failure(struct kzg_mctx *m);
/* the next exchange sits behind a spin kernel of `ms` milliseconds on local GPU 0 (a peer that arrives late or never: option
 * "gather_timeout_ms" turns it into KZG_ERR_INTERNAL and a dead group) */
int kzg_test_mctx_inject_stall(struct kzg_mctx *m, int ms);
#ifdef __cplusplus
}
#endif
#endif
