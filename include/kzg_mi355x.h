/*
 * kzg_mi355x.h -- C ABI of the MI355X-native (gfx950) KZG commit/open engine.
 *
 * This is the drop-in boundary for the hot path of proxima-one/kzg (crate kzg 0.8.0-beta.1).  The
 * reference has no FFI of its own (it is pure Rust calling blstrs); the entry points below are the
 * ones a `kzg-mi355x-sys` binding would splice in at the reference's call sites, cited per function
 * as (reference file:line).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ exceptions or callbacks cross the ABI.
 *   - every call returns a kzg_status; 0 = ok, >0 = the reference's own error conditions,
 *     <0 = runtime failure (HIP).  kzg_last_error(ctx) gives a human-readable string.
 *   - a kzg_ctx is bound to one GPU and is thread-safe.  The reference's blocking calls -- kzg_commit_coeff,
 *     kzg_commit_eval, kzg_msm_g1, kzg_witness_coeff, kzg_witness_coeff_batched, kzg_witness_eval, kzg_verify_poly_coeff /
 *     _eval, kzg_ntt_fr, kzg_coset_ntt_fr, kzg_poly_mul, kzg_poly_divide, kzg_poly_eval, kzg_poly_multi_eval, kzg_interpolate, kzg_quotient_linear / _eval,
 *     kzg_point_tree_product, kzg_point_tree_eval, kzg_point_tree_combine, kzg_point_tree_interpolate, kzg_fr_vec_mul / _sub, kzg_divide_by_z_on_coset, kzg_fr_scan, kzg_fr_grand_product, kzg_fr_batch_inverse,
 *     kzg_lookup_setup, kzg_lookup_count, kzg_logup_terms, kzg_fr_program_run,
 *     kzg_mle_eq, kzg_mle_bind, kzg_mle_eval, kzg_sumcheck_round (KZGProver / KZGProverEvalForm / KZGVerifier are Clone + &self, src/coeff_form.rs:37-124; an
 *     EvaluationDomain is the caller's own) -- run CONCURRENTLY on one ctx: each call leases one of the context's lanes
 *     (option "streams", default and maximum 16), submits its kernels there and waits for its own result only, so N host
 *     threads calling commit() / create_witness_batched() against one resident SRS fill the GPU like kzg_msm_g1_batch does.
 *     Every other call (the *_batch / *_many forms, SRS construction, the pairing verifier, options, profiling) takes the
 *     context exclusively (it waits for the leased lanes to drain).  kzg_dev_alloc / _upload / _download take no lock at all and
 *     are NOT ordered against calls in flight on other threads: a download sees the results of every call that has RETURNED;
 *     reading a buffer another thread's call is still writing is the caller's race.  A kzg_srs / kzg_srs_g2 is immutable after creation
 *     and may be used from any number of threads and from every kzg_ctx on the same device.  kzg_last_error returns the
 *     calling thread's own last failure.  There is NO CPU fallback: without a usable HIP device kzg_ctx_create fails
 *     with KZG_ERR_NO_DEVICE.
 *   - points entering through kzg_srs_upload_g1/g2, the verifier entry points and kzg_pairing_check are validated the way
 *     blstrs' G1Affine / G2Affine deserialisation validates them upstream, in EVERY format: coordinates < q, on the curve,
 *     in the r-torsion subgroup ([r]P == O); failure -> KZG_ERR_BAD_POINT.  Option "trusted_points" = 1 skips the subgroup
 *     test (never the on-curve test).  kzg_g1_sum[_batch] checks coordinates and the curve equation only.
 *   - scalars in KZG_FR_CANONICAL_LE_32 that are >= r are taken mod r (single host scalars such as x, y, tau must be < r:
 *     KZG_ERR_SHAPE).
 *   - `flags` says where buffers live: scalars/points in host memory (default) or already resident
 *     in this GPU's HBM (KZG_IN_DEVICE), result written to host (default) or device (KZG_OUT_DEVICE).
 *
 * Data formats (all little-endian unless "ZCASH")
 *   KZG_FR_MONT_LE_32        4 x u64 limbs of a*2^256 mod r      (= blst_fr = blstrs::Scalar in memory)
 *   KZG_FR_CANONICAL_LE_32   32 bytes of a < r                    (= Scalar::to_bytes_le)
 *   KZG_G1_AFFINE_MONT_96    x,y: 6 x u64 Montgomery limbs each; identity = all zero (= blst_p1_affine)
 *   KZG_G1_JACOBIAN_MONT_144 X,Y,Z Montgomery limbs; identity has Z = 0 (= blst_p1 = G1Projective)
 *   KZG_G1_ZCASH_UNCOMPRESSED_96 / KZG_G1_ZCASH_COMPRESSED_48   big-endian canonical with flag bits
 *                            (bit7 compressed, bit6 infinity, bit5 y-sign) = G1Affine::to_uncompressed
 *                            / to_compressed
 *   KZG_G2_AFFINE_MONT_192   x.c0,x.c1,y.c0,y.c1 Montgomery limbs; identity all zero (= blst_p2_affine)
 *   KZG_G2_JACOBIAN_MONT_288 X,Y,Z in Fq2; identity has Z = 0 (= blst_p2 = G2Projective)
 *   KZG_G2_ZCASH_UNCOMPRESSED_192 / KZG_G2_ZCASH_COMPRESSED_96  x.c1 || x.c0 [|| y.c1 || y.c0] big-endian
 *                            with the same flag bits (= G2Affine::to_uncompressed / to_compressed)
 *
 * Decoding (what "validated" above means format by format; ONE byte string per group element, so a caller may hash the bytes it
 * hands in -- the challenge r of kzg_verify_cosets_batch / kzg_verify_eval_batch).  Anything else is KZG_ERR_BAD_POINT:
 *   ZCASH compressed     bit 7 set.  Bit 6 set: bit 5 clear and EVERY other bit of the encoding zero -> the identity.  Otherwise x
 *                        (G2: c1 || c0) is the remaining 381 bits, every component < q; x^3 + b must be a square; y is the
 *                        lexicographically larger root exactly when bit 5 is set (G1: y > (q-1)/2; G2: (c1, c0) against the
 *                        negation's, c0 deciding when c1 = 0).
 *   ZCASH uncompressed   bit 7 clear.  Bit 6 set: every other bit, bit 5 included, zero -> the identity.  Otherwise bit 5 clear,
 *                        every coordinate < q, (x, y) on the curve.  All-zero bytes are (0, 0), which is not.
 *   affine Montgomery    every limb vector < q; all-zero is the identity; anything else, (0, y) and (x, 0) included, must satisfy
 *                        the curve equation.
 *   Jacobian Montgomery  X, Y, Z < q (also when Z = 0); Z = 0 is the identity; otherwise Y^2 = X^3 + b Z^6.
 *   then [r]P == O unless option "trusted_points" = 1.  The encoders write exactly these forms, so re-encoding a decoded wire
 *   point gives back its bytes (oracle/decode.py is the reference decoder; tests/test_gpu_decode.py).
 */
#ifndef KZG_MI355X_H
#define KZG_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (each returns KZG_ERR_SHAPE with a message in kzg_last_error; tests/test_gpu_validation.py):
 *   kzg_ntt_fr                              log_n <= 28                      (2^24: two LDS passes of <= 2^12 points; above: one
 *                                                                             more four-step level of <= 16 around them)
 *   kzg_coset_ntt_fr                        log_n <= 28;  kzg_poly_mul: products of up to 2^27 coefficients;
 *   kzg_ntt_fr_batch,
 *   kzg_coset_ntt_fr_batch                  log_n <= 28; any batch and stride: vectors go in chunks of max(1, 2^21 / n) (option "ntt_batch_chunk");
 *                                                                             the workspace is one chunk's scratch (chunk x n x 32 B: 64 MiB, or one
 *                                                                             vector; none at all up to 2^12 points) and does not grow with batch; host
 *                                                                             data is staged in pieces of max(1, 2^21 / n) vectors (<= 64 MiB, or one vector)
 *   kzg_witness_coeff_batched               polynomials of up to 2^26 coefficients (the SRS with its window tables is 118 GB there);
 *   kzg_verify_poly_eval                    as far as the monomial SRS goes (MSM limit below)
 *   kzg_witness_coeff_batched,
 *   kzg_verify_eval_batched                 k <= 16384 opening points         (the interpolation works on a k x k matrix: 8.6 GB there)
 *   kzg_poly_multi_eval                     n <= 2^28; any k and batch: points go in passes of at most 4096, polynomials in chunks that
 *                                                                             fill the grid; the workspace is at most 17 MiB of partial sums
 *                                                                             beside one chunk's staged coefficients (host input: <= 256 MiB)
 *   kzg_interpolate                         k <= 16384 points                (the k x k basis matrix: 8.6 GB there); any batch
 *   kzg_poly_divide                         na <= 2^27 (the product limit of kzg_poly_mul); any nb and batch: dividends go in chunks of
 *                                                                             min(256, max(1, 2^20 / na)); the workspace does not grow with batch
 *   kzg_fr_scan, kzg_fr_grand_product,
 *   kzg_fr_batch_inverse                    n <= 2^28; any t and batch: vectors go in chunks of min(65535, max(1, 65536 / ceil(n / 2048))), three
 *                                                                             launches each; the workspace is 64 B (scan) / 128 B (grand product) per
 *                                                                             tile of a chunk (<= 16 MiB at the default tile) beside one staged piece of
 *                                                                             host data (<= 64 MiB, or one vector -- with its 2 t columns) and does not
 *                                                                             grow with batch; the inversion: <= 64 MiB of scratch when in == out
 *   kzg_lookup_setup                        1 <= n_t <= 2^26 table rows      (the plan holds 32 B per key plus the slot array, 8 B x next_pow2(n_t) x 2
 *                                                                             by default -- option "lookup_spare_log" --: 48 to 64 B per row, 4.3 GB at 2^26)
 *   kzg_lookup_count                        n <= 2^28; any batch: vectors go in chunks of min(65535, max(1, 2^24 / n_t)) (option "lookup_chunk");
 *                                                                             the workspace is one uint32_t counter per table row and vector of a
 *                                                                             chunk (<= 64 MiB, or one vector's) and 16 B per vector of a chunk, beside
 *                                                                             one staged piece of host data (<= 64 MiB) each way; it does not grow with batch
 *   kzg_logup_terms                         n <= 2^28; any t and batch: chunks of at most 2^21 denominators (whole vectors, or a run of one vector's
 *                                                                             elements with its t + 1 columns), 64 B of workspace per denominator
 *                                                                             (128 MiB) beside one staged piece of host data; it does not grow with batch
 *   kzg_fr_program_setup                    1 <= n_insns <= 65,536; n_cols, n_consts <= 4,096; 1 <= n_out <= 64; at most 16 temporaries (the plan
 *                                                                             holds the validated words on the host: 24 B per instruction)
 *   kzg_fr_program_run                      n <= 2^28; the workspace holds the program (24 B per instruction), the const table (32 B per const),
 *                                                                             16 B per column and 8 B per output, every HOST column whole
 *                                                                             (32 B x col_len, uploaded once each) and, without KZG_OUT_DEVICE,
 *                                                                             every output whole (32 B x n): KZG_ERR_ALLOC if they do not fit
 *   kzg_mle_eq                              m <= 28; the workspace holds the point and, without KZG_OUT_DEVICE, the table whole (32 B x 2^m)
 *   kzg_mle_bind                            n <= 2^28, a power of two; n_cols <= 4,096; the workspace holds 16 B per column, every HOST column whole
 *                                                                             (32 B x n, uploaded once each, folded in that copy) and, for device
 *                                                                             columns with host outputs, every output whole (32 B x n / 2)
 *   kzg_mle_eval                            m <= 28; any batch: tables go in chunks of min(65535, max(1, 2^21 / n)) (option "mle_eval_chunk");
 *                                                                             the workspace is one chunk's first level (32 B x n / 2 per table, none
 *                                                                             up to 2^10 scalars), a HOST chunk whole (32 B x n per table) and, without
 *                                                                             KZG_OUT_DEVICE, the chunk's quotients (32 B x (n - 1) per table): it does
 *                                                                             not grow with batch
 *   kzg_sumcheck_round                      n <= 2^28, a power of two; n_eval <= 16, n_out x n_eval <= 32; the workspace holds the program (24 B per
 *                                                                             instruction), the const table, 8 B per column, one partial sum of 32 B
 *                                                                             per accumulator and wave of the grid (<= 8 MiB at the default grid) and every HOST column
 *                                                                             whole (32 B x n, uploaded once each)
 *   kzg_point_tree_setup                    1 <= k <= 2^22 points             (the plan holds 32 x (3 log2 K + 1) bytes per point of the padded
 *                                                                             size K: 9.0 GB at 2^22); kzg_point_tree_eval: n <= 2^28; any batch:
 *                                                                             chunks of max(1, 2^21 / K) blocks, the workspace does not grow with it
 *   kzg_srs_lagrange_from_monomial_g1       d <= 2^24;  _g2: d <= 2^20
 *   kzg_ntt_g1 / kzg_ntt_g2                 log_n <= 22 / log_n <= 20; any batch: chunks of at most 2^21 / 2^20 points (option
 *                                                                             "group_ntt_chunk_points"), the workspace does not grow with it:
 *                                                                             G1 224 B a point and <= 470 MB of scratch, G2 288 B and <= 302 MB
 *   kzg_fk20_setup                          log_n <= 22                      (the plan holds 2N points of 224 B: 1.9 GB there)
 *   kzg_fk20_cosets_setup                   log_n <= 22, 1 <= log_l <= log_n (the plan holds 8 x 2N rows of 128 B: 8.6 GB there)
 *   kzg_cosets_verifier_setup               log_n <= 22, log_l <= 8           (the plan's window table: 32 x l x 128 affine points of 96 B,
 *                                                                             393 KiB x l: 25 MB at l = 64, 101 MB at l = 256, the bound)
 *   kzg_verify_cosets_batch                 the plan's limits; any count: the workspace is 3 x 8 x 32 x 128 buckets of 192 B (18.9 MB)
 *                                                                             beside one chunk's buffers and 32 B per commitment
 *   kzg_verify_eval_batch                   any count: the same three bucket sets beside one chunk's buffers (16,384 openings), and
 *                                                                             32 B per commitment when indices are given
 *   kzg_witness_coeff_tree                  the plan's 1 <= k <= 2^22, n <= 2^27 (the division's), n - k <= the SRS; any batch: chunks of
 *                                                                             min(16, max(1, 2^24 / max(n, K))) polynomials, the workspace does not grow with it
 *   kzg_msm_g2_bucket                       any n the SRS holds: the workspace is 16 x 32 x 128 buckets of 288 B (18.9 MB) beside the
 *                                                                             staged scalars (32 B per term)
 *   MSM                                     table rows x points < 2^31      (the sorted entry is a 31-bit table index + sign);
 *                                           window_bits 18, 19 (option), and 20 with option sort_single_pass: windows x points < 2^27
 *   kzg_g1_sum_batch                        count <= 2^20, groups <= 2^24
 *   kzg_commit_coeff_sharded_batch          batch <= 2^20
 * SRS footprint in HBM: points x (96 + rows x 128) bytes, rows = windows = ceil(256 / c) with c chosen from the size
 * (c = 20, 13 windows from 2^23 points on; c = 17, 15 windows from 2^17 on; 13 / 10 / 8 bits below: 1.97 GiB at 2^20, 27.5 GiB at 2^24;
 * kzg_srs_footprint computes it).  A host that
 * keeps many SRSs resident can trade speed for memory with option "window_rows" = r < windows: only r table rows are kept and
 * every MSM takes ceil(windows / r) passes over its scalars plus a doubling chain of c x r x (passes - 1) doublings. */
typedef struct kzg_ctx kzg_ctx;
typedef struct kzg_srs kzg_srs;
typedef struct kzg_srs_g2 kzg_srs_g2; /* the G2 half of KZGParams (hs) or a G2 Lagrange basis */

typedef enum {
    KZG_OK = 0,
    KZG_ERR_POINT_NOT_ON_POLY = 1,  /* KZGError::PointNotOnPolynomial      (src/lib.rs:30-31) */
    KZG_ERR_DEGREE_TOO_LARGE = 2,   /* KZGError::PolynomialDegreeTooLarge  (src/lib.rs:34-35) */
    KZG_ERR_SHAPE = 3,              /* a condition on which the reference panics (slice OOB,
                                       assert!(d == evals.d), index out of range, ...) */
    KZG_ERR_BAD_POINT = 4,          /* input point failed to decode / not on the curve */
    KZG_ERR_HIP = -1,
    KZG_ERR_NO_DEVICE = -2,
    KZG_ERR_ALLOC = -3,
    KZG_ERR_INTERNAL = -4
} kzg_status;

enum { KZG_FR_MONT_LE_32 = 0, KZG_FR_CANONICAL_LE_32 = 1 };
enum {
    KZG_G1_AFFINE_MONT_96 = 0,
    KZG_G1_JACOBIAN_MONT_144 = 1,
    KZG_G1_ZCASH_UNCOMPRESSED_96 = 2,
    KZG_G1_ZCASH_COMPRESSED_48 = 3
};
enum {
    KZG_G2_AFFINE_MONT_192 = 0,
    KZG_G2_JACOBIAN_MONT_288 = 1,
    KZG_G2_ZCASH_UNCOMPRESSED_192 = 2,
    KZG_G2_ZCASH_COMPRESSED_96 = 3
};
enum { KZG_IN_DEVICE = 1, KZG_OUT_DEVICE = 2 };

/* ---- context ------------------------------------------------------------------------------- */
const char *kzg_version(void);
/* Hardware queues: the pipelined paths (kzg_msm_g1_batch, concurrent blocking callers) want one HIP hardware queue per stream
 * (lanes + 2); the HIP runtime sizes its pool from GPU_MAX_HW_QUEUES (default 4) at the FIRST HIP call of the process.  The
 * library never changes the host's environment by itself.  A host that wants the full pipeline either exports
 * GPU_MAX_HW_QUEUES (>= 18) itself or calls kzg_init_hw_queues(n) (n = 0: 24) BEFORE its first HIP call -- it sets the
 * variable unless the host already did -- or starts with KZG_SET_HW_QUEUES=1 in the environment (the library's load-time
 * constructor then makes that call).  Otherwise the engine measures the queues it has and narrows the pipeline to fit
 * (4 queues: 3 lanes + 1 accumulation stream; loss: INTEGRATION.md section 6).  kzg_msm_g1_batch with 17-bit windows and 4-byte
 * sort records (2^17 .. 2^21 points) does not run as lanes: the MSMs of a batch travel in groups of sixteen (option "group_msms":
 * 1..16, 0 = lanes), every sort and tail kernel is launched once per group, and one sort stream, one tail stream and two
 * accumulation streams need four queues only.  Measured at 2^20: 467.7 commitments/s on four queues against 448.3 for the narrowed
 * lanes and 461.2 for 13 + 4 lanes on 24 queues; the other sizes measured are in profiles/grouped_pipeline_ab.txt (same bytes).
 * Other sizes and window widths, kzg_witness_*_many, the device group and concurrent blocking callers run
 * as lanes and do want the queues.  kzg_ctx_info reports the group size (group_msms=<g>, 0 = lanes only). */
int kzg_init_hw_queues(int queues);
int kzg_device_count(void);  /* usable HIP devices (0 if none) */
/* "hip=<file of the HIP runtime this library is bound to> runtime_version=<n> driver_version=<n>": a process may hold two HIP
 * runtimes (PyTorch wheels bundle their own); which one the library runs on follows from the host's load order. */
int kzg_runtime_info(char *buf, size_t buflen);
/* device: HIP device ordinal.  Fails with KZG_ERR_NO_DEVICE if no gfx950-class device is usable. */
int kzg_ctx_create(int device, kzg_ctx **out);
void kzg_ctx_destroy(kzg_ctx *ctx);
const char *kzg_last_error(kzg_ctx *ctx);
int kzg_sync(kzg_ctx *ctx);
/* tunables: "window_bits" (0 = auto, 4..20), "window_rows" (0 = one table row per window; applies to SRSs created afterwards),
 * "trusted_points" (0 / 1), "streams" (1..16: batch pipelining depth, default 13), "accum_streams" (0..4), "accum_blocks[_batch]",
 * "sort_threads[_batch]", "ntt_vec_log" / "ntt_vec2_log" (tile widths of the NTT passes), "ntt_kernel" (1 = default: tile load / store fused
 * into the first / last stage pair; 0 = the round-5 three-phase passes, 2 = two butterflies per thread: A/B only), "ntt_three_from" (sizes from
 * 2^this on take three passes of <= 2^8 points, default 23; 0 = never),
 * "ntt_batch_chunk" (0 = default, max(1, 2^21 / n); 1..2^20: kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch work in chunks of that many vectors -- from 2^13
 *  points on a chunk's scratch is chunk x n x 32 bytes; the same bytes), "ntt_batch_rows_log" (0 = auto; 1 + v: the batched single-tile kernel
 *  of sizes up to 2^12 takes 2^v transforms per workgroup, as far as 2^v x n <= 4096 and the LDS layouts go; the same bytes, for A/B and for tests
 *  that put tile boundaries at single-digit batches), "ntt_batch_loop_from" (0 = default, 20; 13..22: batched sizes from 2^this on run as one
 *  kzg_ntt_fr per vector; the same bytes, for A/B), "hw_queues" (0 = measure), "tail_quads" (0 / 1: latency-mode tail kernels of a
 * lone MSM), "host_affine" (1 / 0: a lone result bound for host memory is converted to affine and serialised by the calling
 * thread -- the same field code compiled for the host -- instead of one GPU lane; same bytes, ~90 us less latency),
 * "sort_single_pass" (0 / 1: 17-bit windows sorted in one pass instead of two levels; A/B only),
 * "defer_tail" (1 / 0: kzg_msm_g1_batch enqueues a lane's tail kernels after the sort of the lane's next MSM; default 1),
 * "group_msms" (0..16, default 16: MSMs per sort / tail launch of the grouped shape of kzg_msm_g1_batch, see kzg_init_hw_queues;
 *  0 = never grouped: lanes; the context's workspace grows to min(batch, 2 x group_msms) MSM workspaces of ~0.3 GB at 2^20 and
 *  ~0.5 GB at 2^21 -- 9.5 GB / 15.5 GB for a batch of 32 or more at the default, kept until the context is destroyed),
 * "accum_blocks_small" / "accum_streams_small" / "small_entries" (MSMs of at most small_entries sorted entries -- windows x terms,
 *  default 2^21: up to 2^17 points -- inside a pipeline take a 160-block accumulation grid and are spread over 4 accumulation
 *  streams instead of 480 blocks on 2: +20 % at 2^16, +50 % at 2^14; accum_blocks_small = 0 switches the rule off),
 * "heavy_bins" (sort bins far above their share -- scalars that are bits, bytes, all equal -- sorted in slices by many blocks:
 *  0 = for the 64 MSMs after one that met such a bin (default; the extra kernels cost uniform scalars 0.8 %), 1 = always, 2 = never;
 *  setting it clears the history),
 * "naf_window" (0 / 18, applies to SRSs created afterwards: 18 = positional tables, 2^j P for every bit position j = 255 rows of
 * 128 B per point, scalars recoded in width-18 non-adjacent form -- 13.9 instead of 15 bucket additions per scalar for 17x the
 * table: 34 GB at 2^20; measured +3.7 % batched throughput at 2^20, nothing below 2^19, +1.3 ms on a lone commit: opt-in);
 * "verify_cosets_chunk" (0 = default; n: kzg_verify_cosets works in chunks of at most n cells),
 * "verify_eval_batch_chunk" (0 = default, 16384; n <= 16384: kzg_verify_eval_batch works in chunks of at most n openings),
 * "multiopen_points_chunk" (0 = default, min(16, 2^22 / d); n <= 16: kzg_multiopen_eval_commit works in chunks of at most n distinct points),
 * "multi_eval_segment" (0 = planned from n, k and batch; a power of two >= 8: kzg_poly_multi_eval cuts the coefficients into segments of
 *  that length) and "multi_eval_points_chunk" (0 = default, 4096; n: at most min(n, 4096) points per pass); either one set also keeps the
 *  call on its own kernels where it would take one kzg_poly_eval scan per value (up to 7 values): the same bytes, for A/B and tests,
 * "poly_divide_base" (0 = default, 64; a power of two in 1..64: the coefficients of the power-series inverse kzg_poly_divide's one-workgroup
 *  base kernel produces before Newton doubling takes over; the same bytes, for A/B and for tests that drive several Newton levels at tiny shapes),
 * "fr_scan_tile" (0 = default, 2048; a power of two in 8..2048: the elements one workgroup of kzg_fr_scan / kzg_fr_grand_product scans, that is
 *  1..256 threads of eight; read per call; the same bytes, for tests that reach tile and carry boundaries at n in the hundreds), "fr_scan_stage"
 *  (0 = default, 64 MiB; a multiple of 32 up to 64 MiB: the bytes of one staged piece of host data in those calls and kzg_fr_batch_inverse) and
 *  "fr_scan_chunk" (0 = the rule alone; 1..65535: at most that many vectors per chunk of launches); the same bytes, for tests,
 * "lookup_spare_log" (0 = default, 2; 1..4: kzg_lookup_setup gives the plan next_pow2(n_t) << (v - 1) slots -- load <= 0.5 by default; with 1 a
 *  power-of-two table of distinct keys fills every slot), "lookup_hash_bits" (0 = all; 1..32: only the low v - 1 bits of a key's hash and tag
 *  are kept -- with 1 every key starts at slot 0 and the table is one probe chain that wraps, every compare a full-key compare); both are read
 *  at setup and kept by the plan; "lookup_stage" (0 = default, 64 MiB; a multiple of 32 up to 64 MiB: the bytes of one staged piece of host
 *  data in kzg_lookup_setup / kzg_lookup_count / kzg_logup_terms, and 1 / 32 of it the denominators of one chunk of kzg_logup_terms) and
 *  "lookup_chunk" (0 = the rule alone; 1..65535: at most that many vectors per chunk), read per call; the same bytes, for tests,
 * "fr_program_block" (0 = the rule: 256 threads a workgroup up to 4 temporaries, 128 up to 8, 64 above; 64 / 128 / 256: that many, whatever
 *  the plan's temporaries take of the LDS; read per call of kzg_fr_program_run; the same bytes, for tests),
 * "sumcheck_block" (0 = the rule of "fr_program_block" over temporaries + n_out x n_eval accumulators; 64 / 128 / 256: that many threads a
 *  workgroup of kzg_sumcheck_round, halved while the slots would pass 128 KiB of LDS), "sumcheck_grid" (0 = default, what the chip holds at
 *  once; 1..2^22: at most that many workgroups, so that every lane strides over many pairs), "mle_block" (0 = default, 256; 64 / 128 / 256:
 *  the threads of a workgroup of kzg_mle_eq / _bind / _eval), "mle_local_log" (0 = default, 10; 1..10: kzg_mle_eq builds its first v levels,
 *  and kzg_mle_eval binds its last v variables, inside one workgroup's LDS; the levels beyond run one launch each) and "mle_eval_chunk"
 *  (0 = the rule alone; 1..65535: at most that many tables per chunk of kzg_mle_eval); read per call; the same bytes, for tests that reach
 *  every boundary at m <= 13,
 * "point_tree_leaf" (0 = default, 16; a power of two in 1..16: kzg_point_tree_setup multiplies nodes of up to that many points by its schoolbook
 *  kernels and the levels above through transforms; read at setup and kept by the plan; the same bytes, for tests that reach many levels at tiny k),
 * "g2_msm_slice" (0 = default, 2048; a power of two in 1..2048: the points one workgroup of kzg_msm_g2_bucket sorts by digit) and
 *  "g2_msm_slots" (0 = default, 16; 1..16: the slice slots of its bucket arena, so a chunk is slots x slice points); read per call; the same
 *  bytes, for tests that put slice and chunk boundaries at single-digit n,
 * "host_pairing" (1 / 0: the one pairing check that ends kzg_verify_cosets_batch / kzg_verify_eval_batch runs on the calling thread -- the same tower code
 *  compiled for the host -- instead of in a one-thread kernel; the same verdict, default 1),
 * "fk20_cosets_combine" (0 = the shared-doubling Straus kernel, default; 1 = one mul256 per term: the same bytes, for comparison),
 * "g2_ntt_mul" (0 = the twiddle products of the G2 DFT split by the endomorphism psi into one joint chain, default; 1 = signed digits over
 *  the whole scalar: the same bytes, for comparison), "group_ntt_chunk_points" (0 = default, 2^21 for kzg_ntt_g1 and 2^20 for kzg_ntt_g2;
 *  1..2^22: the points of one chunk of arrays, at least one array) and "group_ntt_threads" (0 = default, 2^18 for G1 and 2^17 for G2; a
 *  power of two in 256..2^17: the threads of one grid-stride launch of those calls and so their scratch slots); read per call; the same
 *  bytes, for tests that make every thread loop at 2,048 points,
 * "g2_lagrange_dft_from" (default 2048; a power of two in 2..2^20: kzg_srs_lagrange_from_monomial_g2 runs the G2 inverse DFT from this
 *  size on and one d-term sum per row below it; the same points either way),
 * unknown keys -> KZG_ERR_SHAPE */
int kzg_ctx_set_option(kzg_ctx *ctx, const char *key, int64_t value);
/* "device=<d> lanes=<n> accum_streams=<m> hw_queues_found=<q> narrowed_from=<L>+<A>|none witness_cache_slots=<s>": the plan of the
 * batched / concurrent-caller pipeline (zeros before the first such call) and whether the process' pool of hardware queues forced it
 * below what was asked for -- another context, an RCCL communicator or the host's own streams hold queues too, and a narrowed
 * pipeline loses 10-25 % of its batched rate.  The narrowing is also reported once per context on stderr. */
int kzg_ctx_info(kzg_ctx *ctx, char *buf, size_t buflen);

/* ---- SRS (KZGParams.gs, src/lib.rs:14-19; lagrange_basis_g, src/eval_form.rs:40-46) --------- */
/* Upload n G1 points once; they stay resident in HBM in the engine's internal layout
 * (affine Montgomery + per-window precomputed multiples).  Caller keeps ownership of `pts`. */
int kzg_srs_upload_g1(kzg_ctx *ctx, const void *pts, size_t n, int pfmt, kzg_srs **out);
/* setup(s, n), G1 half (src/lib.rs:38-47): gs[i] = [s^i]G, generated on the GPU. */
int kzg_srs_setup_g1(kzg_ctx *ctx, const void *s, int sfmt, size_t n, kzg_srs **out);
/* One contiguous shard of the same SRS: gs[first .. first+n) = [s^(first+i)]G (multi-GPU sharding). */
int kzg_srs_setup_g1_shard(kzg_ctx *ctx, const void *s, int sfmt, size_t first, size_t n, kzg_srs **out);
/* Lagrange-basis SRS for a known secret: L_i(s) G, i < d, d a power of two.  Same group elements
 * as compute_lagrange_basis(&setup(s, d)).0 (src/eval_form.rs:254-280), in O(d) not O(d^3). */
int kzg_srs_setup_lagrange_g1(kzg_ctx *ctx, const void *s, int sfmt, size_t d, kzg_srs **out);
/* compute_lagrange_basis (src/eval_form.rs:254-280), G1 half, from the monomial SRS alone (no secret): the inverse
 * group-NTT of gs, L_i = (1/d) sum_j w^(-ij) gs[j] (radix-2 over G1 points, one 255-bit scalar multiplication per
 * butterfly: ~0.7 s at d = 2^20).  d = len(gs) must be a power of two (KZG_ERR_SHAPE otherwise, the reference's assert)
 * and at most 2^24. */
int kzg_srs_lagrange_from_monomial_g1(kzg_ctx *ctx, const kzg_srs *monomial, kzg_srs **out);
int kzg_srs_download_g1(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, size_t n, void *out, int pfmt);
size_t kzg_srs_len(const kzg_srs *srs);
/* HBM bytes an SRS of n points occupies under the given options (0 = engine defaults); host-only helper */
int kzg_srs_footprint(size_t n, int window_bits, int window_rows, size_t *bytes);
void kzg_srs_free(kzg_ctx *ctx, kzg_srs *srs);

/* ---- MSM: G1Projective::multi_exp(&gs[offset..offset+n], scalars) --------------------------- */
/* (call sites src/coeff_form.rs:61,78,102; src/eval_form.rs:118,136).  n may be 0 (-> identity). */
int kzg_msm_g1(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n, int sfmt,
               int flags, void *out, int ofmt);
/* `batch` scalar vectors (each n scalars, contiguous, stride n*32 B) against one SRS; out gets
 * `batch` points.  Throughput mode: independent MSMs are pipelined on several HIP streams, two in flight per lane (option
 * "defer_tail"): the context's workspace grows to 2 x `streams` MSM workspaces (2 x 16 x ~0.25 GB at 2^20, 17-bit windows). */
int kzg_msm_g1_batch(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n,
                     size_t batch, int sfmt, int flags, void *out, int ofmt);
/* sum of `count` G1 points (multi-GPU combine of per-rank partial MSMs). points in pfmt. */
int kzg_g1_sum(kzg_ctx *ctx, const void *points, size_t count, int pfmt, int flags, void *out, int ofmt);
/* `groups` independent sums: out[g] = sum_i points[g*count + i] (batched multi-GPU combine). */
int kzg_g1_sum_batch(kzg_ctx *ctx, const void *points, size_t count, size_t groups, int pfmt, int flags, void *out,
                     int ofmt);
/* The DFT over the group (not a reference method; EvaluationDomain::fft / ifft, src/ft.rs:100-140, with points for values): `batch`
 * arrays of d = 2^log_n points, array b at points + b d, w = compute_omega(d).omega.
 *   forward:  out[b][m] = sum_j [w^(jm)] P[b][j]
 *   inverse:  out[b][j] = [1/d] sum_m [w^(-jm)] P[b][m]
 * Natural order in and out; the inverse is scaled, so the two directions undo each other.  Moves a vector of commitments or proofs
 * between coefficient and evaluation form, extends one by a low-degree extension (inverse, pad, forward), or builds Lagrange parameters
 * from a ceremony file.  kzg_ntt_g1 runs the G1 DFT of the FK20 calls (radix 2, the twiddle products split by the GLV endomorphism,
 * the 1/d one 255-bit product per point); log_n <= 22.  points in any KZG_G1_* format, out in any KZG_G1_* format; host memory, or
 * device memory with KZG_IN_DEVICE / KZG_OUT_DEVICE; out may be points when the two formats have the same size.  The points are
 * checked like those of kzg_srs_upload_g1 (curve and subgroup; option "trusted_points": curve only -- the caller then vouches for the
 * subgroup, on which the endomorphism split relies): KZG_ERR_BAD_POINT with out untouched.  log_n == 0 copies the input, re-encoded;
 * batch == 0: KZG_OK, nothing written.  KZG_ERR_SHAPE before out is touched: a NULL argument, an unknown format, log_n over the
 * limit, in place with formats of different sizes.  The batch runs in chunks of at most 2^21 points (option
 * "group_ntt_chunk_points"; with more than one chunk every point is checked before the first is written), so the workspace does not
 * grow with batch.  Takes the context exclusively. */
int kzg_ntt_g1(kzg_ctx *ctx, const void *points, uint32_t log_n, size_t batch, int inverse, int pfmt, int flags, void *out, int ofmt);
/* The same over G2, on kernels of its own (kzg_amd/csrc/g2ntt.hip): log_n <= 20, chunks of at most 2^20 points, KZG_G2_* formats,
 * the points checked like those of kzg_srs_upload_g2.  The twiddle products are split four ways by the endomorphism psi (option
 * "g2_ntt_mul" = 1: signed digits over the whole scalar, the same bytes).  DESIGN.md section 3.5h. */
int kzg_ntt_g2(kzg_ctx *ctx, const void *points, uint32_t log_n, size_t batch, int inverse, int pfmt, int flags, void *out, int ofmt);

/* ---- multi-GPU: the SRS sharded over up to 8 GPUs, partial commitments combined over RCCL / xGMI ---------------------
 * (north star: "MSM shards the SRS across up to 8 GPUs with an RCCL all-reduce of partial bucket sums"; the seam is the
 * multi_exp call of KZGProver::commit, src/coeff_form.rs:59-64, and of create_witness, :66-81.)
 * A kzg_mctx is a group of `world` GPUs (ranks).  Rank r holds the contiguous SRS range kzg_shard_range(n, r, world) resident
 * and reduces the matching scalar slice of every polynomial to ONE partial point on its GPU; the 144-byte Jacobian partials are
 * exchanged with one ncclAllGather and every rank adds them locally (EC addition is not an RCCL reduction op, so the
 * "all-reduce" is all-gather + local sum).  Two ways to form the group:
 *   - one host process driving n GPUs: kzg_mctx_create(devices, n)   (ncclCommInitAll; one host thread per device per call);
 *   - one process per GPU:  rank 0 calls kzg_mctx_unique_id, the host distributes the 128 bytes by any means (MPI, a TCP
 *     store, torch.distributed), every rank calls kzg_mctx_create_rank(device, rank, world, id)   (ncclCommInitRank).
 * RCCL (librccl.so.1) is loaded on first use; a group of one GPU needs no RCCL unless option "always_gather" is set.
 * Streams: all contexts of one device in a process -- plain ones and a group's -- take their streams from ONE pool (lane i of every
 * context is the same HIP stream), 13 lanes + 4 accumulation streams (+ one exchange stream per device group): the runtime multiplexes a process' streams onto one pool of
 * hardware queues (24 after kzg_init_hw_queues) of which an RCCL communicator needs about six, and streams that share a queue
 * serialise.  A plain prover context and a device group alive in one process therefore cost each other nothing (group path 471
 * against 473 commitments/s alone; both committing at once 512-517 in total).  kzg_ctx_info / kzg_mctx_info report each context's plan
 * and say so (also once on stderr) when the pool was short and a pipeline had to be narrowed.
 * Every entry point below is collective in the one-process-per-GPU mode: all ranks call it with the same arguments.
 * Failures stay collective too: a rank whose local phase fails still enters the exchange, its status travels with its
 * partials, and EVERY rank returns that error (no rank is left waiting inside the all-gather).  A rank-local resource failure
 * BEFORE the exchange (growing the exchange / quotient buffers: the only allocations a call makes, and only when a call is larger
 * than any the ranks have agreed on before) is agreed on through a status-only all-gather over buffers that exist since the group
 * was formed; after such a failure the failing call may simply be repeated.  What
 * cannot be agreed on -- a peer process that died, a hung GPU, a rank that could not create its communicator -- is bounded by a
 * deadline: the wait behind every exchange polls for at most "gather_timeout_ms" (kzg_mctx_set_option, default 60000, 0 = wait
 * for ever); when it expires the communicators are aborted (ncclCommAbort), the call returns KZG_ERR_INTERNAL and the group is
 * DEAD -- every later call on it fails at once with KZG_ERR_INTERNAL; destroy it and form a new one (kzg_mctx_destroy of a dead
 * group never synchronises on a stream an aborted collective still holds: such a context is left behind, with a line on stderr).
 * Communicator FORMATION is bounded the same way: ncclGetUniqueId / ncclCommInitRank / ncclCommInitAll / ncclCommDestroy run on
 * a helper thread and the caller waits at most "comm_timeout_ms" (kzg_mctx_set_option for a group that forms its communicator
 * lazily; the environment variable KZG_COMM_TIMEOUT_MS for the ones formed inside kzg_mctx_create*; default 60000, 0 = wait for
 * ever).  RCCL bootstraps over TCP on an interface of its own choosing even on one node, and a host whose interface swallows
 * packets stalls it for minutes.  On expiry the call returns KZG_ERR_INTERNAL with the phase timings in its message
 * (kzg_mctx_last_error, or kzg_mctx_create_error when the group was never handed out), the group is dead, and -- because the
 * abandoned call may hold RCCL's locks for ever -- no further communicator is formed in this process.  A one-node host should
 * export NCCL_SOCKET_IFNAME=lo, NCCL_RAS_ENABLE=0 and NCCL_IB_DISABLE=1 before the first RCCL call (INTEGRATION.md section 5b;
 * kzg_amd.api.DeviceGroup does).  KZG_DEBUG=1 prints every phase with its duration on stderr. */
typedef struct kzg_mctx kzg_mctx;
typedef struct kzg_msrs kzg_msrs;   /* an SRS sharded contiguously over the group */
enum { KZG_UNIQUE_ID_BYTES = 128 };
int kzg_mctx_create(const int *devices, int n, kzg_mctx **out);
int kzg_mctx_unique_id(void *id_out);
int kzg_mctx_create_rank(int device, int rank, int world, const void *unique_id, kzg_mctx **out);
void kzg_mctx_destroy(kzg_mctx *m);
const char *kzg_mctx_last_error(kzg_mctx *m);
/* why the calling thread's last kzg_mctx_create / kzg_mctx_create_rank / kzg_mctx_unique_id failed (no group exists to ask);
 * "" when it did not.  Valid until the thread's next call of one of the three. */
const char *kzg_mctx_create_error(void);
/* "rccl=<file> version=<n> hip=<runtime file> world=.. local=.. mode=.. formation_ms=<f> phases_ms=[load=.. uid=.. init=..
 * first_exchange=.. destroy=..] comm_timeout_ms=.. gather_timeout_ms=.. dead=0|1": which RCCL the group adopted (the copy the
 * process already holds, else librccl.so.1 from the library path), the HIP runtime it is bound to, and what forming the
 * communicator cost (wall-clock ms per phase: loading RCCL, ncclGetUniqueId, ncclCommInit*, the first exchange -- RCCL loads its
 * kernels there --; -1 = has not happened).  The library refuses an RCCL that
 * is bound to a different HIP runtime than itself (streams and device pointers cross the boundary): KZG_ERR_INTERNAL. */
int kzg_mctx_info(kzg_mctx *m, char *buf, size_t buflen);
int kzg_mctx_world(const kzg_mctx *m);        /* ranks in the group */
int kzg_mctx_local_count(const kzg_mctx *m);  /* GPUs this process drives (n, or 1 in the per-process mode) */
int kzg_mctx_rank(const kzg_mctx *m, int local_index);          /* global rank of a local GPU */
kzg_ctx *kzg_mctx_ctx(kzg_mctx *m, int local_index);            /* its single-GPU context (NTT, scans, device memory) */
/* options: "always_gather" (run the collective even in a group of one), "gather_timeout_ms", "comm_timeout_ms" (above), plus every
 * kzg_ctx_set_option key (applied to all) */
int kzg_mctx_set_option(kzg_mctx *m, const char *key, int64_t value);
/* rank r of `world` holds terms [lo, hi) of n: the first n % world ranks get one extra.  Host-only helper. */
int kzg_shard_range(size_t n, int rank, int world, size_t *lo, size_t *hi);
/* setup(s, n), G1 half, sharded: rank r generates gs[lo_r .. hi_r) on its GPU (src/lib.rs:38-47). */
int kzg_srs_setup_g1_sharded(kzg_mctx *m, const void *s, int sfmt, size_t n, kzg_msrs **out);
/* KZGParams.gs supplied by the caller: `pts` is the WHOLE vector (n points, host); every rank uploads its own range. */
int kzg_srs_upload_g1_sharded(kzg_mctx *m, const void *pts, size_t n, int pfmt, kzg_msrs **out);
size_t kzg_msrs_len(const kzg_msrs *srs);
const kzg_srs *kzg_msrs_shard(const kzg_msrs *srs, int local_index, size_t *first);  /* the resident shard and its first index */
void kzg_msrs_free(kzg_mctx *m, kzg_msrs *srs);
/* KZGProver::commit over the group (src/coeff_form.rs:59-64).  coeffs: the whole polynomial (n scalars, host), every rank
 * reads its slice; with KZG_IN_DEVICE `coeffs` is instead an array of kzg_mctx_local_count() device pointers, entry i
 * pointing at local GPU i's slice ([hi - lo] scalars, resident in that GPU's HBM).  out: one point (host), on every rank.
 * KZG_ERR_SHAPE if n > kzg_msrs_len (the slice index panic).  (This is the sharded multi_exp: with a Lagrange-basis SRS
 * uploaded through kzg_srs_upload_g1_sharded it is KZGProverEvalForm::commit, src/eval_form.rs:114-122, as well.) */
int kzg_commit_coeff_sharded(kzg_mctx *m, const kzg_msrs *srs, const void *coeffs, size_t n, int sfmt, int flags, void *out,
                             int ofmt);
/* `batch` polynomials of n coefficients each (host: contiguous, stride n * 32 B; KZG_IN_DEVICE: per local GPU a
 * [batch][hi - lo] array of slices).  One all-gather of batch x 144 B per rank for the whole batch.  out: batch points. */
int kzg_commit_coeff_sharded_batch(kzg_mctx *m, const kzg_msrs *srs, const void *coeffs, size_t n, size_t batch, int sfmt,
                                   int flags, void *out, int ofmt);
/* KZGProver::create_witness over the group (src/coeff_form.rs:66-81): every rank computes the quotient (p - y)/(X - x) on its
 * GPU (a replicated O(n) scan) and reduces its own slice of it.  coeffs: the whole polynomial in host memory, or with
 * KZG_IN_DEVICE an array of kzg_mctx_local_count() device pointers, entry i = the WHOLE polynomial resident on local GPU i.
 * KZG_ERR_POINT_NOT_ON_POLY iff p(x) != y. */
int kzg_witness_coeff_sharded(kzg_mctx *m, const kzg_msrs *srs, const void *coeffs, size_t n, const void *x, const void *y,
                              int sfmt, int flags, void *out, int ofmt);
/* KZGProver::create_witness_batched over the group (src/coeff_form.rs:83-111): interpolant and quotient (p - I)/Z replicated on
 * every GPU (NTTs do not shard), the quotient MSM sharded like the commit.  Arguments and errors as kzg_witness_coeff_batched;
 * coeffs as for kzg_witness_coeff_sharded.  out_w: one point (host), out_r: the interpolant (host, sfmt), on every rank. */
int kzg_witness_coeff_batched_sharded(kzg_mctx *m, const kzg_msrs *srs, const void *coeffs, size_t n, const void *xs,
                                      const void *ys, size_t k, int sfmt, int flags, void *out_w, int ofmt, void *out_r,
                                      size_t *out_r_len);

/* KZGProverEvalForm::create_witness over the group (src/eval_form.rs:124-140): `lagrange` is the Lagrange-basis SRS sharded over
 * the group (kzg_srs_upload_g1_sharded); every rank computes div_by_omega_i of (evals - evals[index]) on its GPU (replicated O(d)
 * pass) and reduces its slice of the quotient.  evals: d scalars in host memory, or with KZG_IN_DEVICE an array of
 * kzg_mctx_local_count() device pointers (the whole vector resident on each local GPU).  KZG_ERR_SHAPE if index >= d, d is not a
 * power of two or d > kzg_msrs_len (the reference's panics). */
int kzg_witness_eval_sharded(kzg_mctx *m, const kzg_msrs *lagrange, const void *evals, size_t d, size_t index, int sfmt, int flags,
                             void *out, int ofmt);

/* ---- NTT: EvaluationDomain::fft / ifft (src/ft.rs:111-140; best_fft :274-288) --------------- */
/* EvaluationDomain::compute_omega (src/ft.rs:55-76): m = next pow2 >= d, exp = log2 m, omega.
 * Returns KZG_ERR_DEGREE_TOO_LARGE if exp >= 32.  Host-only helper; omega written in sfmt. */
int kzg_compute_omega(size_t d, size_t *m, uint32_t *exp, void *omega, int sfmt);
/* In place, natural order in and out: out[i] = sum_j a[j] w^(ij); inverse uses w^-1 and scales by
 * d^-1.  The transform is linear, so data may be in either Fr format (it is preserved).  There is no sfmt parameter: a word at or
 * above r counts as its residue (canonical data under the rule above), and every output word is the residue below r. */
int kzg_ntt_fr(kzg_ctx *ctx, void *data, uint32_t log_n, int inverse, int flags);
/* coset_fft / icoset_fft (src/ft.rs:168-178): distribute_powers(g = 7) then fft; ifft then g^-i. */
int kzg_coset_ntt_fr(kzg_ctx *ctx, void *data, uint32_t log_n, int inverse, int sfmt, int flags);
/* `batch` transforms of 2^log_n points each, in place, natural order in and out; vector b starts at data + b * stride * 32 bytes.
 * stride is in elements: 0 means 2^log_n (contiguous), otherwise stride >= 2^log_n; the words between the vectors are neither
 * read for the result nor changed.  The bytes of `batch` calls of kzg_ntt_fr / kzg_coset_ntt_fr, one per vector, in fewer launches:
 * up to 2^12 points a workgroup takes several whole transforms into its LDS (one launch per chunk); from 2^13 to 2^19 points the two
 * pass kernels of kzg_ntt_fr run once per chunk with the vector index folded into their grids; from 2^20 points on (and with option
 * "ntt_kernel" = 0) one transform fills the chip and the call is a loop over the vectors (measured on one MI355X, batched kernels against
 * the loop inside one call: 0.18 against 0.33 ms at 2^18 x 8, 0.40 against 0.46 ms at 2^19 x 8, 0.39 against 0.38 ms at 2^20 x 4, 0.42 against
 * 0.42 ms at 2^21 x 2).  The coset call scales
 * all vectors in one launch.  KZG_ERR_SHAPE: 0 < stride < 2^log_n, (batch - 1) * stride + 2^log_n elements or their bytes overflow
 * size_t, log_n > 28; KZG_ERR_DEGREE_TOO_LARGE: log_n >= 32; batch = 0: KZG_OK, nothing touched.  Blocking; callable from many threads. */
int kzg_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int flags);
int kzg_coset_ntt_fr_batch(kzg_ctx *ctx, void *data, uint32_t log_n, size_t batch, size_t stride, int inverse, int sfmt, int flags);

/* EvaluationDomain::z (src/ft.rs:182-187): tau^d - 1.  Host-only helper; tau (< r in canonical form) and out are both in sfmt. */
int kzg_domain_z(size_t d, const void *tau, int sfmt, void *out);
/* EvaluationDomain::divide_by_z_on_coset (src/ft.rs:192-217): data[i] *= 1 / (7^d - 1), d = 2^log_n. */
int kzg_divide_by_z_on_coset(kzg_ctx *ctx, void *data, uint32_t log_n, int sfmt, int flags);
/* EvaluationDomain::mul_assign / sub_assign (src/ft.rs:220-271): a[i] *= b[i] / a[i] -= b[i], n elements each
 * (KZG_IN_DEVICE: both resident). */
int kzg_fr_vec_mul(kzg_ctx *ctx, void *a, const void *b, size_t n, int sfmt, int flags);
int kzg_fr_vec_sub(kzg_ctx *ctx, void *a, const void *b, size_t n, int sfmt, int flags);

/* ---- coefficient form (src/coeff_form.rs) ---------------------------------------------------- */
/* KZGProver::commit (:59-64).  coeffs[0..n) = polynomial.slice_coeffs(); KZG_ERR_SHAPE if n > SRS. */
int kzg_commit_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, int sfmt, int flags,
                     void *out, int ofmt);
/* KZGProver::create_witness (:66-81): [(p - y)/(X - x)]_1; KZG_ERR_POINT_NOT_ON_POLY iff p(x) != y.
 * x, y are host scalars in sfmt.  n = polynomial.num_coeffs() >= 1. */
int kzg_witness_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, const void *x,
                      const void *y, int sfmt, int flags, void *out, int ofmt);
/* Throughput form of the above ("256 independent create_witness calls sharing one SRS"): `count`
 * openings (xs[j], ys[j]) of ONE polynomial, pipelined like kzg_msm_g1_batch -- quotient scan and MSM of opening j on lane
 * j % streams.  out: count points in ofmt.  status (optional, count ints): 0 or KZG_ERR_POINT_NOT_ON_POLY per opening, the
 * call then returns KZG_OK; without it the call returns KZG_ERR_POINT_NOT_ON_POLY if any opening is off the polynomial (every
 * witness is still written).  Not a reference method: equivalent to calling create_witness count times. */
int kzg_witness_coeff_many(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, const void *xs, const void *ys,
                           size_t count, int sfmt, int flags, void *out, int ofmt, int *status);
/* KZGProver::create_witness_batched (:83-111): w = [(p - I)/Z]_1 and r = I (the interpolant through
 * (xs, ys)).  xs, ys: k host scalars.  out_r receives *out_r_len scalars (host, sfmt): k normally,
 * 2 for k == 1 (the reference returns X + (y - x), src/polynomial.rs:244-247).
 * KZG_ERR_POINT_NOT_ON_POLY iff some p(xs[i]) != ys[i].
 * Opening-point sets are remembered per context: what depends on xs alone (Z, the barycentric weights, the coset shift, 1 / Z on the
 * coset: N x 32 bytes) is kept in one of "witness_cache_slots" equal slots (kzg_ctx_set_option, default 16, 0 = off; the pool is
 * allocated by the first call, sized for that call), so that opening many polynomials at ONE point set -- the way batched openings are
 * used -- pays for the point set once.  Results are identical with and without the cache.  kzg_prof_get(ctx, "point_set_cache",
 * &hits, &misses_as_double) reports its use. */
int kzg_witness_coeff_batched(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n,
                              const void *xs, const void *ys, size_t k, int sfmt, int flags, void *out_w,
                              int ofmt, void *out_r, size_t *out_r_len);
/* KZGVerifier::verify_poly (:119-124): *ok = (commit(coeffs) == commitment). */
int kzg_verify_poly_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *commitment, int pfmt,
                          const void *coeffs, size_t n, int sfmt, int flags, int *ok);

/* ---- evaluation form (src/eval_form.rs) ------------------------------------------------------ */
/* KZGProverEvalForm::commit (:114-122): MSM against the Lagrange SRS.  KZG_ERR_SHAPE unless
 * d == kzg_srs_len(lagrange) (assert!(self.d == evals.d)). */
int kzg_commit_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, int sfmt, int flags,
                    void *out, int ofmt);
/* KZGProverEvalForm::create_witness (:124-140) incl. div_by_omega_i (:58-84).  KZG_ERR_SHAPE if
 * i >= d (the reference panics on the index). */
int kzg_witness_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t i, int sfmt,
                     int flags, void *out, int ofmt);
/* Throughput form: `count` openings (indices[j]) of ONE evaluation vector, pipelined like kzg_msm_g1_batch.  out: count points.
 * Not a reference method: equivalent to calling KZGProverEvalForm::create_witness count times. */
int kzg_witness_eval_many(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, const size_t *indices,
                          size_t count, int sfmt, int flags, void *out, int ofmt);
/* ---- openings at ANY point of Fr, in batches, against the Lagrange SRS alone (not a reference method) -------------------------
 * kzg_witness_eval opens at a point of the domain, by index.  These three open at any z: with f_i = p(w^i), i < d = 2^k,
 * w = compute_omega(d).omega,
 *   z off the domain:  y = (z^d - 1)/d  sum_i f_i w^i / (z - w^i),  q_i = (f_i - y) / (w^i - z),  witness = sum_i q_i L_i;
 *   z = w^m:           y = f_m and q is kzg_quotient_eval(evals, d, m): the witness bytes are kzg_witness_eval(evals, d, m)'s.
 * Which case a z is in is decided on the host (z^d == 1; m is read one bit per squaring level), so no zero denominator reaches
 * the batch inversion.  The denominators are formed and inverted once per DISTINCT z of a chunk: a batch that shares one
 * challenge pays for one inversion of d elements per chunk.  No monomial SRS, no inverse transform.
 * evals: batch x d scalars in sfmt, stride d; KZG_IN_DEVICE applies to it.  zs: batch host scalars in sfmt, each < r (else
 * KZG_ERR_SHAPE, the rule for single host scalars); always host memory.  ys_out: batch scalars in sfmt, always host memory.
 * KZG_ERR_SHAPE, before any memory is touched: d == 0 or not a power of two, an unknown format, a NULL input, a z >= r, and for
 * kzg_open_eval d != kzg_srs_len(lagrange) (assert!(self.d == evals.d)) or an SRS on another GPU.  batch == 0 returns KZG_OK.
 * d == 1: y = f_0 and the witness is the identity. */
/* ys_out[b] = p_b(zs[b]).  Leases one lane like the other blocking calls; works in chunks of at most min(16, 2^22 / d)
 * polynomials. */
int kzg_eval_form_eval(kzg_ctx *ctx, const void *evals, size_t d, size_t batch, const void *zs, int sfmt, int flags,
                       void *ys_out);
/* The any-point sibling of kzg_quotient_eval, one polynomial: *y_out = p(z) (host, optional) and q_out = the d values of
 * (p - y)/(X - z) on the domain (host, or device with KZG_OUT_DEVICE) -- the scalars of the witness MSM. */
int kzg_quotient_eval_at(kzg_ctx *ctx, const void *evals, size_t d, const void *z, int sfmt, int flags, void *y_out,
                         void *q_out);
/* The full call: ys_out[b] = p_b(zs[b]) and out_w[b] = its witness in ofmt (host, or device with KZG_OUT_DEVICE).  Either
 * output may be NULL, not both (out_w == NULL: no MSM runs).  Takes the context exclusively, like kzg_msm_g1_batch whose
 * pipeline the quotients feed without leaving HBM: chunks of one polynomial per lane (option "streams"), the Fr stage of chunk
 * c + 1 on a stream of its own beside the MSMs of chunk c.  The workspace does not grow with `batch` (but for its 32 bytes per
 * value): per chunk 2 x d x 32 bytes of quotients per lane, at most as much again for denominators and inverses (one set per
 * distinct z), and the lanes' MSM workspaces. */
int kzg_open_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t batch, const void *zs, int sfmt,
                  int flags, void *ys_out, void *out_w, int ofmt);
/* ---- many polynomials opened at ONE point with a single folded witness (not a reference method) -------------------------------
 * The shape of PLONK-style provers and aggregate blob proofs: t polynomials p_0 .. p_{t-1} opened at a common z are answered by their
 * t values and ONE group element.  With a challenge gamma,
 *   F = sum_i gamma^i p_i,   y_F = sum_i gamma^i y_i,   witness = [(F - y_F)/(X - z)]_1:
 * one MSM per group of t polynomials instead of t, after one streaming pass over the inputs (the fold).  `groups` such groups per call,
 * group g with its own point zs[g] and challenge gammas[g] (host scalars in sfmt; a z >= r, a gamma == 0 or >= r: KZG_ERR_SHAPE).
 * kzg_verify_fold (below) checks the result; what the caller owes for gamma is said there.
 * The fold alone: out[g d + j] = sum_{i < t} gammas[g]^i vecs[(g t + i) d + j] for `groups` groups of t vectors of d >= 1 scalars (any d,
 * not only a power of two).  vecs and out are host memory, or device memory with KZG_IN_DEVICE / KZG_OUT_DEVICE; out has the form of
 * the inputs (canonical in, canonical out; Montgomery in, Montgomery out).  Canonical inputs may hold any 256-bit value: they count as
 * their residue.  Host inputs are staged in pieces of at most 64 MiB with the running sum on the device, host outputs come back per
 * chunk of groups: the workspace does not grow with t x groups.  Leases one lane.  KZG_ERR_SHAPE, before memory is touched: d == 0,
 * t == 0, a NULL pointer with groups > 0, an unknown format, a gamma == 0 or >= r, groups x t x d x 32 beyond size_t.  groups == 0:
 * KZG_OK. */
int kzg_fr_fold(kzg_ctx *ctx, const void *vecs, size_t d, size_t t, size_t groups, const void *gammas, int sfmt, int flags, void *out);
/* Evaluation form: evals holds groups x t vectors of d values (stride d; KZG_IN_DEVICE applies), group g opened at zs[g], any point
 * of Fr.  ys_out[g t + i] = p_{g,i}(zs[g]) (host, optional; the values of kzg_eval_form_eval) and out_w[g] = the folded witness in ofmt
 * (host, or device with KZG_OUT_DEVICE; optional; not both NULL).  At z = w^m the witness bytes are kzg_witness_eval's of the folded
 * vector at m; everywhere they are kzg_open_eval's of the folded vector.  Takes the context exclusively like kzg_open_eval, whose
 * pipeline it feeds: per chunk of one group per lane the t vectors of a group are evaluated (only when ys_out is given) and folded
 * in pieces of at most 16 vectors, the folded vectors go through the evaluation stage once more for their quotients, and the MSMs
 * of the chunk run beside the Fr stage of the next.  Workspace: one piece of staged input (host input only), per lane one folded vector
 * and two quotients of d scalars, the denominators and inverses of one chunk, the lanes' MSM workspaces, 32 bytes per value.
 * KZG_ERR_SHAPE as for kzg_open_eval, and t == 0, a gamma == 0 or >= r; groups == 0: KZG_OK. */
int kzg_open_fold_eval(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t t, size_t groups, const void *zs,
                       const void *gammas, int sfmt, int flags, void *ys_out, void *out_w, int ofmt);
/* Coefficient form: coeffs holds groups x t polynomials of n >= 1 coefficients each (the caller pads to the common length; stride n;
 * KZG_IN_DEVICE applies), n - 1 <= kzg_srs_len(srs).  ys_out[g t + i] = p_{g,i}(zs[g]) (kzg_poly_eval's values) and out_w[g] =
 * kzg_witness_coeff of the folded polynomial at (zs[g], F(zs[g])).  Group g runs on lane g mod lanes: values, fold, the linear quotient
 * of the folded coefficients, one MSM.  Outputs, errors and groups == 0 as above (n == 0 and n - 1 > kzg_srs_len(srs): KZG_ERR_SHAPE). */
int kzg_open_fold_coeff(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t t, size_t groups, const void *zs,
                        const void *gammas, int sfmt, int flags, void *ys_out, void *out_w, int ofmt);
/* ---- many polynomials at MANY points with one two-element proof (not a reference method) -----------------------------------------
 * N = count claims p_{m(k)}(z_k) = y_k, claim k naming polynomial m(k) = poly_idx[k] < n_polys (NULL: m(k) = k, count == n_polys
 * required) and any point z_k of Fr, are answered by the N values and TWO group elements, whatever N and however many distinct points:
 *   g(X) = sum_k r^k (p_{m(k)}(X) - y_k) / (X - z_k),   D = [g(tau)]_1                                  (first phase:  *_commit)
 *   w_k = r^k / (t - z_k),  W_m = sum_{m(k) = m} w_k,  v = sum_m W_m p_m - g,  pi = [(v - v(t)) / (X - t)]_1   (second phase: *_finish)
 * and v(t) = g2 = sum_k w_k y_k identically.  kzg_verify_multiopen (below) checks (D, pi): one pairing check.  The shape of PLONK-family
 * provers (openings at z, z w and beyond) and of Verkle-style / aggregate-blob provers (thousands of openings at points of the domain).
 * Against kzg_open_eval (one MSM and one witness per claim) and kzg_open_fold_* (one per distinct point) a call costs one streaming
 * pass per claim and ONE MSM per phase.
 * WHAT THE CALLER OWES.  r must be unpredictable to whoever chose the polynomials, points and values: a hash of the commitments, zs
 * and ys.  t MUST BE DRAWN AFTER D EXISTS: a hash that includes D.  With a t known in advance a single wrong claim (C, z, y') passes
 * without any knowledge of tau: take pi = the identity and D = (C - [y'] gs[0]) / (t - z).  This is why the prover is TWO calls: the
 * library has no hash.  The phases are stateless; the caller carries g (and may drop everything else) between them.  If t equals
 * some z_k the second phase and the verifier return KZG_ERR_SHAPE and the caller draws another t.
 * The linear combination alone: out[j] = sum_{k < count} weights[k] vecs[idx[k] d + j] for j < d (any d >= 1), idx[k] < n_vecs; weights:
 * host scalars below the modulus in sfmt.  vecs and out are host memory, or device memory with KZG_IN_DEVICE / KZG_OUT_DEVICE; out
 * has the form of the inputs; canonical inputs may hold any 256-bit value (they count as their residue).  Host vectors are staged in
 * pieces of at most 64 MiB with the running sum on the device.  Leases one lane.  count == 0: out is zeroed. */
int kzg_fr_lincomb(kzg_ctx *ctx, const void *vecs, size_t d, size_t n_vecs, const uint32_t *idx, const void *weights, size_t count, int sfmt,
                   int flags, void *out);
/* ---- scans over Fr, the grand product and batch inversion (not a reference method) -------------------------------------------------
 * The running product of a permutation argument and the running sum of a logUp-style lookup argument, without leaving the device.
 * Scalars are sfmt; in KZG_FR_CANONICAL_LE_32 any 256-bit word counts as its residue, in KZG_FR_MONT_LE_32 inputs are below r; outputs
 * are in sfmt and always below r.  Products are products of the represented values in both formats (Montgomery in: the Montgomery
 * form of the product out).  KZG_IN_DEVICE covers in / num / den, KZG_OUT_DEVICE covers out / z_out; totals, zeros and zero_den are
 * ALWAYS host memory.  Aliasing: for kzg_fr_scan and kzg_fr_batch_inverse out == in EXACTLY is allowed (on the device with both flags
 * set, and for two host buffers); any other overlap of an output with an input or with another output is the caller's error.
 * kzg_fr_grand_product's z_out overlaps neither num nor den.
 * All three are blocking calls that lease one lane (they run concurrently with each other and with the calls listed at the top).
 * Host inputs and outputs are staged in pieces of at most 64 MiB -- whole vectors for kzg_fr_scan (one vector if a vector is larger),
 * whole vectors' 2 t columns for kzg_fr_grand_product (one vector's columns if they are larger), any run of elements for
 * kzg_fr_batch_inverse --, and the vectors of a call are worked off in chunks of min(65535, max(1, 65536 / ceil(n / 2048))) vectors, three
 * kernel launches per chunk: the workspace does not grow with batch (Limits).
 * KZG_ERR_SHAPE, before any memory is touched: a NULL ctx, an unknown sfmt or op, exclusive not 0 or 1, n == 0, t == 0, a NULL input
 * or output with work to do, n > 2^28, batch x t x n x 32 beyond size_t.  batch == 0: KZG_OK, nothing touched.
 * Options, read per call, for tests; the bytes are the same: "fr_scan_tile" (0 = default, 2048; a power of two in 8..2048: the elements
 * one workgroup of kzg_fr_scan / kzg_fr_grand_product scans, 1..256 threads of eight -- tile and carry boundaries at n in the hundreds),
 * "fr_scan_stage" (0 = default, 64 MiB; a multiple of 32 up to 64 MiB: the bytes of one staged piece, all three calls) and
 * "fr_scan_chunk" (0 = the rule above alone; 1..65535: at most that many vectors per chunk). */
enum { KZG_SCAN_PRODUCT = 0, KZG_SCAN_SUM = 1 };

/* out[i] = 1 / in[i]; a zero (a word whose residue is 0) maps to zero.  *zeros (optional) = how many. */
int kzg_fr_batch_inverse(kzg_ctx *ctx, const void *in, size_t n, int sfmt, int flags, void *out, size_t *zeros);

/* `batch` vectors of n scalars, contiguous (vector b at element b*n).
 * exclusive = 0: out[b*n+i] = in[b*n+0] (op) ... (op) in[b*n+i]
 * exclusive = 1: out[b*n+0] = identity (1 for PRODUCT, 0 for SUM), out[b*n+i] = in[b*n+0] (op) ... (op) in[b*n+i-1]
 * totals (optional; batch scalars, ALWAYS host memory, sfmt): the (op) of all n elements of each vector. */
int kzg_fr_scan(kzg_ctx *ctx, const void *in, size_t n, size_t batch, int op, int exclusive, int sfmt, int flags,
                void *out, void *totals);

/* The permutation / lookup accumulator.  num, den: batch x t x n scalars each, column j of vector b at element (b*t + j)*n
 * (the layout of kzg_fr_fold).  With f_b[i] = prod_j num[b][j][i] / prod_j den[b][j][i]:
 *   z_out[b*n + 0] = 1,  z_out[b*n + i] = f_b[0] ... f_b[i-1]  (i < n),  totals[b] = f_b[0] ... f_b[n-1]  (1 for a valid permutation).
 * totals: optional, host.  zero_den: optional, batch ints, host.
 * A vector with a zero denominator (a den word whose residue is 0) has its row of z_out and its total written as all zero.  With
 * zero_den given, zero_den[b] = 1 for those vectors and 0 for the others, and the call returns KZG_OK; with zero_den == NULL the call
 * returns KZG_ERR_SHAPE if any vector has one (the reference's invert().unwrap() panic; the status argument of kzg_witness_coeff_many
 * is the model).  A zero in num is legal: z is zero from there on.  No element is inverted: one field inversion per vector. */
int kzg_fr_grand_product(kzg_ctx *ctx, const void *num, const void *den, size_t n, size_t t, size_t batch, int sfmt, int flags,
                         void *z_out, void *totals, int *zero_den);
/* ---- lookup arguments: multiplicities and the logUp column (not a reference method) -------------------------------------------------
 * The column that the running sum of a logUp-style lookup argument runs over, without leaving the device: the multiplicity of every
 * table row among the witness values, m_i = #{ j : w_j = t_i } -- a join of two vectors of field elements -- and the terms
 * sum_j 1 / (beta + w_j[i]) - m_i / (beta + t_i).  kzg_fr_scan(..., KZG_SCAN_SUM, exclusive = 1, ...) over the terms is then the logUp
 * accumulator, and its total is 0 for a valid lookup.  Tables of several columns are the caller's business: compress the rows (and the
 * witness tuples) into one column with kzg_fr_lincomb first.
 *
 * A kzg_lookup is a table of n_t scalars prepared for membership queries: the keys stored once, reduced, and an open-addressing hash
 * table of 64-bit slots (hash tag, table index) over them in HBM.  It is immutable after setup and may be queried by any number of
 * threads.  Keys are residues modulo r: in KZG_FR_CANONICAL_LE_32 any 256-bit word counts as its residue, in KZG_FR_MONT_LE_32 inputs
 * are below r; a plan set up in one format answers queries in the other.  The table may hold duplicates (a table padded to its domain
 * by repeating its last row): `distinct` is the number of different residues, and a residue's OWNER is the lowest index that holds it.
 *
 * kzg_lookup_setup: table = n_t scalars in sfmt, host memory or device memory with KZG_IN_DEVICE; 1 <= n_t <= 2^26.
 * kzg_lookup_shape: n_t, distinct and the bytes the plan holds in HBM (each optional).
 * kzg_lookup_count: `batch` vectors of n scalars, vector b at values + b n (n <= 2^28).  For vector b
 *   index_out[b n + j]   = the owner of values[b][j], or 0xFFFFFFFF if the value is not in the table;
 *   mult_out[b n_t + i]  = the number of j whose owner is i, as a field element in sfmt (0 at rows that own nothing);
 *   missing[b]           = the number of values that are not in the table;
 *   first_missing[b]     = the lowest such j, or SIZE_MAX if there is none.
 * Every output is a function of the inputs alone: two calls give the same bytes.  Each of the four is optional, not all NULL.
 * KZG_IN_DEVICE covers table / values, KZG_OUT_DEVICE covers mult_out / index_out; missing / first_missing are ALWAYS host memory.
 * With missing or first_missing given, values outside the table are reported there and the call returns KZG_OK; with both NULL the call
 * returns KZG_ERR_SHAPE when any value is missing (the zero_den == NULL rule of kzg_fr_grand_product) -- the other outputs are still
 * written in full.
 * KZG_ERR_SHAPE, before any memory is touched: a NULL ctx or plan, an unknown sfmt, n_t == 0, n == 0 with batch > 0, n_t > 2^26,
 * n > 2^28, batch x n x 32 or batch x n_t x 32 beyond size_t, a NULL table / out / values, every output NULL, a plan of another GPU.
 * batch == 0: KZG_OK, nothing touched.  KZG_ERR_INTERNAL: the build found no free slot (every probe loop is bounded by the slot count).
 * Setup and count are blocking calls that lease one lane (they run concurrently with the calls listed at the top).  Host data is staged
 * in pieces of at most 64 MiB (option "lookup_stage"), and the vectors are worked off in chunks of min(65535, max(1, 2^24 / n_t)) (option
 * "lookup_chunk"): the workspace does not grow with batch (Limits).  Options "lookup_spare_log" and "lookup_hash_bits" shape the slot
 * array at setup, for tests; the bytes are the same under every setting. */
typedef struct kzg_lookup kzg_lookup;
int kzg_lookup_setup(kzg_ctx *ctx, const void *table, size_t n_t, int sfmt, int flags, kzg_lookup **out);
void kzg_lookup_free(kzg_ctx *ctx, kzg_lookup *plan);
int kzg_lookup_shape(const kzg_lookup *plan, size_t *n_t, size_t *distinct, size_t *bytes);
int kzg_lookup_count(kzg_ctx *ctx, const kzg_lookup *plan, const void *values, size_t n, size_t batch, int sfmt, int flags,
                     void *mult_out, uint32_t *index_out, size_t *missing, size_t *first_missing);
/* values: batch x t x n scalars, column j of vector b at element (b*t + j)*n (the layout of kzg_fr_fold); table: n scalars shared by all
 * vectors; mult: batch x n scalars; beta: one host scalar in sfmt, below r.
 *   out[b*n + i] = sum_{j < t} 1 / (beta + values[b][j][i]) - mult[b][i] / (beta + table[i])
 * table and mult may both be NULL (only the sum), t may be 0 when they are given (only the second term); both absent, or one of the
 * two without the other, is KZG_ERR_SHAPE.  KZG_IN_DEVICE covers values / table / mult, KZG_OUT_DEVICE covers out, which overlaps no
 * input; formats and residues as for kzg_fr_grand_product.  A vector with a zero denominator (beta = -x somewhere in its columns or
 * in the table) has its row of out written as all zero; with zero_den given (batch ints, host) zero_den[b] = 1 for those vectors and
 * 0 for the others and the call returns KZG_OK; with zero_den == NULL the call returns KZG_ERR_SHAPE if any vector has one.  No element is
 * inverted on its own (Montgomery's trick, 16 denominators per inversion).  n <= 2^28, any t and batch; KZG_ERR_SHAPE, before any memory
 * is touched, as for kzg_fr_grand_product (n == 0, an unknown sfmt, beta not below r, sizes beyond size_t); batch == 0: KZG_OK.  Leases
 * one lane; works in chunks of at most 2^21 denominators (Limits). */
int kzg_logup_terms(kzg_ctx *ctx, const void *values, const void *table, const void *mult, const void *beta, size_t n, size_t t, size_t batch,
                    int sfmt, int flags, void *out, int *zero_den);
/* ---- constraint expressions over columns in one pass (not a reference method) -----------------------------------------------------
 * The quotient round of a PLONK-family prover evaluates its gate, permutation and lookup constraints row by row on the extended
 * coset: polynomial expressions in the columns and in rotations of them.  A kzg_fr_program is a small straight-line program over Fr,
 * validated once and kept; kzg_fr_program_run runs it for every row i < n of a set of columns in ONE pass over HBM: each column
 * element an instruction names is read once, each output written once, the temporaries never leave the chip.  With it the sequence
 * coset transforms -> constraints -> 1 / Z_H -> inverse coset transform -> commit stays in device memory.
 *
 * An instruction is KZG_FRP_WORDS = 6 uint32_t words:
 *   word 0      op | dst_kind << 8 | a_kind << 16 | b_kind << 24
 *   words 1..3  the indices dst, a, b
 *   words 4, 5  the shifts of a and b, two's-complement int32_t; meaningful for KZG_FRP_COL operands, 0 otherwise
 * and means, for row i, dst = a (op) b with op one of KZG_FRP_ADD / _SUB / _MUL.  Operands:
 *   KZG_FRP_COL c, shift s   element (i + s) mod col_len[c] of cols[c]
 *   KZG_FRP_CONST k          consts[k]: n_consts host scalars below r in sfmt, one set per run (the challenges; a plan is reused
 *                            across proofs)
 *   KZG_FRP_TEMP t           a per-row temporary, t < KZG_FRP_MAX_TEMPS = 16; read only after an earlier instruction wrote it
 * Destinations: KZG_FRP_TEMP t (may equal a source) or KZG_FRP_OUT o, outs[o][i]: write-only, every output written by exactly one
 * instruction of the program.
 * Columns: col_len[c] is n (any n) or a power of two that divides n: a short column is periodic (the e values of 1 / Z_H on an e-fold
 * extended coset are one column of length e).  A rotation by one row of the base domain on an e-fold extended domain is shift = e:
 * the caller's arithmetic.  Any int32_t is a legal shift; no row performs a division.
 * Formats are those of kzg_fr_scan: in KZG_FR_CANONICAL_LE_32 any 256-bit column word counts as its residue, in KZG_FR_MONT_LE_32
 * column words are below r; outputs are in sfmt and below r; a product is the product of the represented values in both formats
 * (Montgomery form is the fast path: canonical data pays one conversion per column load and one per store).  KZG_IN_DEVICE covers
 * every cols[c], KZG_OUT_DEVICE every outs[o]; the arrays cols, col_len, outs themselves and consts are ALWAYS host memory.  Host
 * columns are uploaded whole, once each (Limits).  An output overlaps no column and no other output -- rotations make in-place
 * evaluation a race --: pointer equality is rejected, any other overlap is the caller's error.
 * kzg_fr_program_shape: the sizes given at setup, the temporaries in use (highest index + 1) and the number of KZG_FRP_MUL
 * instructions; every out-pointer is optional.
 * KZG_ERR_SHAPE, before any memory is touched -- at setup (*out is left as it was): a NULL ctx, words or out; n_insns == 0 or above
 * 65,536, n_cols or n_consts above 4,096, n_out == 0 or above 64; an unknown op or kind; KZG_FRP_OUT as a source, KZG_FRP_COL / _CONST as
 * a destination; an index out of range, a temporary index >= 16; a temporary read before any instruction wrote it; a non-zero shift on
 * an operand that is no column; an output written twice or never.  At run: a NULL plan, a plan of another GPU, n == 0 or n > 2^28, an
 * unknown sfmt, a col_len that is 0 or neither n nor a power of two dividing n, a const not below r, a NULL cols / col_len (n_cols > 0),
 * consts (n_consts > 0) or outs, a NULL pointer among the columns or outputs, an output equal to a column or to another output.
 * The run is a blocking call that leases one lane (it runs concurrently with the calls listed at the top); setup and shape touch no GPU.
 * A plan is immutable and may be run by any number of threads.  Option "fr_program_block" picks the workgroup size, for tests. */
typedef struct kzg_fr_program kzg_fr_program;
enum { KZG_FRP_ADD = 0, KZG_FRP_SUB = 1, KZG_FRP_MUL = 2 };                       /* op */
enum { KZG_FRP_COL = 0, KZG_FRP_CONST = 1, KZG_FRP_TEMP = 2, KZG_FRP_OUT = 3 };  /* operand / destination kinds */
enum { KZG_FRP_WORDS = 6, KZG_FRP_MAX_TEMPS = 16 };
int kzg_fr_program_setup(kzg_ctx *ctx, const uint32_t *words, size_t n_insns, size_t n_cols, size_t n_consts, size_t n_out,
                         kzg_fr_program **out);
void kzg_fr_program_free(kzg_ctx *ctx, kzg_fr_program *plan);
int kzg_fr_program_shape(const kzg_fr_program *plan, size_t *n_insns, size_t *n_cols, size_t *n_consts, size_t *n_out, size_t *n_temps,
                         size_t *n_mul);
int kzg_fr_program_run(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const size_t *col_len, const void *consts,
                       size_t n, int sfmt, int flags, void *const *outs);
/* ---- sumcheck rounds on the device: multilinear tables (not reference methods) --------------------------------------------------------
 * The provers that commit to a table of 2^m values with kzg_commit_coeff over the table itself and open it with HyperKZG / Gemini or
 * Zeromorph -- HyperPlonk-style gate checks, Spartan, logUp-GKR -- spend their time in m rounds of: evaluate a constraint expression on
 * every pair of rows at X = 0 .. D and add everything up; draw a challenge; fold every column with it.  The plan of the constraint is a
 * kzg_fr_program (above); these calls run it on pairs, fold, build the eq table and evaluate.  Everything is Fr-only and bit-exact.
 *
 * Conventions
 *   - a multilinear polynomial in m variables is a table f of n = 2^m scalars; f[i] is its value at the corner whose coordinate x_j is
 *     bit j of i.
 *   - rounds bind the TOP variable: with h = n / 2, lo = f[0, h) is x_{m-1} = 0 and hi = f[h, n) is x_{m-1} = 1; binding to rho gives
 *     lo[i] + rho (hi[i] - lo[i]) in h elements.  That runs in place: lane i reads i and i + h and writes i.
 *   - a point is m scalars, point[j] for variable j.  Round k of a sumcheck therefore fixes point[m - 1 - k].
 *   - formats and residues are those of kzg_fr_scan: in KZG_FR_CANONICAL_LE_32 any 256-bit data word counts as its residue, in
 *     KZG_FR_MONT_LE_32 data is below r; outputs are in sfmt and below r; a product is the product of the represented values in both.
 *   - single scalars (point, rho, consts) are host memory and below r, else KZG_ERR_SHAPE.
 *
 * kzg_mle_eq: out[i] = prod_{j < m} (bit_j(i) ? point[j] : 1 - point[j]), 2^m scalars, 0 <= m <= 28 (m = 0: out[0] = 1).  KZG_OUT_DEVICE
 *   covers out.  Built by doubling, t[i + 2^j] = t[i] u_j then t[i] -= t[i + 2^j]: one product per output element, not m.  The first 10
 *   levels run inside one workgroup's LDS (option "mle_local_log"), the rest level by level.
 * kzg_mle_bind: for every column c < n_cols and i < n / 2, outs[c][i] = cols[c][i] + rho (cols[c][i + n / 2] - cols[c][i]).  n a power of
 *   two, 2 <= n <= 2^28; 1 <= n_cols <= 4,096; all columns in one launch.  outs[c] == cols[c] EXACTLY is allowed: in place, the upper half
 *   left byte for byte as it was.  Otherwise outs[c] is a buffer of n / 2 scalars that overlaps no column and no other output: the
 *   ranges are known, so any overlap is rejected (columns and outputs in different memories -- one of the two flags -- cannot meet; the
 *   outputs are still compared with each other).  KZG_IN_DEVICE covers the columns, KZG_OUT_DEVICE the outputs; the pointer arrays are
 *   host memory.  Host columns are uploaded whole.
 * kzg_mle_eval: ys_out[b] = f_b(point) for `batch` tables, table b at element b 2^m; ys_out is ALWAYS host memory.  Binds from the top
 *   variable down; the inputs are never written (the first level goes into the lane's workspace).  quotients_out (optional, follows
 *   KZG_OUT_DEVICE): batch x (n - 1) scalars; for table b the 2^k values of q_k = hi - lo at the level where variable k is bound sit at
 *   element b (n - 1) + 2^k - 1.  These are the Zeromorph quotients, f(X) - f(u) = sum_k (X_k - u_k) q_k(X_0 .. X_{k-1}); committing to
 *   them is kzg_commit_coeff.  0 <= m <= 28; KZG_IN_DEVICE covers tables.  batch == 0: KZG_OK, nothing touched.
 * kzg_fr_program_degree: degrees[o], o < n_out: an upper bound of the total degree of output o in the columns -- a const counts 0, a
 *   column 1, add / sub the maximum, mul the sum, saturating at 2^32 - 1.  Host only.  A sumcheck needs n_eval = degree + 1.
 * kzg_sumcheck_round: with h = n / 2 and v_c(i, X) = cols[c][i] + X (cols[c][i + h] - cols[c][i]), for X = 0 .. n_eval - 1 and every
 *   output o of the plan: sums_out[o n_eval + X] = sum_{i < h} P_o(v_0(i, X), ..., v_{C-1}(i, X); consts).  sums_out is ALWAYS host
 *   memory, in sfmt, below r.  Every column has n elements, n a power of two, 2 <= n <= 2^28; KZG_IN_DEVICE covers the columns, the
 *   array cols and consts are host memory.  Each column element comes from HBM once per round; the sum is deterministic (no atomics).
 * KZG_ERR_SHAPE, before any memory is touched: a NULL ctx; an unknown sfmt; m > 28; n no power of two or outside 2 .. 2^28; n_cols
 * outside 1 .. 4,096; a point coordinate, rho or const not below r; NULL pointers (arrays, their entries, point with m > 0, rho,
 * consts with n_consts > 0, out, ys_out, sums_out, degrees, the plan); an output of kzg_mle_bind that overlaps; for the round a plan
 * with a non-zero shift (a rotation has no meaning on the hypercube), n_eval outside 1 .. 16, n_out x n_eval > 32, a plan of another GPU.
 * All but kzg_fr_program_degree are blocking calls that lease one lane (they run concurrently with the calls listed at the top).
 * Options, read per call, the same bytes under every setting: "sumcheck_block", "sumcheck_grid", "mle_block", "mle_local_log",
 * "mle_eval_chunk" (kzg_ctx_set_option). */
enum { KZG_SUMCHECK_MAX_EVAL = 16, KZG_SUMCHECK_MAX_ACC = 32 };
int kzg_mle_eq(kzg_ctx *ctx, const void *point, size_t m, int sfmt, int flags, void *out);
int kzg_mle_bind(kzg_ctx *ctx, const void *const *cols, size_t n_cols, size_t n, const void *rho, int sfmt, int flags, void *const *outs);
int kzg_mle_eval(kzg_ctx *ctx, const void *tables, size_t m, size_t batch, const void *point, int sfmt, int flags, void *ys_out,
                 void *quotients_out);
int kzg_fr_program_degree(const kzg_fr_program *plan, size_t *degrees);
int kzg_sumcheck_round(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const void *consts, size_t n, size_t n_eval,
                       int sfmt, int flags, void *sums_out);
/* Evaluation form: evals holds n_polys vectors of d values (stride d), d a power of two == kzg_srs_len(lagrange).  First phase:
 * ys_out[k] = p_{m(k)}(z_k) (host, count scalars: the values of kzg_eval_form_eval), g_out = the d values of g on the domain, D at out_d
 * in ofmt (each of the three optional, not all NULL).  evals and g / g_out are host memory, or device memory with KZG_IN_DEVICE; g has the
 * form (canonical or Montgomery) of the inputs; D and pi follow KZG_OUT_DEVICE; zs, r, t, ys_out and y_out are host memory.  Second
 * phase: the same claims and r, the t drawn from D, g as the first phase left it; pi at out_pi and v(t) at y_out (optional; a caller
 * may check v(t) == g2).  Both take the context exclusively and run ONE MSM each.  The claims are sorted by point on the host; distinct
 * points off the domain are worked off in chunks of at most min(16, 2^22 / d) (option "multiopen_points_chunk": 0 = that, 1..16 lowers
 * it): per chunk the denominators w^i - z_u are inverted once per distinct point, the chunk's values are formed, and ONE pass
 * (k_multiopen_accum) adds the chunk's share to g in device memory -- no quotient and no combined polynomial is written.  Points
 * w^m of the domain take the materialised route one by one (combination, the quotient of kzg_quotient_eval, an add into g).
 * Limits: host polynomials are uploaded once, whole, per call (both phases read them at random through the indices): n_polys x d x 32
 * bytes of workspace, KZG_ERR_ALLOC if that does not fit -- callers with large sets keep them resident (KZG_IN_DEVICE).  Beyond that:
 * g, per chunk 2 x min(16, 2^22 / d) x d scalars, 72 bytes per claim, one MSM workspace.
 * KZG_ERR_SHAPE, before memory is touched: d not a power of two or != kzg_srs_len(lagrange), a z, r or t >= modulus, r == 0, t equal to a
 * z_k, an index >= n_polys, NULL indices with count != n_polys, an unknown format, a NULL pointer with count > 0, an SRS on another
 * GPU.  count == 0: g_out is zeroed, D and pi are the identity, KZG_OK. */
int kzg_multiopen_eval_commit(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t n_polys, const uint32_t *poly_idx,
                              const void *zs, size_t count, const void *r, int sfmt, int flags, void *ys_out, void *g_out, void *out_d, int ofmt);
int kzg_multiopen_eval_finish(kzg_ctx *ctx, const kzg_srs *lagrange, const void *evals, size_t d, size_t n_polys, const uint32_t *poly_idx,
                              const void *zs, size_t count, const void *r, const void *t, const void *g, int sfmt, int flags, void *y_out,
                              void *out_pi, int ofmt);
/* Coefficient form: coeffs holds n_polys polynomials of n >= 1 coefficients each (the caller pads to the common length; stride n),
 * n - 1 <= kzg_srs_len(srs); g has n - 1 coefficients.  Values from kzg_poly_eval's stage per claim, per distinct point the combination
 * (k_fr_lincomb) and the linear quotient of kzg_quotient_linear accumulated into g, one MSM of n - 1 scalars; the second phase is the
 * combination minus g, the linear quotient at t, one MSM.  Outputs, flags, errors and count == 0 as above (n == 0, n - 1 >
 * kzg_srs_len(srs): KZG_ERR_SHAPE). */
int kzg_multiopen_coeff_commit(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t n_polys, const uint32_t *poly_idx,
                               const void *zs, size_t count, const void *r, int sfmt, int flags, void *ys_out, void *g_out, void *out_d, int ofmt);
int kzg_multiopen_coeff_finish(kzg_ctx *ctx, const kzg_srs *srs, const void *coeffs, size_t n, size_t n_polys, const uint32_t *poly_idx,
                               const void *zs, size_t count, const void *r, const void *t, const void *g, int sfmt, int flags, void *y_out,
                               void *out_pi, int ofmt);
/* ---- all openings over the domain (FK20, single-point case; not a reference method) ---------------------------------
 * Every witness of a polynomial at every point w^m of its size-N domain (w = compute_omega(N).omega) in O(N log N) group
 * operations instead of N MSMs: two G1 DFTs, 2N variable-base scalar multiplications and one Fr NTT per polynomial, against a
 * plan that holds DFT_2N of the reversed monomial SRS.  Witness m equals kzg_witness_coeff_many at (w^m, p(w^m)) and
 * KZGProverEvalForm::create_witness(evals, m) (src/eval_form.rs:124-140) when the Lagrange SRS comes from the same tau.
 * A kzg_fk20 holds that transform and the twiddle tables for one monomial SRS and one domain 2^log_n; it is immutable after
 * creation and may be used from any thread and every kzg_ctx on its device.  Setup: KZG_ERR_DEGREE_TOO_LARGE if log_n + 1 reaches
 * the two-adicity of Fr, KZG_ERR_SHAPE for log_n > 22 (Limits) or an SRS on another GPU.  SRS points past len(srs) count as the
 * identity, which is exact for every polynomial the calls below accept. */
typedef struct kzg_fk20 kzg_fk20;
int kzg_fk20_setup(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, kzg_fk20 **out);
void kzg_fk20_free(kzg_ctx *ctx, kzg_fk20 *plan);
size_t kzg_fk20_domain(const kzg_fk20 *plan); /* N */
/* `batch` polynomials of n coefficients each (stride n); out: batch x N witnesses, witness m of polynomial b at w^m.  KZG_ERR_SHAPE
 * if n == 0, n > N, n - 1 > len(srs) (the reference's slice panic) or the plan lives on another GPU.  N == 1: the identity.  Takes
 * the context exclusively; works in chunks of at most 2^21 / 2N polynomials, so the workspace does not grow with `batch`. */
int kzg_witness_all_coeff(kzg_ctx *ctx, const kzg_fk20 *plan, const void *coeffs, size_t n, size_t batch, int sfmt, int flags,
                          void *out, int ofmt);
/* `batch` evaluation vectors of length d == N (else KZG_ERR_SHAPE): iNTT in Fr, then the above; witness m ==
 * KZGProverEvalForm::create_witness(evals, m). */
int kzg_witness_all_eval(kzg_ctx *ctx, const kzg_fk20 *plan, const void *evals, size_t d, size_t batch, int sfmt, int flags,
                         void *out, int ofmt);
/* ---- all coset openings over the domain (FK20, multi-point case; not a reference method) -------------------------------
 * The domain of N = 2^log_n points split into K = N / l cosets of l = 2^log_l points: C_i = { w^(i + tK) : t < l }, i < K, with
 * vanishing polynomial X^l - w^(il).  One call computes, for every coset, what create_witness_batched(p, C_i, p(C_i))
 * (src/coeff_form.rs:83-111, kzg_witness_coeff_batched) returns: w = [(p - I_i) / (X^l - w^(il))]_1 and r = I_i, in O(N log N)
 * group operations instead of K MSMs.  Per polynomial: 2l Fr NTTs of sizes 2K and K, one l-term linear combination of G1
 * points at each of 2K frequencies (2N scalar multiplications sharing one doubling chain per frequency), an inverse G1 DFT of
 * size 2K and a forward one of size K.  The witness bytes equal kzg_witness_coeff_batched's in every format; r equals its l
 * interpolant scalars (for n <= l: the witness is the identity and r is p zero-padded, as there).
 * A kzg_fk20_cosets holds, for one monomial SRS, one domain and one coset size, the multiples 1..8 of DFT_2K of the l residue
 * classes of the reversed SRS in affine form (8 x 2N rows of 128 B: 2.1 GB at 2^20) and the twiddle tables; it is immutable
 * after creation and may be used from any thread and every kzg_ctx on its device.  Setup: KZG_ERR_DEGREE_TOO_LARGE if
 * log_n + 1 reaches the two-adicity of Fr; KZG_ERR_SHAPE for log_n > 22 (Limits), log_l == 0 (single points: kzg_fk20_setup),
 * log_l > log_n or an SRS on another GPU.  SRS points past len(srs) count as the identity, exact for every accepted polynomial. */
typedef struct kzg_fk20_cosets kzg_fk20_cosets;
int kzg_fk20_cosets_setup(kzg_ctx *ctx, const kzg_srs *monomial, uint32_t log_n, uint32_t log_l, kzg_fk20_cosets **out);
void kzg_fk20_cosets_free(kzg_ctx *ctx, kzg_fk20_cosets *plan);
/* *domain = N, *coset_size = l (either may be NULL); KZG_ERR_SHAPE for a NULL plan */
int kzg_fk20_cosets_shape(const kzg_fk20_cosets *plan, size_t *domain, size_t *coset_size);
/* `batch` polynomials of n coefficients each (stride n).  out_w: batch x K points in ofmt, witness i of polynomial b at index
 * b K + i, opening C_i (cosets in natural order).  out_r (optional, NULL skips it): batch x K x l scalars in sfmt, coset i's
 * interpolant coefficients r_0 .. r_{l-1} at (b K + i) l.  KZG_IN_DEVICE applies to the input, KZG_OUT_DEVICE to both outputs.
 * KZG_ERR_SHAPE if n == 0, n > N, n > l with n - l > len(srs) (the reference's slice panic), an unknown format, a NULL pointer or
 * a plan on another GPU; batch == 0 returns KZG_OK.  Takes the context exclusively; works in chunks of at most 2^21 / 2N
 * polynomials, so the workspace does not grow with `batch`. */
int kzg_witness_cosets_coeff(kzg_ctx *ctx, const kzg_fk20_cosets *plan, const void *coeffs, size_t n, size_t batch, int sfmt,
                             int flags, void *out_w, int ofmt, void *out_r);
/* `batch` evaluation vectors of length d == N (else KZG_ERR_SHAPE), natural domain order: iNTT in Fr, then the above */
int kzg_witness_cosets_eval(kzg_ctx *ctx, const kzg_fk20_cosets *plan, const void *evals, size_t d, size_t batch, int sfmt,
                            int flags, void *out_w, int ofmt, void *out_r);
/* ---- recovery from a subset of the cosets (erasure recovery; Fr only, no SRS; not a reference method) ------------------------
 * The other half of the coset calls above: a polynomial of at most n coefficients from ANY `known` of the K = N / l cosets of
 * its size-N domain (N = 2^log_n, l = 2^log_l) with known * l >= n.  coset_ids: `known` distinct ids < K in any order (host
 * memory, always).  cells: batch x known x l scalars in sfmt, cell j of polynomial b at (b known + j) l, holding
 * p_b(w^(id_j + t K)) for t = 0 .. l-1 (the point order of the coset calls); KZG_IN_DEVICE applies to it.  out_coeffs
 * (optional): batch x n scalars, stride n -- what kzg_witness_cosets_coeff takes.  out_evals (optional): batch x N scalars in
 * natural domain order -- what kzg_witness_cosets_eval takes; the known cells come back bit-identical.  At least one output;
 * KZG_OUT_DEVICE applies to both, both are in sfmt.  status (optional, host, batch ints): 0 = recovered, 1 = the cells of that
 * polynomial are not the values of a polynomial of fewer than n coefficients (detectable iff known * l > n); the call then
 * returns KZG_OK and a failed polynomial's outputs are unspecified but stay inside their slots.  Without status any such
 * polynomial makes the call return KZG_ERR_POINT_NOT_ON_POLY (the convention of kzg_witness_coeff_many).
 * With M the missing ids, nu = w^l and Zs(Y) = prod_{i in M} (Y - nu^i): the cells times Zs(nu^id) are the values of
 * p(X) Zs(X^l), of degree < N; one iNTT, a division by Zs(X^l) on the coset 7 H (where it has no root) and the transform
 * back give p: three size-N transforms per polynomial (four with out_evals).  Zs is built once per call by a product tree in
 * O(m log^2 m) (leaves of 256 roots), its K values and K inverses by two size-K transforms and one batch inversion.
 * KZG_ERR_SHAPE, before any memory is touched: log_l > log_n, log_n > 22 (the FK20 plans' limit), n == 0, n > N, known == 0,
 * known > K, known * l < n, an id >= K, a duplicate id, NULL coset_ids or cells, both outputs NULL, an unknown scalar format.
 * batch == 0 returns KZG_OK.  Leases one lane like the other blocking calls (concurrent callers run side by side); works in
 * chunks of at most max(1, 2^21 / 2N) polynomials (the rule of the FK20 calls), so the workspace does not grow with `batch`. */
int kzg_recover_cosets(kzg_ctx *ctx, uint32_t log_n, uint32_t log_l, size_t n, const size_t *coset_ids, size_t known,
                       const void *cells, size_t batch, int sfmt, int flags, void *out_coeffs, void *out_evals, int *status);
/* KZGVerifierEvalForm::verify_poly (:162-171): ifft then monomial MSM, compare. */
int kzg_verify_poly_eval(kzg_ctx *ctx, const kzg_srs *monomial, const void *commitment, int pfmt,
                         const void *evals, size_t d, int sfmt, int flags, int *ok);

/* ---- verifier: G2 parameters and pairing checks (src/coeff_form.rs:126-182, src/eval_form.rs:173-217) ----
 * The reference runs these on the CPU through blstrs' pairing(); here one GPU thread evaluates one check
 * (shared Miller loop over both pairs + one final exponentiation), so `count` openings verify in one launch.
 * Host-resident inputs only; commitments / witnesses in an affine G1 format (KZGCommitment = G1Affine). */
/* setup(), G2 half (src/lib.rs:48-52): hs[i] = [s^i] H for i < n. */
int kzg_srs_setup_g2(kzg_ctx *ctx, const void *s, int sfmt, size_t n, kzg_srs_g2 **out);
/* [L_i(s)] H over the size-d domain (lagrange_basis_h of KZGVerifierEvalForm::new, src/eval_form.rs:150). */
int kzg_srs_setup_lagrange_g2(kzg_ctx *ctx, const void *s, int sfmt, size_t d, kzg_srs_g2 **out);
/* compute_lagrange_basis, G2 half, from hs alone (src/eval_form.rs:254-280); d = len(hs) a power of two <= 2^20 (KZG_ERR_SHAPE
 * otherwise).  Below option "g2_lagrange_dft_from" (default 2048) every row is one d-term G2 sum (d^2 scalar multiplications); from it
 * on the basis is the G2 inverse DFT of hs (kzg_ntt_g2's kernels).  Both paths give the same group elements, so the same bytes. */
int kzg_srs_lagrange_from_monomial_g2(kzg_ctx *ctx, const kzg_srs_g2 *hs, kzg_srs_g2 **out);
/* KZGParams.hs supplied by the caller (Vec<G2Projective> = KZG_G2_JACOBIAN_MONT_288, or any G2 format);
 * KZG_ERR_BAD_POINT if a point does not decode / is not on the twist. */
int kzg_srs_upload_g2(kzg_ctx *ctx, const void *pts, size_t n, int pfmt, kzg_srs_g2 **out);
int kzg_srs_download_g2(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, size_t n, void *out, int pfmt);
size_t kzg_srs_g2_len(const kzg_srs_g2 *srs);
void kzg_srs_g2_free(kzg_ctx *ctx, kzg_srs_g2 *srs);
/* G2Projective::multi_exp (call site src/coeff_form.rs:156): sum scalars[i] * srs[offset+i]; meant for the
 * verifier's small n (one thread per term). */
int kzg_msm_g2(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, const void *scalars, size_t n, int sfmt, void *out,
               int ofmt);
/* The same sum by the bucket method, for large n (not a reference method; the G2 counterpart of the variable-base sum behind
 * kzg_verify_cosets_batch): signed 8-bit windows, slices of S points (option "g2_msm_slice") sorted by |digit| in LDS, one owner
 * thread per (slice slot, window, bucket) adding its list with mixed additions, chunk after chunk of "g2_msm_slots" x S points into
 * one arena of fixed size; then the slots are folded, every window reduced by a suffix scan and a tree sum, and one Horner chain over
 * the 32 windows ends in an affine point on the device.  A term costs 32 mixed additions instead of ~380 point operations.  The
 * result is a group element, so `out` holds the bytes kzg_msm_g2 writes for the same inputs, in any KZG_G2_* format.  scalars: host,
 * or device with KZG_IN_DEVICE, in either format; a canonical value >= r counts as its residue.  n == 0 gives the identity.
 * KZG_ERR_SHAPE before `out` is touched: the range exceeds the SRS, an unknown format, a NULL argument, an SRS of another GPU.  Takes
 * the context exclusively, like the other verifier-side calls.  DESIGN.md section 3.6b says from which n on it is the faster call. */
int kzg_msm_g2_bucket(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, const void *scalars, size_t n, int sfmt, int flags,
                      void *out, int ofmt);
/* ok[c] = (prod_{i < pairs_per_check} e(g1[c*ppc + i], g2[c*ppc + i]) == 1), 1 <= pairs_per_check <= 4. */
int kzg_pairing_check(kzg_ctx *ctx, const void *g1_points, int pfmt1, const void *g2_points, int pfmt2,
                      size_t pairs_per_check, size_t checks, uint8_t *ok);
/* KZGVerifier::verify_eval (src/coeff_form.rs:126-142) for `count` independent (x, y, commitment, witness)
 * tuples: ok[c] = e(w_c, hs[1] - [x_c]hs[0]) == e(C_c - [y_c]gs[0], hs[0]).  KZGVerifierEvalForm::verify_eval
 * (src/eval_form.rs:173-190) is the same check at x = omega^i.  KZG_ERR_SHAPE if hs has fewer than 2 points. */
int kzg_verify_eval(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt,
                    const void *commitments, const void *witnesses, int pfmt, size_t count, uint8_t *ok);
/* KZGVerifier::verify_eval_batched (src/coeff_form.rs:144-182): z = prod (X - xs[i]), hz = MSM(hs, z),
 * gr = MSM(gs, r) with r = witness.r (r_len = num_coeffs), *ok = e(w, hz) == e(C - gr, hs[0]).
 * KZG_ERR_SHAPE if k + 1 > len(hs) or r_len > len(gs) (slice index panics), k = 0, or k > 16384. */
int kzg_verify_eval_batched(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, size_t k,
                            const void *r_coeffs, size_t r_len, int sfmt, const void *commitment, const void *witness,
                            int pfmt, int *ok);
struct kzg_point_tree; /* (the typedef is with kzg_point_tree_setup below) */
/* KZGProver::create_witness_batched (src/coeff_form.rs:83-111) for callers who hold a kzg_point_tree of the opening points, without that
 * call's bound of 16384 points: `batch` polynomials (coeffs: batch x n scalars, stride n) opened at the plan's k points.  With M the
 * plan's product and p_b = q_b M + r_b, deg r_b < k:  out_w[b] = [q_b]_1 in ofmt;  out_r[b k + j] (optional) = coefficient j of r_b, the
 * interpolant through (x_i, p_b(x_i)), zero-padded to k scalars in sfmt.  KZG_IN_DEVICE applies to coeffs and ys, KZG_OUT_DEVICE to out_w
 * and out_r.  M stays on the device; quotient and remainder come from the division stages of kzg_poly_divide with the power-series
 * inverse of rev(M) computed once per call; the quotients of a chunk of min(16, max(1, 2^24 / max(n, K))) polynomials go to the batched
 * MSM pipeline without leaving HBM, so the workspace (allocated and freed by the call) does not grow with batch.
 * ys (optional, batch x k claimed values): the claim of polynomial b holds iff r_b equals the tree interpolation of ys_b, compared on
 * the device; status (optional, batch ints) receives 0 or KZG_ERR_POINT_NOT_ON_POLY per polynomial and the call returns KZG_OK; without
 * status the call returns KZG_ERR_POINT_NOT_ON_POLY if any claim fails.  Every witness and every remainder is still written (the rule
 * of kzg_witness_coeff_many).  n <= k: the witness is the identity and r is p zero-padded.  k == 1: r is the constant p(x_0) (the
 * reference's X + (y - x) is for the mirrors, as for kzg_point_tree_interpolate).
 * KZG_ERR_SHAPE before any output is written: n == 0, n > 2^27, n - k > kzg_srs_len(srs), a plan with repeated points, a plan or an
 * SRS of another GPU, a NULL srs, plan, coeffs or out_w, an unknown format.  batch == 0: KZG_OK.  out_w and out_r hold the bytes of
 * kzg_witness_coeff_batched for every (p, xs) that call accepts with k >= 2.  The Fr stage of a chunk takes the context exclusively. */
int kzg_witness_coeff_tree(kzg_ctx *ctx, const kzg_srs *srs, const struct kzg_point_tree *plan, const void *coeffs, size_t n, size_t batch,
                           const void *ys, int sfmt, int flags, void *out_w, int ofmt, void *out_r, int *status);
/* The check of kzg_verify_eval_batched for callers who hold a kzg_point_tree of the opening points (kzg_point_tree_setup), without that
 * call's bound of 16384 points: `count` openings at ONE point set, tuple c = (commitments[c], witnesses[c], r_c) with r_c =
 * r_coeffs[c k .. c k + k), the remainder zero-padded to the plan's k coefficients.  hz = [M(tau)]_2 = MSM(hs[0 .. k], M) from the plan's
 * product by the bucket method of kzg_msm_g2_bucket, ONCE per call and on the device; gr_c = MSM(gs[0 .. k), r_c), the `count` sums one
 * after the other on one stream, each remainder staged from host memory (the pairing checks then run side by side);
 * ok[c] = e(w_c, hz) == e(C_c - gr_c, hs[0]), one GPU thread per check.  All inputs in host memory; points are validated as in
 * kzg_verify_eval (KZG_ERR_BAD_POINT, ok untouched).  KZG_ERR_SHAPE: k + 1 > len(hs), k > len(gs), a NULL buffer (also at count == 0), a
 * Jacobian point format, an unknown format, a plan with repeated points, a plan or an SRS of another GPU.  For k <= 16384 the verdicts are
 * those of kzg_verify_eval_batched on the same inputs.  Takes the context exclusively. */
int kzg_verify_eval_tree(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const struct kzg_point_tree *plan, const void *r_coeffs, int sfmt,
                         const void *commitments, const void *witnesses, int pfmt, size_t count, uint8_t *ok);
/* KZGVerifierEvalForm::verify_eval_all (src/eval_form.rs:192-217) exactly as written there. */
int kzg_verify_eval_all(kzg_ctx *ctx, const kzg_srs *lagrange_g, const kzg_srs_g2 *lagrange_h, const kzg_srs_g2 *hs,
                        const void *ys, size_t ys_len, int sfmt, const void *commitment, const void *witness, int pfmt,
                        int *ok);
/* ---- bulk verification of coset openings (not a reference method) ---------------------------------------------------------
 * The check of kzg_verify_eval_batched for the cells of the coset calls above ("all coset openings": N = 2^log_n, l = 2^log_l,
 * K = N / l, coset i = { w^(i + tK) : t < l } with vanishing polynomial X^l - w^(il)), `count` cells per call, independent checks,
 * one verdict per cell -- what a caller needs before kzg_recover_cosets, which is only sound on verified cells.  Per cell:
 *   r_i from the l values in Fr (u = iNTT_l(v) over nu = w^K, r_{i,j} = u_j w^(-ij): the out_r of kzg_witness_cosets_coeff),
 *   R_i = sum_j r_{i,j} gs[j] gathered from a fixed-base window table of gs[0 .. l) (signed 8-bit digits: 32 l mixed additions, no
 *   doubling, no bucket method), and e(pi_i, hs[l]) e(-([w^(il)] pi_i + C - R_i), hs[0]) == 1 -- the equation
 *   e(pi_i, [tau^l]H - [w^(il)]H) == e(C - R_i, H) with both G2 arguments fixed, so one GPU thread runs one check against stored
 *   Miller lines as kzg_verify_eval does.
 * A kzg_cosets_verifier holds, for one SRS, one domain and one coset size, the table T[win][j][d] = [d 2^(8 win)] gs[j] (affine,
 * d = 1 .. 128: 393 KiB x l, at most 101 MB at the limit l = 256), the lines of hs[0] and hs[l] and the powers of w; it is immutable
 * after creation and may be used from any thread and every kzg_ctx on its device.  Setup (takes the context exclusively):
 * KZG_ERR_SHAPE if len(gs) < l, len(hs) < l + 1, log_l > log_n, log_n > 22, log_l > 8 or an SRS on another GPU.  log_l == 0 is
 * kzg_verify_eval at the points w^i. */
typedef struct kzg_cosets_verifier kzg_cosets_verifier;
int kzg_cosets_verifier_setup(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, uint32_t log_n, uint32_t log_l,
                              kzg_cosets_verifier **out);
void kzg_cosets_verifier_free(kzg_ctx *ctx, kzg_cosets_verifier *plan);
/* *domain = N, *coset_size = l, *table_bytes = the window table's size in HBM (each may be NULL); KZG_ERR_SHAPE for a NULL plan */
int kzg_cosets_verifier_shape(const kzg_cosets_verifier *plan, size_t *domain, size_t *coset_size, size_t *table_bytes);
/* Cell k belongs to commitments[commitment_idx[k]] (n_commitments points in pfmt, host) and coset coset_ids[k]; its l values are at
 * cells + 32 k l (sfmt; KZG_IN_DEVICE applies to `cells` alone), its proof is proofs[k] (pfmt, host).  Ids and indices are host
 * memory, always.  ok[k] = 1 or 0.  Duplicate (commitment, coset) pairs are allowed; the identity proof verifies iff C == R (what
 * FK20 emits for n <= l).  Points are validated as in kzg_verify_eval: a malformed, off-curve or out-of-subgroup commitment or proof
 * makes the call return KZG_ERR_BAD_POINT and leaves `ok` unwritten.  KZG_ERR_SHAPE, before any memory is touched: an id >= K, an
 * index >= n_commitments, an unknown format, a Jacobian pfmt, a NULL pointer with count > 0, a plan on another GPU; count == 0
 * returns KZG_OK.  Leases one lane like the other blocking calls (concurrent callers run side by side); works in chunks of at most
 * min(16384, 2^20 / l) cells (option "verify_cosets_chunk" lowers it), so the workspace does not grow with `count`; the commitments are decoded once per call, which takes
 * n_commitments x (point size + 192) bytes of it. */
int kzg_verify_cosets(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                      const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs, size_t count,
                      int sfmt, int pfmt, int flags, uint8_t *ok);
/* "Are all of these cells good?": ONE verdict for the whole call from one pairing check (the verify_cell_kzg_proof_batch shape of the
 * data-availability-sampling specifications).  Every argument means what it means in kzg_verify_cosets and the plan is the same.  With
 * the challenge r (one host scalar in sfmt) the per-cell equations are weighted by rho_k = r^k, k = 0 .. count - 1, and summed:
 *   a_j = sum_k rho_k r_{k,j},  Ragg = sum_j a_j gs[j];   c_m = sum_{k: m_k = m} rho_k,  Cagg = sum_m c_m C_m;
 *   P1 = sum_k rho_k pi_k,  P2 = sum_k (rho_k w^(i_k l)) pi_k;   *ok = [ e(P1, hs[l]) e(-(P2 + Cagg - Ragg), hs[0]) == 1 ].
 * Per cell that is an interpolation in Fr and 2 x 32 bucket additions of a variable-base multi-scalar sum (signed 8-bit digits);
 * the fixed-base sum and the pairing check happen once per call.
 * WHAT THE CALLER OWES.  The verdict is sound only if r is unpredictable to whoever produced the cells: draw it at random AFTER the
 * cells, proofs and commitments have been received, or derive it as a hash of ALL inputs of the call, as the consensus specifications
 * do (the library has no hash, and the domain separation is the protocol's business).  With a predictable r a forger can make errors
 * cancel: with r = 1, pi_a + D and pi_b - D in one coset pass.  Honest cells pass for every r.  *ok == 0 says nothing about WHICH
 * cell is bad: follow it with kzg_verify_cosets.
 * r == 0 (only cell 0 would be checked) or r >= modulus: KZG_ERR_SHAPE.  count == 0: *ok = 1 (if ok is non-NULL), KZG_OK.  Every other
 * shape error and KZG_ERR_BAD_POINT follow the rules of kzg_verify_cosets exactly and leave *ok unwritten; duplicate (commitment,
 * coset) pairs and identity proofs are allowed.  Leases one lane, works in the chunks of kzg_verify_cosets (option
 * "verify_cosets_chunk"), so the workspace does not grow with `count` (Limits).  Option "host_pairing" chooses where the one pairing
 * check runs. */
int kzg_verify_cosets_batch(kzg_ctx *ctx, const kzg_cosets_verifier *plan, const void *commitments, size_t n_commitments,
                            const uint32_t *commitment_idx, const size_t *coset_ids, const void *cells, const void *proofs,
                            size_t count, const void *r, int sfmt, int pfmt, int flags, int *ok);
/* "Are all of these openings good?" for single-point openings: ONE verdict for the whole call from one pairing check (the
 * verify_kzg_proof_batch / verify_blob_kzg_proof_batch shape of the data-availability specifications; not a reference method).
 * Opening k claims p_{m_k}(x_k) = y_k with the witness witnesses[k], where m_k = commitment_idx[k] names one of the n_commitments
 * points of `commitments`; commitment_idx == NULL means m_k = k and requires n_commitments == count (one commitment per opening).
 * With the challenge r (one host scalar in sfmt) the equations of kzg_verify_eval are weighted by rho_k = r^k, k = 0 .. count - 1,
 * and summed:
 *   P1 = sum_k rho_k pi_k,  P2 = sum_k (rho_k x_k) pi_k;   c_m = sum_{k: m_k = m} rho_k,  Cagg = sum_m c_m C_m;
 *   yagg = sum_k rho_k y_k;   *ok = [ e(P1, hs[1]) e(-(P2 + Cagg - [yagg] gs[0]), hs[0]) == 1 ].
 * Per opening that is 2 x 32 (3 x 32 without indices) bucket additions of a variable-base multi-scalar sum; the pairing check happens
 * once per call.  xs, ys, the points, the indices and r are host memory.  xs and ys (count scalars each, sfmt) are taken as
 * kzg_verify_eval takes them: they are not range-checked, and a value >= the modulus counts as its residue.  pfmt: any affine format.
 * Duplicate openings, the identity witness (a constant polynomial), the identity commitment and commitments that no opening names
 * (c_m = 0; they are validated all the same) are allowed.
 * WHAT THE CALLER OWES.  The verdict is sound only if r is unpredictable to whoever produced the openings: draw it at random AFTER the
 * points, values, witnesses and commitments have been received, or derive it as a hash of ALL inputs of the call, as the consensus
 * specifications do (the library has no hash, and the domain separation is the protocol's business).  With a predictable r a forger
 * can make errors cancel: with r = 1, pi_a + D and pi_b - D at one common x pass while both openings fail alone.  Honest openings
 * pass for every r.  *ok == 0 says nothing about WHICH opening is bad: follow it with kzg_verify_eval.
 * KZG_ERR_SHAPE, before any memory is touched and with *ok unwritten: r == 0 (only opening 0 would be checked) or r >= modulus, gs
 * without a point or hs with fewer than two, an index >= n_commitments, NULL indices with n_commitments != count, an unknown format,
 * a Jacobian pfmt, a NULL pointer with count > 0, an SRS on another GPU.  count == 0: *ok = 1 (if ok is non-NULL), KZG_OK -- of
 * the errors above only the formats and the SRS (NULL, too short, another GPU) are looked at then, not r, the pointers or n_commitments,
 * as in kzg_verify_cosets_batch.  Points are
 * validated as in kzg_verify_eval (option "trusted_points"): a malformed, off-curve or out-of-subgroup commitment or witness makes
 * the call return KZG_ERR_BAD_POINT and leaves *ok unwritten.  Leases one lane like the other blocking calls (concurrent callers run
 * side by side); works in chunks of at most 16384 openings (option "verify_eval_batch_chunk" lowers it), so the workspace does not
 * grow with `count` (Limits).  Option "host_pairing" chooses where the one pairing check runs. */
int kzg_verify_eval_batch(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *xs, const void *ys, int sfmt,
                          const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt,
                          size_t count, const void *r, int *ok);
/* The verifier of kzg_open_fold_eval / kzg_open_fold_coeff: ONE verdict from one pairing check for `groups` folded openings.  Group g
 * claims p_{m(g,i)}(zs[g]) = ys[g t + i] for i < t with the ONE witness witnesses[g], folded with gammas[g]; m(g,i) =
 * commitment_idx[g t + i] names one of the n_commitments points of `commitments` (NULL: m(g,i) = g t + i, and n_commitments ==
 * groups x t is required).  With rho_{g,i} = r^g gammas[g]^i:
 *   c_m = sum_{m(g,i) = m} rho_{g,i},  Cagg = sum_m c_m C_m,  yagg = sum rho_{g,i} y_{g,i};
 *   P1 = sum_g r^g pi_g,  P2 = sum_g (r^g z_g) pi_g;   *ok = [ e(P1, hs[1]) e(-(P2 + Cagg - [yagg] gs[0]), hs[0]) == 1 ].
 * zs, gammas: `groups` host scalars each, ys: groups x t, r: one (may be NULL when groups == 1), all in sfmt.  ys are taken as
 * kzg_verify_eval_batch takes them (a value >= the modulus counts as its residue); zs, gammas and r are range-checked.
 * WHAT THE CALLER OWES.  gamma_g must be unpredictable to whoever chose the polynomials AND the claimed values of group g: in practice
 * a hash of the commitments, z and the ys.  With a predictable gamma wrong values cancel inside the fold: for t = 2 the claims
 * y_0 + D and y_1 - D / gamma have the fold y_F of the true values, so the honest folded witness passes although both values are
 * wrong (gamma = 1: y_0 + 1 and y_1 - 1).  r must be unpredictable to whoever produced EVERYTHING, witnesses included: draw it after
 * all inputs are received or hash all of them, as for kzg_verify_eval_batch (with r = 1, pi_a + D and pi_b - D at one z pass).
 * Honest openings pass for every gamma and r.  *ok == 0 does not say which group or value is bad.
 * KZG_ERR_SHAPE, before memory is touched and with *ok unwritten: t == 0, a gamma == 0 or >= modulus, r == 0 or >= modulus or NULL
 * when groups > 1, a z >= modulus, an index >= n_commitments, NULL indices with n_commitments != groups x t, groups x t beyond
 * size_t, and every condition of kzg_verify_eval_batch (formats, SRS, NULL pointers).  groups == 0: *ok = 1 (if ok is non-NULL),
 * KZG_OK.  Point validation and KZG_ERR_BAD_POINT (*ok unwritten), the lane, the chunking (option "verify_eval_batch_chunk": witnesses
 * per chunk, then values and commitments per chunk) and options "host_pairing" / "trusted_points" are kzg_verify_eval_batch's. */
int kzg_verify_fold(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt,
                    const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, const void *witnesses, int pfmt,
                    size_t t, size_t groups, const void *gammas, const void *r, int *ok);
/* The verifier of kzg_multiopen_*_commit / _finish: ONE verdict from one pairing check for count claims p_{m(k)}(zs[k]) = ys[k] answered
 * by the two elements d_point (D) and pi; m(k) = commitment_idx[k] names one of the n_commitments points of `commitments` (NULL:
 * m(k) = k, n_commitments == count required).  With w_k = r^k / (t - z_k):
 *   E = sum_m W_m C_m,  W_m = sum_{m(k) = m} w_k,  g2 = sum_k w_k y_k;   *ok = [ e(pi, hs[1]) e(-(t pi + E - D - [g2] gs[0]), hs[0]) == 1 ]:
 * kzg_verify_eval of the commitment E - D at (t, g2) with the witness pi.  zs, ys: count host scalars, r, t: one each, all in sfmt; ys
 * are taken as kzg_verify_eval_batch takes them (a value >= the modulus counts as its residue); zs, r and t are range-checked.
 * WHAT THE CALLER OWES.  r must be unpredictable to whoever chose the polynomials, points and values; t MUST BE DRAWN AFTER D WAS
 * RECEIVED, as a hash that includes D.  With a t the prover knew before it chose D, ONE WRONG claim (C, z, y') passes: pi = the
 * identity and D = (C - [y'] gs[0]) / (t - z), which needs no knowledge of tau.  Honest proofs pass for every r and every t that is
 * no z_k.  *ok == 0 does not say which claim is bad.
 * KZG_ERR_SHAPE, before memory is touched and with *ok unwritten: r == 0 or >= modulus, t or a z >= modulus, t equal to a z_k (the
 * caller draws another t), an index >= n_commitments, NULL indices with n_commitments != count, and every condition of
 * kzg_verify_eval_batch (formats, SRS, NULL pointers).  count == 0: *ok = 1 (if ok is non-NULL), KZG_OK.  Point validation of every
 * C_m, D and pi and KZG_ERR_BAD_POINT (*ok unwritten), the lane, the chunking (option "verify_eval_batch_chunk": the weights are
 * formed on the host with one inversion per chunk) and options "host_pairing" / "trusted_points" are kzg_verify_eval_batch's. */
int kzg_verify_multiopen(kzg_ctx *ctx, const kzg_srs *gs, const kzg_srs_g2 *hs, const void *zs, const void *ys, int sfmt,
                         const void *commitments, size_t n_commitments, const uint32_t *commitment_idx, size_t count, const void *r,
                         const void *t, const void *d_point, const void *pi, int pfmt, int *ok);

/* ---- Fr polynomial helpers on the path (device) ---------------------------------------------- */
/* Polynomial::eval (src/polynomial.rs:156-165) at one point.  x is a host scalar in sfmt; y_out: one scalar in sfmt, always host memory. */
int kzg_poly_eval(kzg_ctx *ctx, const void *coeffs, size_t n, const void *x, int sfmt, int flags, void *y_out);
/* Polynomial::multi_eval (src/polynomial.rs:229-233) without its xs.len() > degree restriction, for `batch` polynomials at one
 * point set: ys_out[b * k + i] = p_b(xs[i]).  coeffs: batch x n scalars in sfmt, stride n (KZG_IN_DEVICE applies to it);
 * xs: k host scalars in sfmt; ys_out: batch x k scalars in sfmt, host, or device with KZG_OUT_DEVICE.
 * One call instead of k x batch kzg_poly_eval calls, and the same bytes: every value is the residue below r in the form of sfmt.
 * Coefficients may be any 256-bit value and count as their residue; each xs[i] must be below r; repeated points give repeated
 * values.  KZG_ERR_SHAPE, before memory is touched: n == 0 or n > 2^28, an unknown format, a NULL context or buffer, an x >= r.
 * k == 0 or batch == 0: KZG_OK, nothing written.  Blocking, on one leased lane.  Cost: n k batch field products in two kernels per
 * pass (Horner per point and segment, then over the segments); up to 7 values in all (k x batch; 12 with k <= 2) one kzg_poly_eval
 * scan per value instead, which is faster there (options "multi_eval_segment" / "multi_eval_points_chunk"; measurements: DESIGN.md
 * section 3.4e). */
int kzg_poly_multi_eval(kzg_ctx *ctx, const void *coeffs, size_t n, size_t batch, const void *xs, size_t k, int sfmt, int flags,
                        void *ys_out);
/* Polynomial::lagrange_interpolation (src/polynomial.rs:266-293): out[b * k + j] = coefficient j of the unique polynomial of degree < k
 * through (xs[i], ys[b * k + i]).  One point set, `batch` value vectors; xs, ys host scalars; out host, or device with KZG_OUT_DEVICE.
 * k <= 16384 (the k x k basis matrix).  Two equal xs: KZG_ERR_SHAPE (the reference panics in invert().unwrap()).
 * k == 1 gives the constant y (the reference returns X + (y - x) there, src/polynomial.rs:269-272: that quirk is the caller's to
 * mirror).  Also KZG_ERR_SHAPE, before `out` is written: k == 0, k > 16384, an x >= r, an unknown format, a NULL context or buffer.
 * batch == 0: KZG_OK.  The basis matrix is built once per call, each value vector costs one k x k matrix-vector product. */
int kzg_interpolate(kzg_ctx *ctx, const void *xs, const void *ys, size_t k, size_t batch, int sfmt, int flags, void *out);
/* SubProductTree (src/polynomial.rs:303-365) as a device-resident plan the caller keeps: the sub-product tree of an arbitrary point
 * set, and on it Polynomial::multi_eval (:229-233), SubProductTree::linear_mod_combination (:347-365), lagrange_interpolation_with_tree
 * (:237-293) and the product polynomial, each in O(k log^2 k) field products where kzg_poly_multi_eval and kzg_interpolate take
 * n k and k^2 (which of the two to call: DESIGN.md section 3.4g; nothing is rerouted).
 * kzg_point_tree_setup: xs = k host scalars in sfmt, each below r (else KZG_ERR_SHAPE), 1 <= k <= 2^22; repeated points are allowed.
 * Exclusive, like the other *_setup calls.  The plan is immutable afterwards and, like a kzg_srs, usable from any thread and from every
 * context on the same device.  It holds the tree padded to next_pow2(k) points with dummy points 0, the transforms of its nodes above
 * the leaf size (option "point_tree_leaf"), the power-series inverse of the reversed root and 1 / M'(x_i).
 * kzg_point_tree_shape: k, the padded size, the bytes the plan holds in HBM, and distinct = 0 if two points coincide.
 * kzg_point_tree_product: the k + 1 coefficients of M = prod (X - x_i) (tree.product).
 * kzg_point_tree_eval: ys_out[b * k + i] = p_b(xs[i]); coeffs is batch x n scalars, stride n; any n >= 1 (n <= 2^28): there is no
 * xs.len() > degree assertion, polynomials longer than the padded size go through in blocks.  The bytes are those of
 * kzg_poly_multi_eval on the same inputs.  Where SubProductTree::eval panics on a zero remainder (:342-343: a polynomial that
 * vanishes on a whole subtree) this call returns the values.
 * kzg_point_tree_combine: out[b * k + j] = coefficient j of sum_i cs[b * k + i] M / (X - x_i); k coefficients, zero-padded.
 * kzg_point_tree_interpolate: the bytes of kzg_interpolate: combine of ys[b * k + i] / M'(x_i).  A plan with repeated points gives
 * KZG_ERR_SHAPE before `out` is written.  k == 1 gives the constant y (the reference's X + (y - x) there is the caller's to mirror).
 * All four: coefficients, cs and ys may be any 256-bit value and count as their residue; outputs are residues below r in sfmt;
 * KZG_IN_DEVICE (coeffs / cs / ys) and KZG_OUT_DEVICE as for kzg_poly_multi_eval; batch == 0: KZG_OK, nothing written; a NULL context,
 * plan or buffer or an unknown format: KZG_ERR_SHAPE before memory is touched.  Blocking, on one leased lane; polynomials / vectors go
 * in chunks of max(1, 2^21 / padded size) blocks, so the workspace (96 bytes per point of a chunk) does not grow with batch. */
typedef struct kzg_point_tree kzg_point_tree;
int kzg_point_tree_setup(kzg_ctx *ctx, const void *xs, size_t k, int sfmt, kzg_point_tree **out);
void kzg_point_tree_free(kzg_ctx *ctx, kzg_point_tree *plan);
int kzg_point_tree_shape(const kzg_point_tree *plan, size_t *k, size_t *padded, size_t *bytes, int *distinct);
int kzg_point_tree_product(kzg_ctx *ctx, const kzg_point_tree *plan, int sfmt, int flags, void *out);
int kzg_point_tree_eval(kzg_ctx *ctx, const kzg_point_tree *plan, const void *coeffs, size_t n, size_t batch, int sfmt, int flags,
                        void *ys_out);
int kzg_point_tree_combine(kzg_ctx *ctx, const kzg_point_tree *plan, const void *cs, size_t batch, int sfmt, int flags, void *out);
int kzg_point_tree_interpolate(kzg_ctx *ctx, const kzg_point_tree *plan, const void *ys, size_t batch, int sfmt, int flags, void *out);
/* quotient of create_witness without the MSM: q = (p - y)/(X - x), n-1 scalars, in place allowed.
 * Returns KZG_ERR_POINT_NOT_ON_POLY if the remainder is non-zero.  x, y: host scalars in sfmt (y is compared with p(x) in that form);
 * q_out is in sfmt, host memory or device memory with KZG_OUT_DEVICE. */
int kzg_quotient_linear(kzg_ctx *ctx, const void *coeffs, size_t n, const void *x, const void *y, int sfmt,
                        int flags, void *q_out);
/* div_by_omega_i (src/eval_form.rs:58-84) applied to (evals - evals[i]): d scalars in sfmt, host memory or device memory with KZG_OUT_DEVICE. */
int kzg_quotient_eval(kzg_ctx *ctx, const void *evals, size_t d, size_t i, int sfmt, int flags, void *q_out);

/* Polynomial::fft_mul / best_mul (src/polynomial.rs:167-191): out = a * b, na + nb - 1 coefficients, by three
 * NTTs of size next_pow2(na + nb) and a pointwise product (EvaluationDomain::mul_assign, src/ft.rs:220-244).
 * The product is unique, so it equals the reference's naive Mul (:473-487) as well.  Host or device buffers. */
int kzg_poly_mul(kzg_ctx *ctx, const void *a, size_t na, const void *b, size_t nb, int sfmt, int flags, void *out);
/* Polynomial::long_division (src/polynomial.rs:193-227) by a divisor of any degree, for `batch` dividends and ONE divisor:
 * a_bi = q_bi b + r_bi with deg r_bi < deg b.  a: batch x na scalars in sfmt, stride na; b: nb scalars, b[0] the constant term
 * (KZG_IN_DEVICE applies to both).  Coefficients may be any 256-bit value and count as their residue.  b[nb - 1] must be non-zero
 * mod r (pass slice_coeffs(), as for kzg_commit_coeff): a zero top coefficient -- the zero divisor included, where the reference
 * panics with "divisor must not be zero" -- is KZG_ERR_SHAPE; for a device-resident divisor the check is one 32-byte read.
 * Dividends may have leading zero coefficients and may be zero.
 * q_out: batch x (na - nb + 1) scalars, stride na - nb + 1; r_out: batch x (nb - 1) scalars, stride nb - 1; both in sfmt, every value
 * the residue below r, zero-padded to these lengths, to the host or (KZG_OUT_DEVICE) the device.  Either may be NULL, not both
 * unless both would be empty.  na < nb: q_out is not touched, r_out is the dividend zero-padded to nb - 1.  nb == 1: r_out is not
 * touched, q = a / b[0].  exact (optional, batch ints, host): exact[bi] = 1 iff the remainder of dividend bi is zero (the
 * reference's None); computed on the device, with or without r_out.  The quotient and the remainder are unique, so the bytes are the
 * reference's.
 * KZG_ERR_SHAPE, before any output is written: a NULL context, NULL a or b (batch > 0), both outputs NULL where one would not be
 * empty, na == 0, nb == 0, an unknown format, a top coefficient that is 0 mod r, na > 2^27, batch x na x 32 beyond size_t.
 * batch == 0: KZG_OK, nothing written.  Blocking, on one leased lane.  Cost: the power-series inverse of rev(b) to na - nb + 1 terms
 * once per call (a one-workgroup schoolbook base, option "poly_divide_base", then Newton doubling through the NTT), per dividend
 * one product of next_pow2(2 (na - nb) + 1) points against the once-transformed inverse and, for the remainder, two streaming
 * folds and one product of next_pow2(nb - 1) points. */
int kzg_poly_divide(kzg_ctx *ctx, const void *a, size_t na, size_t batch, const void *b, size_t nb, int sfmt, int flags, void *q_out,
                    void *r_out, int *exact);

/* ---- device memory + measurement ------------------------------------------------------------- */
int kzg_dev_alloc(kzg_ctx *ctx, size_t bytes, void **out);
int kzg_dev_free(kzg_ctx *ctx, void *p);
int kzg_dev_upload(kzg_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int kzg_dev_download(kzg_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Fill n Fr elements with a counter-based generator (SplitMix64 of (seed, i), reduced mod r;
 * `u64_valued` != 0 mirrors the reference benches' u64-valued coefficients,
 * benches/commit_coeff_form.rs:16-21).  Output canonical or Montgomery per sfmt. */
int kzg_fill_random_fr(kzg_ctx *ctx, void *dst_dev, size_t n, uint64_t seed, int u64_valued, int sfmt);
/* Per-kernel HIP-event timing on the stream the kernels run on (for bench.py's roofline line).  on = 1: every kernel; on = 2: the
 * bucket-accumulation kernel only (two events per launch of all ~14 kernels of an MSM cost 1.4 % of the batched rate, one pair per
 * MSM does not); 0: off. */
int kzg_prof_enable(kzg_ctx *ctx, int on);
int kzg_prof_reset(kzg_ctx *ctx);
int kzg_prof_get(kzg_ctx *ctx, const char *kernel, uint64_t *launches, double *total_ms);
/* comma-separated list of kernel names seen so far */
int kzg_prof_names(kzg_ctx *ctx, char *buf, size_t buflen);
/* The v_mad_i64_i32 issue rate of THIS device, measured now (~30 ms at 8 waves per SIMD: 8 independent accumulator chains per
 * lane), in 10^12 lane-multiply-adds per second: the roofline peak bench.py prices the bucket-accumulation kernel against
 * (devices of one pool differ by several percent, and the sustained clock under this load is not the nominal one). */
int kzg_measure_mad_issue_rate(kzg_ctx *ctx, int waves_per_simd, double *tera_lane_mads_per_s);
/* number of window bits and windows the engine chose for this SRS (for G1-adds accounting) */
int kzg_srs_window_info(const kzg_srs *srs, int *window_bits, int *windows);
int kzg_srs_table_rows(const kzg_srs *srs);   /* resident table rows (= windows unless option window_rows) */

#ifdef __cplusplus
}
#endif
#endif /* KZG_MI355X_H */
