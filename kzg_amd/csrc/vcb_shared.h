// vcb_shared.h -- what verify_cosets_batch.hip (one verdict for a call of coset openings) and verify_eval_batch.hip (one verdict for a
// call of single-point openings, of folded openings, of a two-element multiproof) share: the shape of the variable-base bucket sum, the
// stages all of them run, each a kernel of verify_cosets_batch.hip behind the function that launches it there (as
// verify_cosets_shared.h shares vc_interp and vc_sum), and the driver core around the stages: the workspace, points into buckets, the
// commitment weights of a chunk and the Cagg loop.  The host-only part of the core is vcb_host.h.
#pragma once
#include "vcb_finish.h"
#include "vcb_host.h"
#include "verify_cosets_shared.h"

namespace kzg {

constexpr uint32_t VCB_S = 2048;                     // points per slice: one workgroup sorts them by digit in LDS (16-bit indices)
constexpr uint32_t VCB_G = VC_CHUNK_CELLS / VCB_S;   // slice slots of a chunk
constexpr size_t VCB_SET = (size_t)VC_W * VC_D;      // buckets of one slot: 32 windows x 128
constexpr uint32_t VCB_FOLD_CELLS = 64;              // cells per k_vcb_fold workgroup
static_assert(VC_W == VCB_W, "vcb_finish.h and verify_cosets_shared.h disagree on the windows");
static_assert(VCB_S <= 32768, "the sorted entries keep the sign in bit 15");

inline unsigned vcb_grid(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

// the challenge r (host, sfmt) in Montgomery form; KZG_ERR_SHAPE in the name of `who` unless it is in [1, modulus)
int load_challenge(kzg_ctx *ctx, const char *who, const void *r, int sfmt, Fr *mont);
// k_vcb_canon: out[i] = in[i] canonical and reduced (in place allowed)
int vcb_canon(kzg_ctx *ctx, hipStream_t st, const Fr *d_in, size_t n, int is_mont, Fr *d_out);
// k_vcb_fold, k_vcb_fold2: d_a[j] += sum_{k < B} d_rho[k] d_r[k l + j] in a fixed order (no atomics); d_r in the caller's scalar format,
// which d_a keeps, d_rho Montgomery, d_part: ceil(B / VCB_FOLD_CELLS) x l scalars of scratch
int vcb_fold(kzg_ctx *ctx, hipStream_t st, const Fr *d_r, const Fr *d_rho, size_t B, uint32_t log_l, Fr *d_part, Fr *d_a);
// k_vcb_cweights: d_c[which[g]] += sum of d_rho over order[start[g] .. start[g + 1]) for g < lists (Montgomery)
int vcb_cweights(kzg_ctx *ctx, hipStream_t st, const Fr *d_rho, const uint32_t *d_which, const uint32_t *d_start, const uint32_t *d_order,
                 size_t lists, Fr *d_c);
// k_vcb_bucket: the buckets of `sets` (1 or 2) scalar sets += the digits' multiples of n points (n <= VCB_G x VCB_S); canonical scalars
int vb_accumulate(kzg_ctx *ctx, hipStream_t st, const G1Xyzz *d_pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1, int sets);
int vb_accumulate(kzg_ctx *ctx, hipStream_t st, const G1Affine *d_pts, const Fr *sc0, const Fr *sc1, size_t n, G1Xyzz *bk0, G1Xyzz *bk1, int sets);
// k_vcb_reduce: three bucket sets of VCB_G slots each at d_bk, of which `slots` were used -> sums->win
int vb_reduce(kzg_ctx *ctx, hipStream_t st, const G1Xyzz *d_bk, uint32_t slots, VcbSums *d_sums);

// The end of both calls, after the reductions: the finish of vcb_finish.h on the calling thread (option host_pairing) or in k_vcb_finish,
// the decode flag d_bad read before the verdict (KZG_ERR_BAD_POINT, *ok unwritten).  d_hq, d_lines / h_hq, h_lines: the two G2 points
// and their stored lines in the order of vcb_check, on the device and on the host.  points (may be null): the four affine points the
// finish consumed (host).  Synchronises the lane.
int vcb_conclude(kzg_ctx *ctx, int lane, const VcbSums *d_sums, const G2Affine *d_hq, const Fq2 *d_lines, const G2Affine *h_hq,
                 const Fq2 *h_lines, const int *d_bad, uint8_t *d_ok, G1Affine *d_parts, void *points, int *ok);

// ---- the driver core: what every one of the four calls does around its own scalars ----
// The workspace of one call in its lane's arena: what all four calls allocate, and how many slice slots the bucket sets have in use.
struct VcbWork {
    kzg_ctx *ctx;
    int lane, pfmt;
    hipStream_t st;
    size_t psz, BP;                     // bytes of an encoded point | points raw and W hold
    int *bad;                           // the decode flag
    uint8_t *d_ok;
    G1Affine *d_parts;
    G1Xyzz *bk[3];                      // the bucket sets: P1, P2, and Cagg with whatever else the call adds to it
    VcbSums *sums;
    Fr *d_c;                            // c_count commitment weights
    uint32_t *d_which, *d_start, *d_order;  // a chunk's lists (VcbLists)
    Fr *d_rho, *d_s1, *d_s2;            // a chunk's weights (Montgomery) and its two scalar sets (canonical), B0 each
    uint8_t *raw;                       // BP encoded points
    G1Xyzz *W;                          // ... decoded
    size_t slots;                       // slice slots any step has used
};
// One lane_reserve for the buffers above (chunks of at most B0 openings, BP >= B0) plus extra_bytes, which the caller takes with
// lane_alloc afterwards (the 64 KiB of slack pay for every alignment); bad, the buckets and d_c zeroed on the lane's stream.
// slots0: the slice slots in use before any point arrives.
int vcb_work(kzg_ctx *ctx, int lane, int pfmt, size_t B0, size_t BP, size_t c_count, size_t extra_bytes, size_t slots0, VcbWork *w);
// B <= BP encoded points of the caller's (host) uploaded, decoded at untrusted_level into w->W, and added to the buckets bk0 and bk1
// against the canonical scalars sc0 and sc1 as vb_accumulate does it
int vcb_points(VcbWork *w, const void *src, size_t B, const Fr *sc0, const Fr *sc1, G1Xyzz *bk0, G1Xyzz *bk1, int sets);
// d_c[m] += the sum of w->d_rho over the chunk's openings of commitment m = cm[k], k < B: the counting sort, its upload, k_vcb_cweights
int vcb_commit_weights(VcbWork *w, VcbLists *lists, const uint32_t *cm, size_t B);
// Cagg: d_c made canonical in place and the n_commitments commitments (host) against it into the third set, in pieces of BP
int vcb_cagg(VcbWork *w, const void *commitments, size_t n_commitments);

}  // namespace kzg
