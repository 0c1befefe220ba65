// verify_cosets_shared.h -- what verify_cosets.hip (one verdict per cell) and verify_cosets_batch.hip (one verdict per call) share:
// the window constants and the digit recoding, the plan, and the two stages both run per chunk (defined in verify_cosets.hip).
#pragma once
#include "pairing_shared.h"

namespace kzg {

constexpr uint32_t VC_MAX_LOG_L = 8;    // cosets of up to 256 points (include/kzg_mi355x.h, Limits)
constexpr uint32_t VC_MAX_LOG_N = 22;   // the FK20 plans' limit: what can be proved can be verified
constexpr int VC_C = 8;                 // window bits: 32 windows x 128 entries per base (DESIGN.md 3.5e for the choice)
constexpr int VC_W = (256 + VC_C - 1) / VC_C;
constexpr uint32_t VC_D = 1u << (VC_C - 1);
constexpr size_t VC_CHUNK_CELLS = 16384, VC_CHUNK_SCALARS = (size_t)1 << 20;  // cells per chunk: min(16384, 2^20 / l)

// Signed digit `win` of a canonical scalar (Booth recoding: every digit from its own c + 1 bits, no carry chain, so any lane can
// take any window): d = bits[c win, c win + c) + bit[c win - 1] - 2^c bit[c win + c - 1], |d| <= 2^(c-1); c W >= 256 > the top bit
__device__ __forceinline__ int vc_digit(const uint32_t *k, int win) {
    const int lo = VC_C * win - 1;
    uint32_t x;
    if (lo < 0) {
        x = (k[0] << 1) & ((2u << VC_C) - 1u);
    } else {
        const int w = lo >> 5, sh = lo & 31;
        x = k[w] >> sh;
        if (sh && w + 1 < 8) x |= k[w + 1] << (32 - sh);
        x &= (2u << VC_C) - 1u;
    }
    const int d = (int)(x >> 1) + (int)(x & 1u);
    return (x >> VC_C) ? d - (1 << VC_C) : d;
}

}  // namespace kzg

struct kzg_cosets_verifier {
    uint32_t log_n = 0, log_l = 0;
    int device = 0;
    size_t table_bytes = 0;
    kzg::G1Affine *table = nullptr;  // [VC_W][l][VC_D]
    kzg::G2Affine *hq = nullptr;     // hs[0], hs[l]
    kzg::Fq2 *lines = nullptr;       // their stored Miller lines, 2 x 2 MILLER_LINES
    // powers of w = compute_omega(N), Montgomery: ninv_lo[e] = w^-e / l and pos_lo[e] = w^e for e < 1024, ninv_hi[h] = w^(-1024 h) and
    // pos_hi[h] = w^(1024 h) for h < max(1, N / 1024); nu_inv[e] = nu^-e for e < max(1, l / 2).  One allocation (ninv_lo).
    kzg::Fr *ninv_lo = nullptr, *ninv_hi = nullptr, *pos_lo = nullptr, *pos_hi = nullptr, *nu_inv = nullptr;
    // host copies of hq and lines: kzg_verify_cosets_batch finishes its one pairing check on the calling thread (option host_pairing)
    kzg::G2Affine h_hq[2];
    kzg::Fq2 h_lines[2 * 2 * kzg::MILLER_LINES];
};

namespace kzg {
// stages 1 and 2 of a chunk of B cells on stream st: d_cells (sfmt) -> d_r (sfmt) -> d_R
int vc_interp(kzg_ctx *ctx, hipStream_t st, const kzg_cosets_verifier *p, const Fr *d_cells, const uint32_t *d_ids, size_t B, Fr *d_r);
int vc_sum(kzg_ctx *ctx, hipStream_t st, const kzg_cosets_verifier *p, const Fr *d_r, size_t B, int sfmt, G1Xyzz *d_R);
size_t vc_chunk(const kzg_ctx *ctx, const kzg_cosets_verifier *p);  // cells per chunk: the rule, lowered by option verify_cosets_chunk
}  // namespace kzg
