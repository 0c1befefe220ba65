// pairing_shared.h -- what the verifier's translation units (pairing.hip, verify_cosets.hip) share besides tower.h: the resident G2
// points and the two helpers every verifier entry point brings its G1 inputs in and its verdicts out with.
#pragma once
#include "common.h"
#include "tower.h"

struct kzg_srs_g2 {
    size_t n = 0;
    kzg::G2Affine *pts = nullptr;  // affine Montgomery (= blst_p2_affine), identity all-zero
    kzg::Fq2 *lines = nullptr;     // Miller-loop lines of pts[0] and pts[1] (2 x 2*MILLER_LINES Fq2): the verifier's
                                   // second pairing argument is always one of these two, so a check does no G2 arithmetic
    int device = 0;
    // host copies of pts[0], pts[1] and lines, made when the points are created (they never change afterwards): kzg_verify_eval_batch
    // finishes its one pairing check on the calling thread (option host_pairing)
    kzg::G2Affine h_pts[2] = {};
    kzg::Fq2 h_lines[2 * 2 * kzg::MILLER_LINES] = {};
};

namespace kzg {
// decode `count` G1 points of format pfmt (host memory) into XYZZ on the device, in the lane's arena and on its stream
int g1_inputs(kzg_ctx *ctx, int lane, const void *host, size_t count, int pfmt, G1Xyzz **d_out, int *d_bad);
// the verdicts and the decode flag of one launch: KZG_ERR_BAD_POINT if the flag is set (ok is then not written); synchronises the lane
int fetch_ok(kzg_ctx *ctx, int lane, const uint8_t *d_ok, const int *d_bad, size_t count, uint8_t *ok);
// bytes of one G2 point in a KZG_G2_* format (0: unknown format); k_g2_encode: n affine points -> d_out, one after the other
size_t g2_point_bytes(int fmt);
int g2_encode_run(kzg_ctx *ctx, hipStream_t st, const G2Affine *d_in, size_t n, int fmt, uint8_t *d_out);
// k_g2_decode: n points of a KZG_G2_* format at d_raw -> affine at d_out, checked at `level` (*d_bad |= 1 at a point that fails)
int g2_decode_run(kzg_ctx *ctx, hipStream_t st, const uint8_t *d_raw, size_t n, int fmt, G2Affine *d_out, int *d_bad, int level);
// g2ntt.hip, the G2 DFT: d_out[i] = (1/d) sum_j w^(-ij) d_in[j] over d = 2^log_d <= 2^20 affine points, on lane 0's stream and arena
// (compute_lagrange_basis, G2 half); d_out may not overlap d_in
constexpr uint32_t G2NTT_MAX_LOG = 20;
int g2_lagrange_dft(kzg_ctx *ctx, const G2Affine *d_in, uint32_t log_d, G2Affine *d_out);
// g2_msm.hip, the bucket method behind kzg_msm_g2_bucket: sum_i d_sc[i] srs[offset + i] -> d_out (affine) on lane 0's stream; d_sc
// canonical and reduced (vcb_canon); takes g2_msm_bucket_workspace_bytes from lane 0's arena
size_t g2_msm_bucket_workspace_bytes(const kzg_ctx *ctx);
int g2_msm_bucket_device(kzg_ctx *ctx, const kzg_srs_g2 *srs, size_t offset, const Fr *d_sc, size_t n, G2Affine *d_out);
}  // namespace kzg
