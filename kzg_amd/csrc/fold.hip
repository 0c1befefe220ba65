// fold.hip -- the random linear combination of t vectors of Fr by the powers of one challenge, for many groups at once:
//   out[g d + j] = sum_{i < t} gamma_g^i v[(g t + i) d + j]
// (kzg_fr_fold, and the fold of kzg_open_fold_eval / kzg_open_fold_coeff in capi.hip).  DESIGN.md section 3.4c.
//
// Horner over i, highest index first: acc = acc gamma + v_i.  gamma_g is the same for every lane of a workgroup (blockIdx.y is the
// group), so it is read through the scalar cache and multiplies out of SGPRs; only the elements differ per lane.  A lane streams
// t elements of 32 bytes, d elements apart: FOLD_U of them (two 16-byte loads each) are requested before the first is used, so the
// loads of a step are in flight while the multiply-adds of the step before run.  The accumulator may start from `out` (carry): a
// caller that stages its vectors in pieces folds piece after piece, from the last one down, with the running sum in HBM between them.
// gamma is Montgomery and the map is linear: the output has the form the inputs have.  Inputs may be any 256-bit value (a caller's
// canonical scalars): they count as their residue, the oe_load rule of open_eval.hip.
#include <algorithm>

#include "common.h"

namespace kzg {

constexpr int FOLD_U = 4;  // vectors whose elements a lane has requested before it uses the first

__device__ __forceinline__ Fr fold_residue(Fr f) { return fr_residue(f); }  // any value below 2^256 < 3r as a residue below r (field.h)

// grid (ceil(d / 256), groups); v: group g at v + g gstride, its vector i at + i d; gammas[g] Montgomery
__global__ __launch_bounds__(256) void k_fr_fold(const Fr *v, size_t d, size_t t, size_t gstride, const Fr *gammas, int carry, Fr *out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= d) return;
    const size_t g = blockIdx.y;
    const Fr gm = gammas[g];  // uniform
    const Fr *p = v + g * gstride + j;
    Fr acc = carry ? out[g * d + j] : Fr::zero();
    size_t i = t;
    for (; i >= (size_t)FOLD_U; i -= FOLD_U) {
        Fr x[FOLD_U];
#pragma unroll
        for (int u = 0; u < FOLD_U; u++) x[u] = p[(i - 1 - u) * d];
#pragma unroll
        for (int u = 0; u < FOLD_U; u++) acc = add(mul(acc, gm), fold_residue(x[u]));
    }
    for (; i > 0; i--) acc = add(mul(acc, gm), fold_residue(p[(i - 1) * d]));
    out[g * d + j] = acc;
}

// d_out[g d + j] (+ carry: = d_out[g d + j] gamma_g^t +) sum_{i < t} gamma_g^i d_v[g gstride + i d + j] for g < groups, on `st`
int fold_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, size_t t, size_t gstride, size_t groups, const Fr *d_gammas_mont,
             bool carry, Fr *d_out) {
    if (!d || !t || !groups) return KZG_OK;
    const size_t nblk = (d + 255) / 256;
    if (nblk > 0x7fffffffu) return fail(ctx, KZG_ERR_SHAPE, "fold: vectors too long");
    for (size_t g0 = 0; g0 < groups; g0 += 65535) {  // (gridDim.y)
        const size_t G = std::min<size_t>(65535, groups - g0);
        KZG_LAUNCH(ctx, st, "k_fr_fold", k_fr_fold, dim3((unsigned)nblk, (unsigned)G), 256, 0, d_v + g0 * gstride, d, t, gstride, d_gammas_mont + g0,
                   carry ? 1 : 0, d_out + g0 * d);
    }
    return KZG_OK;
}

}  // namespace kzg
