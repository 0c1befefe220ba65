// fr_program.h -- what the interpreters of a kzg_fr_program share: the plan, the column descriptor, the 32-byte global loads and stores
// and the conflict-free LDS slots of k_fr_program (fr_program.hip) and k_sumcheck_round (mle.hip).
#pragma once
#include "common.h"

struct kzg_fr_program {
    int device = 0;
    size_t n_cols = 0, n_consts = 0, n_out = 0, n_temps = 0, n_mul = 0;
    std::vector<uint32_t> words;   // validated, as given
};

namespace kzg {

struct FrpCol {
    const Fr *p;
    uint32_t len;
    uint32_t mask;   // len - 1 of a periodic column (a power of two); 0xFFFFFFFF: a full-length column, len == n
};

typedef uint32_t frp_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) frp_v4 frp_g4;   // column and output words are global memory: no flat access, whose loads would wait for LDS too

__device__ __forceinline__ Fr frp_load(const Fr *p) {
    const frp_g4 *g = (const frp_g4 *)p;
    const frp_v4 lo = g[0], hi = g[1];
    Fr v;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v.v[k] = lo[k];
        v.v[4 + k] = hi[k];
    }
    return v;
}

__device__ __forceinline__ void frp_store(Fr *p, const Fr &v) {
    frp_g4 *g = (frp_g4 *)p;
    g[0] = frp_v4{v.v[0], v.v[1], v.v[2], v.v[3]};
    g[1] = frp_v4{v.v[4], v.v[5], v.v[6], v.v[7]};
}

// slot t of the calling thread: the four 8-byte limb pairs of a value lie T = blockDim.x slots apart, the threads' copies side by side
__device__ __forceinline__ void frp_put(uint2 *lds, uint32_t T, uint32_t t, const Fr &v) {
#pragma unroll
    for (int k = 0; k < 4; k++) lds[(t * 4 + k) * T + threadIdx.x] = make_uint2(v.v[2 * k], v.v[2 * k + 1]);
}

__device__ __forceinline__ Fr frp_get(const uint2 *lds, uint32_t T, uint32_t t) {
    Fr v;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint2 w = lds[(t * 4 + k) * T + threadIdx.x];
        v.v[2 * k] = w.x;
        v.v[2 * k + 1] = w.y;
    }
    return v;
}

}  // namespace kzg
