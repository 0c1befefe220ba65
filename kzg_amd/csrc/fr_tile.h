// fr_tile.h -- a workgroup's tile of Fr elements between global memory and the threads' registers, through LDS.  Shared by the Horner
// kernels of poly.hip and the scans of fr_scan.hip.
//
// A thread owns EIGHT CONSECUTIVE elements (256 bytes), so direct loads / stores put the 64 lanes of an instruction 256 bytes apart --
// every instruction touched 64 lines for 16 bytes each (k_quotient_apply moved 64 MB in 59 us, k_horner_partials 32 MB in 38 us: 1.1
// and 0.9 TB/s).  Here lane l of an instruction moves the 16-byte chunk l of a run of whole lines (4 KiB with 256
// threads), and the thread's own 16 chunks sit in LDS at chunk index 17 t + j: the 272-byte stride spreads 16 lanes of a ds_read_b128
// over all 64 banks.
#pragma once
#include "field.h"

namespace kzg {

constexpr int HE = 8;            // elements per thread
typedef uint32_t __attribute__((ext_vector_type(4))) hchunk;   // 16 bytes: half an element

// LDS bytes of the tile of a workgroup of T threads: 16 chunks per thread and one pad chunk per thread segment
constexpr int tile_lds_bytes(int T) { return (T * 2 * HE + T) * 16; }

__device__ __forceinline__ uint32_t h_slot(uint32_t c) { return c + (c >> 4); }

// a[k] = base[tile * 8 T + 8 t + k] (zero beyond n) for thread t of the T = blockDim.x threads, through the LDS tile `lds`
// (tile_lds_bytes(T)).  Every thread of the workgroup calls it; a second call needs a barrier after the reads of the first.
__device__ __forceinline__ void load8_tile(const Fr *base, size_t n, size_t tile, int T, hchunk *lds, Fr a[HE]) {
    const int t = threadIdx.x;
    const size_t c0 = tile * (size_t)(T * 2 * HE), cn = n * 2;     // chunk indices; the array holds cn chunks
    const hchunk *g = (const hchunk *)base;
    hchunk v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const size_t c = c0 + (size_t)(t + j * T);
        v[j] = c < cn ? g[c] : hchunk{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 16; j++) lds[h_slot(t + j * T)] = v[j];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < HE; k++) {
        const hchunk lo = lds[17 * t + 2 * k], hi = lds[17 * t + 2 * k + 1];
        a[k].v[0] = lo.x; a[k].v[1] = lo.y; a[k].v[2] = lo.z; a[k].v[3] = lo.w;
        a[k].v[4] = hi.x; a[k].v[5] = hi.y; a[k].v[6] = hi.z; a[k].v[7] = hi.w;
    }
}

// the store twin: every thread puts its eight results into the tile (after a barrier behind the tile's last use), a barrier, then
// store8_tile writes base[tile * 8 T + i] for the elements below n in whole lines
__device__ __forceinline__ void tile_put(hchunk *lds, int t, int k, const Fr &out) {
    lds[17 * t + 2 * k] = hchunk{out.v[0], out.v[1], out.v[2], out.v[3]};
    lds[17 * t + 2 * k + 1] = hchunk{out.v[4], out.v[5], out.v[6], out.v[7]};
}
__device__ __forceinline__ void store8_tile(Fr *base, size_t n, size_t tile, int T, const hchunk *lds) {
    const int t = threadIdx.x;
    const size_t c0 = tile * (size_t)(T * 2 * HE), cn = n * 2;
    hchunk *g = (hchunk *)base;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const size_t cc = c0 + (size_t)(t + j * T);
        if (cc < cn) g[cc] = lds[h_slot(t + j * T)];
    }
}

}  // namespace kzg
