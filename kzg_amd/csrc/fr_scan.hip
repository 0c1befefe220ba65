// fr_scan.hip -- scans over Fr with a variable operand, and the public batch inversion (not reference methods):
//   kzg_fr_scan            running products / sums of `batch` vectors
//   kzg_fr_grand_product   the permutation / lookup accumulator z_i = prod_{k < i} N_k / D_k, N_k = prod_j num_j[k], D_k = prod_j den_j[k]
//   kzg_fr_batch_inverse   k_batch_inverse of poly.hip behind a C call
//
// A scan is a blocked scan in THREE launches per chunk of vectors: tile partials, a carry scan over the partials of each vector (one
// workgroup per vector), apply.  Kernel boundaries are the only synchronisation between workgroups.  The vector is blockIdx.y of the
// tile kernels and blockIdx.x of the carry kernel: the launches do not multiply with the batch.
//
// The tile is poly.hip's: a thread owns eight consecutive elements, and the tile moves through LDS in whole 16-byte chunks
// (fr_tile.h).  The operator is the Montgomery product of field.h (or add) with variable operands.  Products are formed in Montgomery
// form whatever the data's format: a canonical word becomes Montgomery at the tile load (one product with R^2, which takes any
// 256-bit word to a residue), and the way back costs ONE product per thread, not eight: the thread's exclusive prefix p R goes to p,
// and p times Montgomery elements stays canonical.  Sums need no conversion (canonical words go to their residue at the load).
//
// The grand product does not invert per element:
//   z_i = (prod_{k < i} N_k) (prod_{k >= i} D_k) (prod_all D)^-1
// an exclusive prefix product of N, an inclusive suffix product of D and one field inversion per vector, in the carry kernel, where
// prod_all D == 0 is the zero-denominator flag; the inverse (zero for a zero product) rides in front of the prefix carries, so such a
// vector's row and total come out zero with no branch.  N and D are formed from the t columns as the tiles are loaded (canonical
// columns: the chain starts from R^(t+1), so t products leave the Montgomery form of the product) and are never written to memory.
#include <algorithm>

#include "common.h"
#include "fr_tile.h"

namespace kzg {

struct OpMul {
    static __device__ __forceinline__ Fr id() { return Fr::one(); }
    static __device__ __forceinline__ Fr ap(const Fr &a, const Fr &b) { return mul(a, b); }
    static __device__ __forceinline__ Fr lift(const Fr &a, int canon) { return canon ? mul(a, Fr::r2()) : a; }   // caller's word -> operand
    static __device__ __forceinline__ Fr lower(const Fr &a, int canon) { return canon ? from_mont(a) : a; }     // operand -> caller's form
};
struct OpAdd {
    static __device__ __forceinline__ Fr id() { return Fr::zero(); }
    static __device__ __forceinline__ Fr ap(const Fr &a, const Fr &b) { return add(a, b); }
    static __device__ __forceinline__ Fr lift(const Fr &a, int canon) { return canon ? fr_residue(a) : a; }
    static __device__ __forceinline__ Fr lower(const Fr &a, int) { return a; }
};

// one value per thread in LDS, limb-major (conflict-free 32-bit accesses)
__device__ __forceinline__ void fs_put(uint32_t *sh, int T, int t, const Fr &v) {
#pragma unroll
    for (int i = 0; i < 8; i++) sh[i * T + t] = v.v[i];
}
__device__ __forceinline__ Fr fs_get(const uint32_t *sh, int T, int t) {
    Fr v;
#pragma unroll
    for (int i = 0; i < 8; i++) v.v[i] = sh[i * T + t];
    return v;
}

// the (op) of the T threads' values, in thread 0.  T a power of two; a step's writers (slots below off) and readers (slots off ..
// 2 off - 1) are disjoint: one barrier per step.
template <class OP>
__device__ __forceinline__ Fr block_reduce(Fr v, uint32_t *sh, int T) {
    const int t = threadIdx.x;
    fs_put(sh, T, t, v);
    __syncthreads();
    for (int off = T >> 1; off > 0; off >>= 1) {
        if (t < off) {
            v = OP::ap(v, fs_get(sh, T, t + off));
            fs_put(sh, T, t, v);
        }
        __syncthreads();
    }
    return v;
}

// inclusive scan over the threads (REV: from thread T - 1 down), left in sh[0, 8 T) behind a barrier
template <class OP, bool REV>
__device__ __forceinline__ void block_scan(Fr v, uint32_t *sh, int T) {
    const int t = threadIdx.x;
    fs_put(sh, T, t, v);
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        const int o = REV ? t + off : t - off;
        const bool has = REV ? o < T : o >= 0;
        Fr x = OP::id();
        if (has) x = fs_get(sh, T, o);
        __syncthreads();
        if (has) {
            v = OP::ap(v, x);
            fs_put(sh, T, t, v);
        }
        __syncthreads();
    }
}

template <class OP>
__device__ __forceinline__ Fr reduce8(const Fr a[HE]) {
    Fr v = a[0];
#pragma unroll
    for (int k = 1; k < HE; k++) v = OP::ap(v, a[k]);
    return v;
}

// The carry scan of one vector by one workgroup of T = blockDim.x threads (a power of two), g = ceil(nblk / T) partials per thread:
// C[i] = first (op) S[0] (op) ... (op) S[i - 1] (REV: the same from the far end, C[i] = first (op) S[nblk - 1] ... S[i + 1]); returns
// first (op) all of S in every thread.  sh: 8 T words, free again on return.  C and S do not alias.
template <class OP, bool REV>
__device__ __forceinline__ Fr carry_scan(const Fr *S, uint32_t nblk, const Fr &first, Fr *C, uint32_t *sh) {
    const int t = threadIdx.x, T = blockDim.x;
    const uint32_t g = (nblk + T - 1) / T, r0 = (uint32_t)t * g;
    Fr v = OP::id();
    for (uint32_t k = 0; k < g; k++) {
        const uint32_t r = r0 + k;
        if (r < nblk) {
            const Fr s = S[REV ? nblk - 1 - r : r];
            v = k ? OP::ap(v, s) : s;
        }
    }
    if (t == 0) v = OP::ap(first, v);
    block_scan<OP, false>(v, sh, T);
    Fr carry = t ? fs_get(sh, T, t - 1) : first;
    const Fr total = fs_get(sh, T, T - 1);
    __syncthreads();
    for (uint32_t k = 0; k < g; k++) {
        const uint32_t r = r0 + k;
        if (r < nblk) {
            const uint32_t i = REV ? nblk - 1 - r : r;
            C[i] = carry;
            carry = OP::ap(carry, S[i]);
        }
    }
    return total;
}

constexpr int FS_CARRY_T = 512;   // threads of the carry kernels, at most (k_horner_scan's measured choice)

// ---------------------------------------------------------------------------------------------
// kzg_fr_scan
// ---------------------------------------------------------------------------------------------
struct ScanArgs {
    const Fr *in;      // the chunk's vectors, n apart
    Fr *out;           // may be `in`: a workgroup reads its whole tile before it writes
    size_t n;
    uint32_t nblk;     // tiles per vector
    int canon, exclusive;
    Fr *S, *C;         // per vector nblk tile partials / exclusive carries (operands)
    Fr *tot;           // per vector: the (op) of all n elements, in the caller's form
};

template <class OP>
__device__ __forceinline__ void scan_load(const ScanArgs &p, hchunk *lds, Fr a[HE]) {
    load8_tile(p.in + (size_t)blockIdx.y * p.n, p.n, blockIdx.x, blockDim.x, lds, a);
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * HE;
#pragma unroll
    for (int k = 0; k < HE; k++) {
        if (i0 + k < p.n) a[k] = OP::lift(a[k], p.canon);
        else a[k] = OP::id();
    }
}

template <class OP>
__global__ __launch_bounds__(256) void k_frscan_partials(ScanArgs p) {
    extern __shared__ __attribute__((aligned(16))) hchunk fs_lds[];
    Fr a[HE];
    scan_load<OP>(p, fs_lds, a);
    Fr v = reduce8<OP>(a);
    __syncthreads();                 // the tile is consumed: its memory carries the tree
    v = block_reduce<OP>(v, (uint32_t *)fs_lds, blockDim.x);
    if (threadIdx.x == 0) p.S[(size_t)blockIdx.y * p.nblk + blockIdx.x] = v;
}

template <class OP>
__global__ __launch_bounds__(FS_CARRY_T) void k_frscan_carry(ScanArgs p) {
    __shared__ uint32_t sh[8 * FS_CARRY_T];
    const size_t b = blockIdx.x;
    const Fr total = carry_scan<OP, false>(p.S + b * p.nblk, p.nblk, OP::id(), p.C + b * p.nblk, sh);
    if (threadIdx.x == 0) p.tot[b] = OP::lower(total, p.canon);
}

template <class OP>
__global__ __launch_bounds__(256) void k_frscan_apply(ScanArgs p) {
    extern __shared__ __attribute__((aligned(16))) hchunk fs_lds[];
    const int t = threadIdx.x, T = blockDim.x;
    uint32_t *sh = (uint32_t *)fs_lds;
    Fr a[HE];
    scan_load<OP>(p, fs_lds, a);
    Fr v = reduce8<OP>(a);
    const Fr cb = p.C[(size_t)blockIdx.y * p.nblk + blockIdx.x];
    if (t == 0) v = OP::ap(cb, v);   // the carry from the tiles before rides in thread 0's value
    __syncthreads();                 // every thread has read its elements: the tile's memory carries the scan
    block_scan<OP, false>(v, sh, T);
    Fr pre = t ? fs_get(sh, T, t - 1) : cb;
    __syncthreads();
    pre = OP::lower(pre, p.canon);   // (a canonical prefix times Montgomery elements stays canonical)
#pragma unroll
    for (int k = 0; k < HE; k++) {
        if (p.exclusive) {
            tile_put(fs_lds, t, k, pre);
            if (k < HE - 1) pre = OP::ap(pre, a[k]);
        } else {
            pre = OP::ap(pre, a[k]);
            tile_put(fs_lds, t, k, pre);
        }
    }
    __syncthreads();
    store8_tile(p.out + (size_t)blockIdx.y * p.n, p.n, blockIdx.x, T, fs_lds);
}

// ---------------------------------------------------------------------------------------------
// kzg_fr_grand_product
// ---------------------------------------------------------------------------------------------
struct GrandArgs {
    const Fr *num, *den;   // the chunk's vectors: t columns of n each, vectors t n apart
    Fr *z;                 // the chunk's rows, n apart
    size_t n, t;
    uint32_t nblk;
    int canon;
    Fr c0;                 // canonical columns: R^(t+1), the start of a column chain
    Fr *SN, *SD, *CN, *CD; // per vector nblk tile products of N / D, the prefix carries of N (times 1 / prod D) and the suffix carries of D
    Fr *tot;               // per vector prod N / prod D in the caller's form
    int *zflag;            // per vector: prod D == 0
};

// X[k] = prod_j col[j n + tile element k] in Montgomery form, one for the elements beyond n
__device__ __forceinline__ void grand_cols(const GrandArgs &p, const Fr *col, bool later, hchunk *lds, Fr X[HE]) {
    for (size_t j = 0; j < p.t; j++) {
        if (later || j) __syncthreads();     // the reads of the column before are done
        Fr a[HE];
        load8_tile(col + j * p.n, p.n, blockIdx.x, blockDim.x, lds, a);
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < HE; k++) X[k] = p.canon ? mul(p.c0, a[k]) : a[k];
        } else {
#pragma unroll
            for (int k = 0; k < HE; k++) X[k] = mul(X[k], a[k]);
        }
    }
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * HE;
#pragma unroll
    for (int k = 0; k < HE; k++)
        if (i0 + k >= p.n) X[k] = Fr::one();
}

__global__ __launch_bounds__(256) void k_grand_partials(GrandArgs p) {
    extern __shared__ __attribute__((aligned(16))) hchunk fs_lds[];
    uint32_t *sh = (uint32_t *)fs_lds;
    const size_t b = blockIdx.y;
    Fr X[HE];
    grand_cols(p, p.num + b * p.t * p.n, false, fs_lds, X);
    Fr vn = reduce8<OpMul>(X);
    grand_cols(p, p.den + b * p.t * p.n, true, fs_lds, X);
    Fr vd = reduce8<OpMul>(X);
    __syncthreads();
    vn = block_reduce<OpMul>(vn, sh, blockDim.x);
    vd = block_reduce<OpMul>(vd, sh, blockDim.x);   // (the tree of vn ended in a barrier)
    if (threadIdx.x == 0) {
        p.SN[b * p.nblk + blockIdx.x] = vn;
        p.SD[b * p.nblk + blockIdx.x] = vd;
    }
}

__global__ __launch_bounds__(FS_CARRY_T) void k_grand_carry(GrandArgs p) {
    __shared__ uint32_t sh[8 * FS_CARRY_T];
    const int t = threadIdx.x, T = blockDim.x;
    const size_t b = blockIdx.x;
    const Fr totd = carry_scan<OpMul, true>(p.SD + b * p.nblk, p.nblk, Fr::one(), p.CD + b * p.nblk, sh);
    if (t == 0) {                        // the one inversion of the vector; zero maps to zero
        Fr iv = inv(totd);
        if (p.canon) iv = from_mont(iv);
        fs_put(sh, T, 0, iv);
        p.zflag[b] = totd.is_zero() ? 1 : 0;
    }
    __syncthreads();
    const Fr first = fs_get(sh, T, 0);
    __syncthreads();
    const Fr total = carry_scan<OpMul, false>(p.SN + b * p.nblk, p.nblk, first, p.CN + b * p.nblk, sh);
    if (t == 0) p.tot[b] = total;
}

__global__ __launch_bounds__(256) void k_grand_apply(GrandArgs p) {
    extern __shared__ __attribute__((aligned(16))) hchunk fs_lds[];
    uint32_t *sh = (uint32_t *)fs_lds;
    const int t = threadIdx.x, T = blockDim.x;
    const size_t b = blockIdx.y;
    Fr N[HE], D[HE];
    grand_cols(p, p.num + b * p.t * p.n, false, fs_lds, N);
    grand_cols(p, p.den + b * p.t * p.n, true, fs_lds, D);
    Fr vn = reduce8<OpMul>(N), vd = reduce8<OpMul>(D);
    const Fr cn = p.CN[b * p.nblk + blockIdx.x], cd = p.CD[b * p.nblk + blockIdx.x];
    if (t == 0) vn = mul(cn, vn);
    if (t == T - 1) vd = mul(vd, cd);
    __syncthreads();
    block_scan<OpMul, false>(vn, sh, T);
    Fr pn = t ? fs_get(sh, T, t - 1) : cn;           // (prod_{k < 8 t} N_k) / prod_all D, tiles before included
    __syncthreads();
    block_scan<OpMul, true>(vd, sh, T);
    const Fr sd = t + 1 < T ? fs_get(sh, T, t + 1) : cd;   // prod_{k >= 8 t + 8} D_k
    __syncthreads();
    D[HE - 1] = mul(D[HE - 1], sd);
#pragma unroll
    for (int k = HE - 2; k >= 0; k--) D[k] = mul(D[k], D[k + 1]);
#pragma unroll
    for (int k = 0; k < HE; k++) {
        tile_put(fs_lds, t, k, mul(pn, D[k]));
        if (k < HE - 1) pn = mul(pn, N[k]);
    }
    __syncthreads();
    store8_tile(p.z + b * p.n, p.n, blockIdx.x, T, fs_lds);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr size_t FS_STAGE_BYTES = (size_t)64 << 20;   // host data is staged in pieces of at most this (the FOLD_STAGE_BYTES convention)
constexpr size_t FS_MAX_N = (size_t)1 << 28;

struct ScanShape {
    int T;            // threads of a tile workgroup
    uint32_t nblk;    // tiles per vector
    uint32_t Tc;      // threads of the carry workgroup
    size_t VC;        // vectors per chunk
    size_t stage;
};

// per_vec_host: bytes of one vector's host-side data that a chunk stages (0: nothing is staged)
static ScanShape scan_shape(const kzg_ctx *ctx, size_t n, size_t batch, size_t per_vec_host) {
    ScanShape s;
    const size_t tile = ctx->opt_fr_scan_tile ? (size_t)ctx->opt_fr_scan_tile : 2048;
    s.T = (int)(tile / HE);
    s.nblk = (uint32_t)((n + tile - 1) / tile);
    s.Tc = 64;
    while (s.Tc < (uint32_t)FS_CARRY_T && s.Tc < s.nblk) s.Tc *= 2;
    s.stage = ctx->opt_fr_scan_stage ? (size_t)ctx->opt_fr_scan_stage : FS_STAGE_BYTES;
    s.VC = std::min<size_t>({batch, (size_t)65535, std::max<size_t>(1, 65536 / s.nblk)});   // (gridDim.y; the partials' workspace)
    if (ctx->opt_fr_scan_chunk) s.VC = std::min<size_t>(s.VC, (size_t)ctx->opt_fr_scan_chunk);
    if (per_vec_host) s.VC = std::min<size_t>(s.VC, std::max<size_t>(1, s.stage / per_vec_host));
    return s;
}

static int scan_attrs(kzg_ctx *ctx) {
    if (ctx->attr_frscan_set) return KZG_OK;
    const int lds = tile_lds_bytes(256);
    const void *fns[] = {(const void *)k_frscan_partials<OpMul>, (const void *)k_frscan_partials<OpAdd>, (const void *)k_frscan_apply<OpMul>,
                         (const void *)k_frscan_apply<OpAdd>,    (const void *)k_grand_partials,         (const void *)k_grand_apply};
    for (const void *f : fns) KZG_HIP_CHECK(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ctx->attr_frscan_set = true;
    return KZG_OK;
}

template <class OP>
static void scan_launch(kzg_ctx *ctx, hipStream_t st, const ScanShape &s, const ScanArgs &a, size_t G) {
    const int lds = tile_lds_bytes(s.T);
    KZG_LAUNCH(ctx, st, "k_frscan_partials", k_frscan_partials<OP>, dim3(s.nblk, (unsigned)G), s.T, lds, a);
    KZG_LAUNCH(ctx, st, "k_frscan_carry", k_frscan_carry<OP>, (unsigned)G, s.Tc, 0, a);
    KZG_LAUNCH(ctx, st, "k_frscan_apply", k_frscan_apply<OP>, dim3(s.nblk, (unsigned)G), s.T, lds, a);
}

static bool fs_sfmt_ok(int sfmt) { return sfmt == KZG_FR_MONT_LE_32 || sfmt == KZG_FR_CANONICAL_LE_32; }

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_fr_scan(kzg_ctx *ctx, const void *in, size_t n, size_t batch, int op, int exclusive, int sfmt, int flags, void *out,
                           void *totals) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_fr_scan";
    if (!fs_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (op != KZG_SCAN_PRODUCT && op != KZG_SCAN_SUM) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": unknown op");
    if (exclusive != 0 && exclusive != 1) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": exclusive must be 0 or 1");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (n > FS_MAX_N) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n > 2^28");
    if (batch > (SIZE_MAX >> 6) / n) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": batch x n too large");
    if (batch == 0) return KZG_OK;
    if (!in || !out) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL in or out");
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const ScanShape s = scan_shape(ctx, n, batch, in_dev && out_dev ? 0 : n * 32);
    KZG_TRY(scan_attrs(ctx));
    const size_t part = align_up(s.VC * s.nblk * 32, 256);
    KZG_TRY(lane_reserve(ctx, lane, (in_dev && out_dev ? 0 : align_up(s.VC * n * 32, 256)) + 2 * part + align_up(s.VC * 32, 256) + 65536));
    Fr *d_stage = in_dev && out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, s.VC * n * 32);
    ScanArgs a;
    a.S = (Fr *)lane_alloc(ctx, lane, part);
    a.C = (Fr *)lane_alloc(ctx, lane, part);
    a.tot = (Fr *)lane_alloc(ctx, lane, s.VC * 32);
    if ((!(in_dev && out_dev) && !d_stage) || !a.S || !a.C || !a.tot) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    a.n = n;
    a.nblk = s.nblk;
    a.canon = sfmt == KZG_FR_CANONICAL_LE_32;
    a.exclusive = exclusive;
    StreamDrain drain{st};
    for (size_t b0 = 0; b0 < batch; b0 += s.VC) {
        const size_t G = std::min(s.VC, batch - b0);
        if (in_dev) {
            a.in = (const Fr *)in + b0 * n;
        } else {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_stage, (const uint8_t *)in + b0 * n * 32, G * n * 32, hipMemcpyHostToDevice, st));
            a.in = d_stage;
        }
        a.out = out_dev ? (Fr *)out + b0 * n : d_stage;
        if (op == KZG_SCAN_PRODUCT) scan_launch<OpMul>(ctx, st, s, a, G);
        else scan_launch<OpAdd>(ctx, st, s, a, G);
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out + b0 * n * 32, d_stage, G * n * 32, hipMemcpyDeviceToHost, st));
        if (totals) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)totals + b0 * 32, a.tot, G * 32, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_fr_grand_product(kzg_ctx *ctx, const void *num, const void *den, size_t n, size_t t, size_t batch, int sfmt, int flags,
                                    void *z_out, void *totals, int *zero_den) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_fr_grand_product";
    if (!fs_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (t == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": t == 0");
    if (n > FS_MAX_N) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n > 2^28");
    if (t > (SIZE_MAX >> 6) / n || batch > (SIZE_MAX >> 6) / (t * n)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": batch x t x n too large");
    if (batch == 0) return KZG_OK;
    if (!num || !den || !z_out) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL num, den or z_out");
    std::vector<int> zf;
    try {  // (no exception may leave through the C ABI)
        zf.resize(batch);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the flags");
    }
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t colb = t * n * 32;       // one side of one vector
    const ScanShape s = scan_shape(ctx, n, batch, in_dev ? (out_dev ? 0 : n * 32) : 2 * colb);
    KZG_TRY(scan_attrs(ctx));
    const size_t part = align_up(s.VC * s.nblk * 32, 256);
    KZG_TRY(lane_reserve(ctx, lane, (in_dev ? 0 : 2 * align_up(s.VC * colb, 256)) + (out_dev ? 0 : align_up(s.VC * n * 32, 256)) + 4 * part +
                                        align_up(s.VC * 32, 256) + align_up(s.VC * sizeof(int), 256) + 65536));
    Fr *d_num = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, s.VC * colb);
    Fr *d_den = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, s.VC * colb);
    Fr *d_z = out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, s.VC * n * 32);
    GrandArgs a;
    a.SN = (Fr *)lane_alloc(ctx, lane, part);
    a.SD = (Fr *)lane_alloc(ctx, lane, part);
    a.CN = (Fr *)lane_alloc(ctx, lane, part);
    a.CD = (Fr *)lane_alloc(ctx, lane, part);
    a.tot = (Fr *)lane_alloc(ctx, lane, s.VC * 32);
    a.zflag = (int *)lane_alloc(ctx, lane, s.VC * sizeof(int));
    if ((!in_dev && (!d_num || !d_den)) || (!out_dev && !d_z) || !a.SN || !a.SD || !a.CN || !a.CD || !a.tot || !a.zflag)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    a.n = n;
    a.t = t;
    a.nblk = s.nblk;
    a.canon = sfmt == KZG_FR_CANONICAL_LE_32;
    a.c0 = Fr::one();
    if (a.canon) {                      // R^(t+1) = the Montgomery form of R^t
        Fr e = Fr::r2();
        for (size_t tt = t; tt; tt >>= 1) {
            if (tt & 1) a.c0 = mul(a.c0, e);
            e = sqr(e);
        }
    }
    const int lds = tile_lds_bytes(s.T);
    StreamDrain drain{st};
    for (size_t b0 = 0; b0 < batch; b0 += s.VC) {
        const size_t G = std::min(s.VC, batch - b0);
        if (in_dev) {
            a.num = (const Fr *)num + b0 * t * n;
            a.den = (const Fr *)den + b0 * t * n;
        } else {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_num, (const uint8_t *)num + b0 * colb, G * colb, hipMemcpyHostToDevice, st));
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_den, (const uint8_t *)den + b0 * colb, G * colb, hipMemcpyHostToDevice, st));
            a.num = d_num;
            a.den = d_den;
        }
        a.z = out_dev ? (Fr *)z_out + b0 * n : d_z;
        KZG_LAUNCH(ctx, st, "k_grand_partials", k_grand_partials, dim3(s.nblk, (unsigned)G), s.T, lds, a);
        KZG_LAUNCH(ctx, st, "k_grand_carry", k_grand_carry, (unsigned)G, s.Tc, 0, a);
        KZG_LAUNCH(ctx, st, "k_grand_apply", k_grand_apply, dim3(s.nblk, (unsigned)G), s.T, lds, a);
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)z_out + b0 * n * 32, d_z, G * n * 32, hipMemcpyDeviceToHost, st));
        if (totals) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)totals + b0 * 32, a.tot, G * 32, hipMemcpyDeviceToHost, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(zf.data() + b0, a.zflag, G * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    bool any = false;
    for (size_t b = 0; b < batch; b++) {
        if (zero_den) zero_den[b] = zf[b];
        any = any || zf[b];
    }
    if (any && !zero_den) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a zero denominator (reference: invert().unwrap() panics)");
    return KZG_OK;
}

extern "C" int kzg_fr_batch_inverse(kzg_ctx *ctx, const void *in, size_t n, int sfmt, int flags, void *out, size_t *zeros) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_fr_batch_inverse";
    if (!fs_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n == 0");
    if (n > FS_MAX_N) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n > 2^28");
    if (!in || !out) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL in or out");
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t stage = ctx->opt_fr_scan_stage ? (size_t)ctx->opt_fr_scan_stage : FS_STAGE_BYTES;
    const size_t CE = std::min(n, stage / 32);                     // elements per piece
    const bool both_dev = in_dev && out_dev;
    // the running products of a piece go to its output, or to scratch where the output is the input (in == out on the device; host
    // to host, staged in place)
    const bool need_pre = both_dev ? in == out : (!in_dev && !out_dev);
    KZG_TRY(lane_reserve(ctx, lane, (both_dev ? 0 : align_up(CE * 32, 256)) + (need_pre ? align_up(CE * 32, 256) : 0) + 65536));
    Fr *d_stage = both_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, CE * 32);
    Fr *d_pre = need_pre ? (Fr *)lane_alloc(ctx, lane, CE * 32) : nullptr;
    unsigned long long *d_zero = (unsigned long long *)lane_alloc(ctx, lane, 256);
    if ((!both_dev && !d_stage) || (need_pre && !d_pre) || !d_zero) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_zero, 0, 8, st));
    for (size_t i0 = 0; i0 < n; i0 += CE) {
        const size_t cnt = std::min(CE, n - i0);
        const Fr *src = (const Fr *)in + i0;
        if (!in_dev) {
            KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_stage, src, cnt * 32, hipMemcpyHostToDevice, st));
            src = d_stage;
        }
        Fr *dst = out_dev ? (Fr *)out + i0 : d_stage;
        KZG_TRY(batch_inverse_pub(ctx, st, src, dst, need_pre ? d_pre : dst, cnt, sfmt == KZG_FR_CANONICAL_LE_32, d_zero));
        if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out + i0 * 32, d_stage, cnt * 32, hipMemcpyDeviceToHost, st));
    }
    unsigned long long z = 0;
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(&z, d_zero, 8, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    if (zeros) *zeros = (size_t)z;
    return KZG_OK;
}
