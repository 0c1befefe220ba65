// mle.hip -- the rounds of a sumcheck prover on the device (not reference methods):
//   kzg_mle_eq              the table eq(point, .) over the hypercube, by doubling: one product per element
//   kzg_mle_bind            every column of a set folded at its top variable with one challenge, one launch, in place or not
//   kzg_mle_eval            multilinear evaluation of `batch` tables, optionally with the Zeromorph quotients of every level
//   kzg_fr_program_degree   the degree bound of a plan's outputs (host only)
//   kzg_sumcheck_round      sum over the pairs (i, i + n / 2) of a plan's outputs at X = 0 .. n_eval - 1
//
// Conventions: a multilinear polynomial in m variables is a table f of n = 2^m scalars, f[i] its value at the corner whose coordinate
// x_j is bit j of i.  Rounds bind the TOP variable: with h = n / 2, lo = f[0, h) is x_{m-1} = 0 and hi = f[h, n) is x_{m-1} = 1, and
// binding to rho gives lo[i] + rho (hi[i] - lo[i]) in h elements.  Lane i reads i and i + h and writes i: in place without a race,
// and a wave reads whole lines.  point[j] belongs to variable j, so round k of a sumcheck fixes point[m - 1 - k].
//
// Formats are those of kzg_fr_scan.  eq, the sumcheck round and their consts compute in Montgomery form whatever the data's format
// (canonical data pays one product per column operand and one per result).  bind and eval are LINEAR in the data: a Montgomery
// challenge times a canonical difference is the canonical product, so canonical words are only reduced below r on their first load.
//
// k_sumcheck_round is the interpreter of k_fr_program (fr_program.hip) with three changes: a lane owns a pair index and strides over
// the pairs on a bounded grid; a column operand at X comes from the two loads of the pair (X = 0: lo, X = 1: hi, above: hi plus
// X - 1 times hi - lo by repeated addition, no product); a store to output o becomes acc[o][X] += d.  The accumulators are indexed by
// run-time values, so they live in LDS behind the temporaries in the same conflict-free layout: (n_temps + n_out n_eval) x 32 x T
// bytes a workgroup.  The row is the outer loop, X the inner: a column element comes from HBM once, the repeats within a row hit the
// cache.  Lanes beyond h walk the stream on the last pair (uniform branches) and their accumulation is masked.  Field addition is
// exact, so the reduction is deterministic: every slot is summed across the wave by cross-lane moves, one lane per wave writes a
// partial, and k_sumcheck_finish adds the partials of each slot -- no atomics on field elements.
#include <algorithm>
#include <new>

#include "common.h"
#include "fr_program.h"
#include "mle_host.h"

namespace kzg {

constexpr size_t MLE_MAX_LOG = 28, MLE_MAX_COLS = 4096;
constexpr int MLE_LOCAL_LOG = 10;                    // tables of up to 2^10 scalars (32 KiB) are worked inside one workgroup's LDS
constexpr int SUMCHECK_LDS_MAX = 128 * 1024;         // (16 + 32) slots at 64 threads take 96 KiB
constexpr size_t SUMCHECK_MAX_BLOCKS = 65536;

struct MleCol {
    const Fr *in;
    Fr *out;
};

// ---- eq ------------------------------------------------------------------------------------------------------------------------------
// levels 0 .. L0 - 1 in LDS: t[i + 2^j] = t[i] u_j, t[i] -= t[i + 2^j]; one workgroup.  pt: Montgomery, read at uniform addresses
template <bool CANON_OUT>
__global__ __launch_bounds__(256) void k_mle_eq_local(const Fr *__restrict__ pt, uint32_t L0, Fr *__restrict__ out) {
    __shared__ Fr t[1 << MLE_LOCAL_LOG];
    if (threadIdx.x == 0) t[0] = Fr::one();
    __syncthreads();
    for (uint32_t j = 0; j < L0; j++) {
        const Fr u = pt[j];
        const uint32_t half = 1u << j;
        for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
            const Fr a = t[i], b = mul(a, u);
            t[i + half] = b;
            t[i] = sub(a, b);
        }
        __syncthreads();
    }
    const uint32_t size = 1u << L0;
    for (uint32_t i = threadIdx.x; i < size; i += blockDim.x) frp_store(out + i, CANON_OUT ? from_mont(t[i]) : t[i]);
}

// one level in global memory, in place: lane i < half reads t[i], writes t[i + half] and t[i]
template <bool CANON_OUT>
__global__ __launch_bounds__(256) void k_mle_eq_level(const Fr *__restrict__ u_ptr, uint32_t half, Fr *t) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const Fr u = *u_ptr;  // uniform
    const Fr a = frp_load(t + i), b = mul(a, u), lo = sub(a, b);
    frp_store(t + i + half, CANON_OUT ? from_mont(b) : b);
    frp_store(t + i, CANON_OUT ? from_mont(lo) : lo);
}

// ---- bind ----------------------------------------------------------------------------------------------------------------------------
// grid (ceil(h / T), n_cols): out_c[i] = in_c[i] + rho (in_c[i + h] - in_c[i]); rho Montgomery, wave-uniform
template <bool CANON>
__global__ __launch_bounds__(256) void k_mle_bind(const MleCol *__restrict__ cols, const Fr *__restrict__ rho, uint32_t h) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h) return;
    const MleCol c = cols[blockIdx.y];  // uniform
    const Fr r = *rho;
    Fr lo = frp_load(c.in + i), hi = frp_load(c.in + i + h);
    if (CANON) {
        lo = fr_residue(lo);
        hi = fr_residue(hi);
    }
    frp_store(c.out + i, add(lo, mul(r, sub(hi, lo))));
}

// ---- eval ----------------------------------------------------------------------------------------------------------------------------
// grid (ceil(h / T), tables): one level of every table of a chunk, table b at src + b src_stride, its h results at dst + b dst_stride
// (src == dst from the second level on); q (optional): the h differences at q + b q_stride + h - 1
template <bool RESIDUE>
__global__ __launch_bounds__(256) void k_mle_eval_level(const Fr *src, size_t src_stride, Fr *dst, size_t dst_stride, const Fr *__restrict__ u_ptr,
                                                        uint32_t h, Fr *q, size_t q_stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h) return;
    const size_t b = blockIdx.y;
    const Fr u = *u_ptr;  // uniform
    const Fr *s = src + b * src_stride;
    Fr lo = frp_load(s + i), hi = frp_load(s + i + h);
    if (RESIDUE) {
        lo = fr_residue(lo);
        hi = fr_residue(hi);
    }
    const Fr d = sub(hi, lo);
    if (q) frp_store(q + b * q_stride + (h - 1) + i, d);
    frp_store(dst + b * dst_stride + i, add(lo, mul(u, d)));
}

// one workgroup per table: the last k <= MLE_LOCAL_LOG levels in LDS, the value to ys[b]
template <bool RESIDUE>
__global__ __launch_bounds__(256) void k_mle_eval_tail(const Fr *__restrict__ src, size_t src_stride, const Fr *__restrict__ pt, uint32_t k, Fr *q,
                                                       size_t q_stride, Fr *__restrict__ ys) {
    __shared__ Fr t[1 << MLE_LOCAL_LOG];
    const size_t b = blockIdx.x;
    const uint32_t size = 1u << k;
    for (uint32_t i = threadIdx.x; i < size; i += blockDim.x) {
        const Fr v = frp_load(src + b * src_stride + i);
        t[i] = RESIDUE ? fr_residue(v) : v;
    }
    __syncthreads();
    for (uint32_t lvl = k; lvl-- > 0;) {
        const uint32_t h = 1u << lvl;
        const Fr u = pt[lvl];
        for (uint32_t i = threadIdx.x; i < h; i += blockDim.x) {   // a thread writes only the t[i] it has read itself
            const Fr lo = t[i], d = sub(t[i + h], lo);
            if (q) frp_store(q + b * q_stride + (h - 1) + i, d);
            t[i] = add(lo, mul(u, d));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) frp_store(ys + b, t[0]);
}

// ---- the round -----------------------------------------------------------------------------------------------------------------------
template <bool CANON>
__device__ __forceinline__ Fr sc_fetch(const Fr *const *__restrict__ cols, const Fr *__restrict__ consts, uint32_t kind, uint32_t idx, uint32_t row,
                                       uint32_t h, uint32_t X, const uint2 *lds) {
    if (kind == KZG_FRP_COL) {
        const Fr *p = cols[idx];   // uniform
        Fr v;
        if (X == 0) {
            v = frp_load(p + row);
            if (CANON) v = fr_residue(v);
        } else {
            Fr hi = frp_load(p + row + h);
            if (CANON) hi = fr_residue(hi);
            v = hi;
            if (X > 1) {
                Fr lo = frp_load(p + row);
                if (CANON) lo = fr_residue(lo);
                const Fr d = sub(hi, lo);
                for (uint32_t k = 1; k < X; k++) v = add(v, d);
            }
        }
        return CANON ? mul(v, Fr::r2()) : v;
    }
    if (kind == KZG_FRP_CONST) return consts[idx];   // uniform: out of SGPRs
    return frp_get(lds, blockDim.x, idx);
}

// grid: at most ceil(h / T) workgroups of T threads; dynamic LDS 32 (n_temps + n_acc) T bytes, n_acc = n_out n_eval.  partial: one row
// of n_acc sums per wave of the grid.  prog as validated (no shifts), consts Montgomery, cols: n_cols pointers to n = 2 h elements
template <bool CANON>
__global__ __launch_bounds__(256) void k_sumcheck_round(const uint32_t *__restrict__ prog, const Fr *const *__restrict__ cols,
                                                        const Fr *__restrict__ consts, uint32_t n_insns, uint32_t h, uint32_t n_eval, uint32_t n_temps,
                                                        uint32_t n_acc, Fr *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint2 sc_lds[];
    const uint32_t T = blockDim.x;
    for (uint32_t s = 0; s < n_acc; s++) frp_put(sc_lds, T, n_temps + s, Fr::zero());
    for (uint32_t base = blockIdx.x * T; base < h; base += gridDim.x * T) {   // uniform in the workgroup
        const uint32_t i = base + threadIdx.x;
        const bool live = i < h;
        const uint32_t row = live ? i : h - 1;
        for (uint32_t X = 0; X < n_eval; X++) {
            for (uint32_t pc = 0; pc < n_insns; pc++) {
                const uint32_t *__restrict__ w = prog + pc * KZG_FRP_WORDS;
                const uint32_t head = w[0], dst = w[1];
                const Fr a = sc_fetch<CANON>(cols, consts, (head >> 16) & 0xFF, w[2], row, h, X, sc_lds);
                const Fr b = sc_fetch<CANON>(cols, consts, head >> 24, w[3], row, h, X, sc_lds);
                const uint32_t op = head & 0xFF;
                Fr d;
                if (op == KZG_FRP_MUL) d = mul(a, b);
                else if (op == KZG_FRP_ADD) d = add(a, b);
                else d = sub(a, b);
                if (((head >> 8) & 0xFF) == KZG_FRP_TEMP) {
                    frp_put(sc_lds, T, dst, d);
                } else if (live) {
                    const uint32_t slot = n_temps + dst * n_eval + X;
                    frp_put(sc_lds, T, slot, add(frp_get(sc_lds, T, slot), d));
                }
            }
        }
    }
    const uint32_t lane = threadIdx.x & 63, wave = (blockIdx.x * T + threadIdx.x) >> 6;
    for (uint32_t s = 0; s < n_acc; s++) {
        Fr v = frp_get(sc_lds, T, n_temps + s);
        for (int off = 32; off > 0; off >>= 1) {
            Fr o;
#pragma unroll
            for (int k = 0; k < 8; k++) o.v[k] = (uint32_t)__shfl_down((int)v.v[k], off, 64);
            v = add(v, o);   // lanes whose partner lies beyond the wave add their own value: lane 0 never reads them
        }
        if (lane == 0) frp_store(partial + (size_t)wave * n_acc + s, v);
    }
}

// grid n_acc workgroups of 256: sums[s] = the sum over the `waves` partial rows of slot s
template <bool CANON>
__global__ __launch_bounds__(256) void k_sumcheck_finish(const Fr *__restrict__ partial, uint32_t waves, uint32_t n_acc, Fr *__restrict__ sums) {
    __shared__ Fr red[256];
    const uint32_t s = blockIdx.x;
    Fr v = Fr::zero();
    for (uint32_t p = threadIdx.x; p < waves; p += 256) v = add(v, frp_load(partial + (size_t)p * n_acc + s));
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] = add(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) frp_store(sums + s, CANON ? from_mont(red[0]) : red[0]);
}

static int sumcheck_attrs(kzg_ctx *ctx) {
    if (ctx->attr_sumcheck_set) return KZG_OK;
    KZG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_sumcheck_round<false>, hipFuncAttributeMaxDynamicSharedMemorySize, SUMCHECK_LDS_MAX));
    KZG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_sumcheck_round<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SUMCHECK_LDS_MAX));
    ctx->attr_sumcheck_set = true;
    return KZG_OK;
}

// threads of a workgroup by the slots (temporaries + accumulators) a thread holds in LDS, the rule of frp_block; a forced size that
// would pass SUMCHECK_LDS_MAX is halved until it fits (48 slots fit at 64 threads)
static int sumcheck_block(const kzg_ctx *ctx, size_t slots) {
    int T = ctx->opt_sumcheck_block ? ctx->opt_sumcheck_block : slots <= 4 ? 256 : slots <= 8 ? 128 : 64;
    while (T > 64 && slots * 32 * (size_t)T > (size_t)SUMCHECK_LDS_MAX) T /= 2;
    return T;
}

static int mle_block(const kzg_ctx *ctx) { return ctx->opt_mle_block ? ctx->opt_mle_block : 256; }
static int mle_local_log(const kzg_ctx *ctx) { return ctx->opt_mle_local_log ? ctx->opt_mle_local_log : MLE_LOCAL_LOG; }

// a host scalar in sfmt, below r, as Montgomery
static bool mle_host_scalar(const void *p, bool canon, Fr *out) {
    Fr x;
    memcpy(x.v, p, 32);
    if (!is_canonical(x)) return false;
    *out = canon ? to_mont(x) : x;
    return true;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_mle_eq(kzg_ctx *ctx, const void *point, size_t m, int sfmt, int flags, void *out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_mle_eq";
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (m > MLE_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, who + ": m > 28");
    if (!out || (m && !point)) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL point or out");
    const bool canon = sfmt == KZG_FR_CANONICAL_LE_32, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    std::vector<Fr> pt;
    try {  // (no exception may leave through the C ABI)
        pt.resize(std::max<size_t>(m, 1));
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the point");
    }
    for (size_t j = 0; j < m; j++)
        if (!mle_host_scalar((const uint8_t *)point + j * 32, canon, &pt[j])) return fail(ctx, KZG_ERR_SHAPE, who + ": point[" + std::to_string(j) + "] is not below r");
    const size_t n = (size_t)1 << m;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_TRY(lane_reserve(ctx, lane, 65536 + (out_dev ? 0 : align_up(n * 32, 256))));
    Fr *d_pt = (Fr *)lane_alloc(ctx, lane, pt.size() * 32);
    Fr *d_t = out_dev ? (Fr *)out : (Fr *)lane_alloc(ctx, lane, n * 32);
    if (!d_pt || !d_t) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_pt, pt.data(), pt.size() * 32, hipMemcpyHostToDevice, st));
    const uint32_t L0 = (uint32_t)std::min<size_t>(m, (size_t)mle_local_log(ctx));
    const int T = mle_block(ctx);
    if (canon && L0 == m) KZG_LAUNCH(ctx, st, "k_mle_eq_local", k_mle_eq_local<true>, 1, T, 0, d_pt, L0, d_t);
    else KZG_LAUNCH(ctx, st, "k_mle_eq_local", k_mle_eq_local<false>, 1, T, 0, d_pt, L0, d_t);
    for (uint32_t j = L0; j < m; j++) {
        const uint32_t half = 1u << j;
        const unsigned blocks = (half + T - 1) / T;   // half <= 2^27, T >= 64: one grid
        if (canon && j + 1 == m) KZG_LAUNCH(ctx, st, "k_mle_eq_level", k_mle_eq_level<true>, blocks, T, 0, d_pt + j, half, d_t);
        else KZG_LAUNCH(ctx, st, "k_mle_eq_level", k_mle_eq_level<false>, blocks, T, 0, d_pt + j, half, d_t);
    }
    if (!out_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, d_t, n * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_mle_bind(kzg_ctx *ctx, const void *const *cols, size_t n_cols, size_t n, const void *rho, int sfmt, int flags,
                            void *const *outs) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_mle_bind";
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n < 2 || n > ((size_t)1 << MLE_MAX_LOG) || (n & (n - 1))) return fail(ctx, KZG_ERR_SHAPE, who + ": n is a power of two, 2 <= n <= 2^28");
    if (n_cols == 0 || n_cols > MLE_MAX_COLS) return fail(ctx, KZG_ERR_SHAPE, who + ": 1 <= n_cols <= 4,096");
    if (!cols || !outs || !rho) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL cols, outs or rho");
    for (size_t c = 0; c < n_cols; c++)
        if (!cols[c] || !outs[c]) return fail(ctx, KZG_ERR_SHAPE, who + ": a NULL column or output");
    const bool canon = sfmt == KZG_FR_CANONICAL_LE_32, in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const long clash = mle_bind_alias(cols, outs, n_cols, n, in_dev == out_dev);
    if (clash >= 0) return fail(ctx, KZG_ERR_SHAPE, who + ": output " + std::to_string(clash) + " overlaps a column or another output (only outs[c] == cols[c] is allowed)");
    Fr r;
    if (!mle_host_scalar(rho, canon, &r)) return fail(ctx, KZG_ERR_SHAPE, who + ": rho is not below r");
    const size_t h = n / 2, meta_bytes = 256 + align_up(n_cols * sizeof(MleCol), 256);
    std::vector<uint8_t> meta;
    try {  // (no exception may leave through the C ABI)
        meta.resize(meta_bytes);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the column table");
    }
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    size_t need = meta_bytes + 65536;
    if (!in_dev) need += n_cols * align_up(n * 32, 256);
    if (!out_dev && in_dev) need += n_cols * align_up(h * 32, 256);   // host columns are folded in place in their staged copy
    KZG_TRY(lane_reserve(ctx, lane, need));
    uint8_t *d_meta = (uint8_t *)lane_alloc(ctx, lane, meta_bytes);
    if (!d_meta) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    memcpy(meta.data(), &r, 32);
    MleCol *h_cols = (MleCol *)(meta.data() + 256);
    for (size_t c = 0; c < n_cols; c++) {
        h_cols[c].in = in_dev ? (const Fr *)cols[c] : (const Fr *)lane_alloc(ctx, lane, n * 32);
        h_cols[c].out = out_dev ? (Fr *)outs[c] : in_dev ? (Fr *)lane_alloc(ctx, lane, h * 32) : (Fr *)h_cols[c].in;
        if (!h_cols[c].in || !h_cols[c].out) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st));
    if (!in_dev)
        for (size_t c = 0; c < n_cols; c++) KZG_HIP_CHECK(ctx, hipMemcpyAsync((void *)h_cols[c].in, cols[c], n * 32, hipMemcpyHostToDevice, st));
    const int T = mle_block(ctx);
    const dim3 grid((unsigned)((h + T - 1) / T), (unsigned)n_cols);   // h <= 2^27, T >= 64; n_cols <= 4,096: one grid
    if (canon) KZG_LAUNCH(ctx, st, "k_mle_bind", k_mle_bind<true>, grid, T, 0, (const MleCol *)(d_meta + 256), (const Fr *)d_meta, (uint32_t)h);
    else KZG_LAUNCH(ctx, st, "k_mle_bind", k_mle_bind<false>, grid, T, 0, (const MleCol *)(d_meta + 256), (const Fr *)d_meta, (uint32_t)h);
    if (!out_dev)
        for (size_t c = 0; c < n_cols; c++) KZG_HIP_CHECK(ctx, hipMemcpyAsync(outs[c], h_cols[c].out, h * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_mle_eval(kzg_ctx *ctx, const void *tables, size_t m, size_t batch, const void *point, int sfmt, int flags, void *ys_out,
                            void *quotients_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_mle_eval";
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (m > MLE_MAX_LOG) return fail(ctx, KZG_ERR_SHAPE, who + ": m > 28");
    const size_t n = (size_t)1 << m;
    if (batch > ((size_t)-1 >> 6) / n) return fail(ctx, KZG_ERR_SHAPE, who + ": batch x n x 32 beyond size_t");
    if (batch == 0) return KZG_OK;
    if (!tables || !ys_out || (m && !point)) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL tables, point or ys_out");
    const bool canon = sfmt == KZG_FR_CANONICAL_LE_32, in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    std::vector<Fr> pt;
    try {  // (no exception may leave through the C ABI)
        pt.resize(std::max<size_t>(m, 1));
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the point");
    }
    for (size_t j = 0; j < m; j++)
        if (!mle_host_scalar((const uint8_t *)point + j * 32, canon, &pt[j])) return fail(ctx, KZG_ERR_SHAPE, who + ": point[" + std::to_string(j) + "] is not below r");
    const bool want_q = quotients_out != nullptr && m > 0;
    const size_t L = (size_t)mle_local_log(ctx);
    size_t B = std::min<size_t>(65535, std::max<size_t>(1, ((size_t)1 << 21) / n));
    if (ctx->opt_mle_eval_chunk) B = std::min<size_t>(B, (size_t)ctx->opt_mle_eval_chunk);
    B = std::min(B, batch);
    const bool levels = m > L;   // some levels run in global memory: the first goes from the input into the workspace
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    size_t need = 65536 + align_up(pt.size() * 32, 256) + align_up(B * 32, 256);
    if (!in_dev) need += align_up(B * n * 32, 256);
    if (levels) need += align_up(B * (n / 2) * 32, 256);
    if (want_q && !out_dev) need += align_up(B * (n - 1) * 32, 256);
    KZG_TRY(lane_reserve(ctx, lane, need));
    Fr *d_pt = (Fr *)lane_alloc(ctx, lane, pt.size() * 32);
    Fr *d_ys = (Fr *)lane_alloc(ctx, lane, B * 32);
    Fr *d_in = in_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, B * n * 32);
    Fr *d_ws = levels ? (Fr *)lane_alloc(ctx, lane, B * (n / 2) * 32) : nullptr;
    Fr *d_qs = want_q && !out_dev ? (Fr *)lane_alloc(ctx, lane, B * (n - 1) * 32) : nullptr;
    if (!d_pt || !d_ys || (!in_dev && !d_in) || (levels && !d_ws) || (want_q && !out_dev && !d_qs)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_pt, pt.data(), pt.size() * 32, hipMemcpyHostToDevice, st));
    const int T = mle_block(ctx);
    for (size_t b0 = 0; b0 < batch; b0 += B) {
        const size_t cnt = std::min(B, batch - b0);
        const Fr *src = in_dev ? (const Fr *)tables + b0 * n : d_in;
        if (!in_dev) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_in, (const uint8_t *)tables + b0 * n * 32, cnt * n * 32, hipMemcpyHostToDevice, st));
        Fr *q = !want_q ? nullptr : out_dev ? (Fr *)quotients_out + b0 * (n - 1) : d_qs;
        size_t stride = n, cur = m;
        bool first = true;
        while (cur > L) {   // the inputs are never written: the first level reads them and writes the workspace
            const uint32_t h = 1u << (cur - 1);
            const dim3 grid((h + T - 1) / T, (unsigned)cnt);
            if (canon && first) KZG_LAUNCH(ctx, st, "k_mle_eval_level", k_mle_eval_level<true>, grid, T, 0, src, stride, d_ws, n / 2, d_pt + (cur - 1), h, q, n - 1);
            else KZG_LAUNCH(ctx, st, "k_mle_eval_level", k_mle_eval_level<false>, grid, T, 0, src, stride, d_ws, n / 2, d_pt + (cur - 1), h, q, n - 1);
            src = d_ws;
            stride = n / 2;
            cur--;
            first = false;
        }
        if (canon && first) KZG_LAUNCH(ctx, st, "k_mle_eval_tail", k_mle_eval_tail<true>, (unsigned)cnt, T, 0, src, stride, d_pt, (uint32_t)cur, q, n - 1, d_ys);
        else KZG_LAUNCH(ctx, st, "k_mle_eval_tail", k_mle_eval_tail<false>, (unsigned)cnt, T, 0, src, stride, d_pt, (uint32_t)cur, q, n - 1, d_ys);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)ys_out + b0 * 32, d_ys, cnt * 32, hipMemcpyDeviceToHost, st));
        if (want_q && !out_dev)
            KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)quotients_out + b0 * (n - 1) * 32, d_qs, cnt * (n - 1) * 32, hipMemcpyDeviceToHost, st));
        KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));   // the chunk's buffers are reused
    }
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}

extern "C" int kzg_fr_program_degree(const kzg_fr_program *plan, size_t *degrees) {
    if (!plan || !degrees) return KZG_ERR_SHAPE;
    frp_degrees(plan->words.data(), plan->words.size() / KZG_FRP_WORDS, plan->n_out, degrees);
    return KZG_OK;
}

extern "C" int kzg_sumcheck_round(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const void *consts, size_t n, size_t n_eval,
                                  int sfmt, int flags, void *sums_out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_sumcheck_round";
    if (!plan) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL plan");
    if (plan->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, who + ": the plan belongs to another GPU");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n < 2 || n > ((size_t)1 << MLE_MAX_LOG) || (n & (n - 1))) return fail(ctx, KZG_ERR_SHAPE, who + ": n is a power of two, 2 <= n <= 2^28");
    const size_t NC = plan->n_cols, NK = plan->n_consts, NO = plan->n_out, NI = plan->words.size() / KZG_FRP_WORDS;
    if (!sumcheck_shape_ok(NO, n_eval)) return fail(ctx, KZG_ERR_SHAPE, who + ": 1 <= n_eval <= 16 and n_out x n_eval <= 32");
    if (frp_has_shift(plan->words.data(), NI)) return fail(ctx, KZG_ERR_SHAPE, who + ": the plan rotates a column (a shift has no meaning on the hypercube)");
    if ((NC && !cols) || (NK && !consts) || !sums_out) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL cols, consts or sums_out");
    for (size_t c = 0; c < NC; c++)
        if (!cols[c]) return fail(ctx, KZG_ERR_SHAPE, who + ": a NULL column");
    const bool canon = sfmt == KZG_FR_CANONICAL_LE_32, in_dev = (flags & KZG_IN_DEVICE) != 0;
    const size_t n_acc = NO * n_eval, slots = plan->n_temps + n_acc, h = n / 2;
    // what the kernel reads besides the columns, in one host buffer and one upload: program | column pointers | consts
    const size_t off_cols = align_up(NI * KZG_FRP_WORDS * 4, 256), off_consts = off_cols + align_up(NC * sizeof(Fr *), 256),
                 meta_bytes = off_consts + align_up(NK * 32, 256);
    std::vector<uint8_t> meta;
    try {  // (no exception may leave through the C ABI)
        meta.resize(meta_bytes);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the program");
    }
    Fr *h_consts = (Fr *)(meta.data() + off_consts);
    for (size_t k = 0; k < NK; k++)
        if (!mle_host_scalar((const uint8_t *)consts + k * 32, canon, &h_consts[k])) return fail(ctx, KZG_ERR_SHAPE, who + ": const " + std::to_string(k) + " is not below r");
    memcpy(meta.data(), plan->words.data(), NI * KZG_FRP_WORDS * 4);
    const int T = sumcheck_block(ctx, slots);
    const size_t lds = slots * 32 * (size_t)T;
    size_t blocks = (h + T - 1) / T;
    {   // the strided grid: what the chip holds at once by LDS and wave slots (160 KiB and 32 waves a CU), or option sumcheck_grid
        const size_t per_cu = std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds, 2048 / (size_t)T));
        const size_t cap = ctx->opt_sumcheck_grid ? (size_t)ctx->opt_sumcheck_grid : per_cu * (size_t)ctx->num_cus;
        blocks = std::min(blocks, std::min(cap, SUMCHECK_MAX_BLOCKS));
    }
    const size_t waves = blocks * (size_t)T / 64;
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_TRY(sumcheck_attrs(ctx));
    size_t need = meta_bytes + 65536 + align_up(waves * n_acc * 32, 256) + align_up(n_acc * 32, 256);
    if (!in_dev) need += NC * align_up(n * 32, 256);
    KZG_TRY(lane_reserve(ctx, lane, need));
    uint8_t *d_meta = (uint8_t *)lane_alloc(ctx, lane, meta_bytes);
    Fr *d_partial = (Fr *)lane_alloc(ctx, lane, waves * n_acc * 32);
    Fr *d_sums = (Fr *)lane_alloc(ctx, lane, n_acc * 32);
    if (!d_meta || !d_partial || !d_sums) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    const Fr **h_cols = (const Fr **)(meta.data() + off_cols);
    for (size_t c = 0; c < NC; c++) {
        h_cols[c] = in_dev ? (const Fr *)cols[c] : (const Fr *)lane_alloc(ctx, lane, n * 32);
        if (!h_cols[c]) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st));
    if (!in_dev)
        for (size_t c = 0; c < NC; c++) KZG_HIP_CHECK(ctx, hipMemcpyAsync((void *)h_cols[c], cols[c], n * 32, hipMemcpyHostToDevice, st));
    const uint32_t *d_prog = (const uint32_t *)d_meta;
    const Fr *const *d_cols = (const Fr *const *)(d_meta + off_cols);
    const Fr *d_consts = (const Fr *)(d_meta + off_consts);
    if (canon) {
        KZG_LAUNCH(ctx, st, "k_sumcheck_round", k_sumcheck_round<true>, (unsigned)blocks, T, lds, d_prog, d_cols, d_consts, (uint32_t)NI, (uint32_t)h,
                   (uint32_t)n_eval, (uint32_t)plan->n_temps, (uint32_t)n_acc, d_partial);
        KZG_LAUNCH(ctx, st, "k_sumcheck_finish", k_sumcheck_finish<true>, (unsigned)n_acc, 256, 0, (const Fr *)d_partial, (uint32_t)waves, (uint32_t)n_acc, d_sums);
    } else {
        KZG_LAUNCH(ctx, st, "k_sumcheck_round", k_sumcheck_round<false>, (unsigned)blocks, T, lds, d_prog, d_cols, d_consts, (uint32_t)NI, (uint32_t)h,
                   (uint32_t)n_eval, (uint32_t)plan->n_temps, (uint32_t)n_acc, d_partial);
        KZG_LAUNCH(ctx, st, "k_sumcheck_finish", k_sumcheck_finish<false>, (unsigned)n_acc, 256, 0, (const Fr *)d_partial, (uint32_t)waves, (uint32_t)n_acc, d_sums);
    }
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(sums_out, d_sums, n_acc * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}
