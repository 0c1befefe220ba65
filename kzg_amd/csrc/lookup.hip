// lookup.hip -- the column of a logUp-style lookup argument (not reference methods):
//   kzg_lookup_setup / _free / _shape   a table of Fr elements prepared for membership queries
//   kzg_lookup_count                    owners, multiplicities and missing values of `batch` vectors against a plan
//   kzg_logup_terms                     sum_j 1 / (beta + w_j[i]) - m_i / (beta + t_i)
//
// The plan is an open-addressing hash table in HBM with linear probing.  The keys are stored once, reduced to canonical residues; a
// slot is 64 bits, a 32-bit hash tag above the table index, all ones when empty.  BUILD and PROBE are separate launches: kernel
// boundaries are the only synchronisation between workgroups.
//
// Inside the build kernel a slot is touched only through atomic read-modify-write operations at agent scope, and every decision uses
// what they return: compare-and-swap claims an empty slot, and a thread that finds its own key there (same tag, then the full-key
// compare against keys[], which was written before the launch and is read plainly) lowers the slot to its index with atomicMin -- tag
// and key are the same, so the 64-bit minimum is the minimum of the indices: the lowest index owns the residue whichever thread won
// the slot.  WHICH slot of a probe chain a residue ends up in depends on the race; no output does.  No thread waits for another
// thread's write: no spin, no flag, no look-back.  Every probe loop is bounded by the slot count and ends as "not found" or, in the
// build, as KZG_ERR_INTERNAL.
//
// Counting is integer atomics into uint32_t counters, one per table row and vector of a chunk, and one more launch turns the counters
// into field elements.  Range checks make skewed inputs the normal case, so equal owners are combined inside a wave first: up to
// LK_ROUNDS rounds, each of which takes the first lane still uncounted, ballots the lanes with the same owner and issues ONE add of
// their number; what is left after that (a wave whose lanes hit many rows) adds lane by lane.  A thread works on LK_E values, and the
// first group of a step is not added at once: it rides along in the wave while the next step's first group has the same owner, so
// n equal values cost n / (64 LK_E) adds to their row's counter.  The missing values are summed in the workgroup: one add and one
// min per workgroup that has any.
//
// kzg_logup_terms writes beta + x for every denominator of a chunk to workspace (Montgomery form), runs the batch-inversion stage of
// poly.hip over all of them (Montgomery's trick, 16 per inversion) and combines in one more kernel.
#include <string.h>

#include <algorithm>
#include <new>

#include "common.h"

namespace kzg {

constexpr unsigned long long LK_EMPTY = ~0ull;
constexpr uint32_t LK_NONE = 0xFFFFFFFFu;
constexpr int LK_ROUNDS = 4;      // rounds of combining equal owners inside a wave before the lanes add one by one
constexpr int LK_E = 8;           // values per thread of the probe kernel
constexpr size_t LK_STAGE_BYTES = (size_t)64 << 20;
constexpr size_t LK_MAX_NT = (size_t)1 << 26;
constexpr size_t LK_MAX_N = (size_t)1 << 28;
constexpr size_t LK_COUNTERS = (size_t)1 << 24;   // counters of one chunk of vectors, at most (or one vector's)

}  // namespace kzg

struct kzg_lookup {
    int device = 0;
    size_t n_t = 0, distinct = 0, bytes = 0;
    uint32_t smask = 0;   // slots - 1 (a power of two)
    uint32_t hmask = 0;   // the bits of hash and tag that are kept (option "lookup_hash_bits")
    kzg::Fr *keys = nullptr;             // n_t canonical residues
    unsigned long long *slots = nullptr;
    ~kzg_lookup() {
        if (keys) hipFree(keys);
        if (slots) hipFree(slots);
    }
};

namespace kzg {

// home slot (before the slot mask) and tag of a canonical residue
__device__ __forceinline__ void lk_hash(const Fr &k, uint32_t hmask, uint32_t *home, uint32_t *tag) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t w = (uint64_t)k.v[2 * i] | ((uint64_t)k.v[2 * i + 1] << 32);
        h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    }
    h *= 0x94D049BB133111EBull;
    h ^= h >> 32;
    *home = (uint32_t)h & hmask;
    *tag = (uint32_t)(h >> 32) & hmask;
}

// keys[i] = the canonical residue of the caller's word (in place)
__global__ __launch_bounds__(256) void k_lookup_reduce(Fr *keys, size_t n, int canon) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr v = keys[i];
    keys[i] = canon ? fr_residue(v) : from_mont(v);
}

// stat[0]: slots claimed = distinct residues; stat[1]: a key found no slot
__global__ __launch_bounds__(256) void k_lookup_build(const Fr *keys, uint32_t n_t, unsigned long long *slots, uint32_t smask, uint32_t hmask,
                                                      unsigned int *stat) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_t) return;
    const Fr key = keys[i];
    uint32_t s, tag;
    lk_hash(key, hmask, &s, &tag);
    s &= smask;
    const unsigned long long want = ((unsigned long long)tag << 32) | i;
    bool placed = false;
    for (uint32_t p = 0; p <= smask; p++) {     // at most one visit per slot
        const unsigned long long cur = atomicCAS(&slots[s], LK_EMPTY, want);
        if (cur == LK_EMPTY) {
            atomicAdd(&stat[0], 1u);
            placed = true;
            break;
        }
        if ((uint32_t)(cur >> 32) == tag && keys[(uint32_t)cur] == key) {   // (whatever index the slot holds by now has this key)
            atomicMin(&slots[s], want);
            placed = true;
            break;
        }
        s = (s + 1) & smask;
    }
    if (!placed) atomicOr(&stat[1], 1u);
}

struct ProbeArgs {
    const Fr *keys;
    const unsigned long long *slots;
    uint32_t smask, hmask;
    const Fr *vals;        // element j0 of the chunk's first vector; vectors vstride apart
    size_t vstride;
    size_t cnt;            // elements of this piece
    size_t j0;             // index of the piece's first element in its vector
    int canon;
    uint32_t *idx_out;     // optional: the piece's element 0 of the chunk's first vector; vectors ostride apart
    size_t ostride;
    uint32_t *counters;    // optional: n_t per vector of the chunk
    size_t n_t;
    unsigned long long *miss, *first;   // per vector of the chunk
};

// A workgroup takes LK_E runs of 256 consecutive values of one vector (every load and store of a wave is one contiguous run).  No thread
// leaves early: whole waves reach the ballots and the barrier.
__global__ __launch_bounds__(256) void k_lookup_probe(ProbeArgs p) {
    __shared__ uint32_t sh_miss[4], sh_first[4];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    uint32_t *row = p.counters ? p.counters + b * p.n_t : nullptr;
    uint32_t run_idx = LK_NONE, run_cnt = 0;      // wave-uniform: the owner the first counted lane of the last step had, not yet added
    uint32_t my_miss = 0, my_first = LK_NONE;     // (positions are below 2^28)
    for (int e = 0; e < LK_E; e++) {
        const size_t j = ((size_t)blockIdx.x * LK_E + e) * 256 + threadIdx.x;
        const bool live = j < p.cnt;
        uint32_t found = LK_NONE;
        if (live) {
            Fr v = p.vals[b * p.vstride + j];
            v = p.canon ? fr_residue(v) : from_mont(v);
            uint32_t s, tag;
            lk_hash(v, p.hmask, &s, &tag);
            s &= p.smask;
            for (uint32_t q = 0; q <= p.smask; q++) {   // at most one visit per slot: a full table ends as "not found"
                const unsigned long long cur = p.slots[s];
                if (cur == LK_EMPTY) break;
                if ((uint32_t)(cur >> 32) == tag && p.keys[(uint32_t)cur] == v) {
                    found = (uint32_t)cur;
                    break;
                }
                s = (s + 1) & p.smask;
            }
            if (p.idx_out) p.idx_out[b * p.ostride + j] = found;
            if (found == LK_NONE) {
                my_miss++;
                my_first = min(my_first, (uint32_t)(p.j0 + j));
            }
        }
        if (row) {
            const bool hit = live && found != LK_NONE;
            unsigned long long rem = __ballot(hit);
            for (int r = 0; r < LK_ROUNDS && rem; r++) {
                const int leader = __ffsll((long long)rem) - 1;
                const uint32_t lidx = __shfl(found, leader);
                const unsigned long long same = __ballot(hit && found == lidx) & rem;
                const uint32_t c = (uint32_t)__popcll(same);
                if (r == 0) {            // the first group of a step rides along while the owner stays the same
                    if (lidx != run_idx) {
                        if (run_cnt && lane == 0) atomicAdd(&row[run_idx], run_cnt);
                        run_idx = lidx;
                        run_cnt = 0;
                    }
                    run_cnt += c;
                } else if (lane == leader) {
                    atomicAdd(&row[lidx], c);
                }
                rem &= ~same;
            }
            if ((rem >> lane) & 1) atomicAdd(&row[found], 1u);
        }
    }
    if (row && run_cnt && lane == 0) atomicAdd(&row[run_idx], run_cnt);
    // the missing values: one pair of atomics per workgroup
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        my_miss += __shfl_down(my_miss, off);
        my_first = min(my_first, __shfl_down(my_first, off));
    }
    if (lane == 0) {
        sh_miss[threadIdx.x >> 6] = my_miss;
        sh_first[threadIdx.x >> 6] = my_first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m = sh_miss[0] + sh_miss[1] + sh_miss[2] + sh_miss[3];
        if (m) {
            atomicAdd(&p.miss[b], (unsigned long long)m);
            atomicMin(&p.first[b], (unsigned long long)min(min(sh_first[0], sh_first[1]), min(sh_first[2], sh_first[3])));
        }
    }
}

// out[e] = counters[e] as a field element in the caller's form
__global__ __launch_bounds__(256) void k_lookup_emit(const uint32_t *counters, Fr *out, size_t n, int canon) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    Fr c = Fr::zero();
    c.v[0] = counters[e];
    out[e] = canon ? c : mul(c, Fr::r2());
}

// ---------------------------------------------------------------------------------------------
// kzg_logup_terms
// ---------------------------------------------------------------------------------------------
struct LogupArgs {
    const Fr *vals;      // element i0 of column 0 of the chunk's first vector; columns vstride apart, t per vector
    const Fr *table;     // element i0, or null
    const Fr *mult;      // element i0 of the chunk's first vector; vectors mstride apart
    Fr *out;             // likewise, ostride apart
    size_t vstride, mstride, ostride;
    size_t cnt;          // elements of this piece
    size_t t, t1;        // columns; denominators per element (t, or t + 1 with the table)
    int canon;
    Fr beta;             // Montgomery
    Fr *den, *inv;       // the chunk's denominators and their inverses (Montgomery): (b t1 + j) cnt + i
    int *zflag;          // per vector of the chunk
};

__global__ __launch_bounds__(256) void k_logup_den(LogupArgs p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
    if (i >= p.cnt) return;
    for (size_t j = blockIdx.y; j < p.t1; j += gridDim.y) {
        Fr x = j < p.t ? p.vals[(b * p.t + j) * p.vstride + i] : p.table[i];
        if (p.canon) x = mul(x, Fr::r2());      // (any 256-bit word -> the Montgomery form of its residue)
        p.den[(b * p.t1 + j) * p.cnt + i] = add(p.beta, x);
    }
}

__global__ __launch_bounds__(256) void k_logup_combine(LogupArgs p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= p.cnt) return;
    const Fr *iv = p.inv + b * p.t1 * p.cnt + i;
    Fr acc = Fr::zero();
    bool zero = false;
    for (size_t j = 0; j < p.t; j++) {
        const Fr v = iv[j * p.cnt];
        zero = zero || v.is_zero();             // (an inverse is zero for a zero denominator only)
        acc = add(acc, v);
    }
    if (p.canon) acc = from_mont(acc);
    if (p.table) {
        const Fr v = iv[p.t * p.cnt];
        zero = zero || v.is_zero();
        // canonical words: m (v R) / R = m v, any 256-bit m; Montgomery: (m R) (v R) / R = m v R
        acc = sub(acc, mul(p.mult[b * p.mstride + i], v));
    }
    if (zero) atomicOr(&p.zflag[b], 1);
    p.out[b * p.ostride + i] = acc;
}

static bool lk_sfmt_ok(int sfmt) { return sfmt == KZG_FR_MONT_LE_32 || sfmt == KZG_FR_CANONICAL_LE_32; }
static size_t lk_stage(const kzg_ctx *ctx) { return ctx->opt_lookup_stage ? (size_t)ctx->opt_lookup_stage : LK_STAGE_BYTES; }

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_lookup_setup(kzg_ctx *ctx, const void *table, size_t n_t, int sfmt, int flags, kzg_lookup **out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_lookup_setup";
    if (!table || !out) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL table or out");
    if (!lk_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n_t == 0 || n_t > LK_MAX_NT) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": 1 <= n_t <= 2^26 table rows");
    kzg_lookup *pl = new (std::nothrow) kzg_lookup;
    if (!pl) return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    struct Drop {       // the plan is the caller's only once everything has worked
        kzg_lookup *p;
        ~Drop() { delete p; }
    } drop{pl};
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const int spare = ctx->opt_lookup_spare_log ? ctx->opt_lookup_spare_log : 2;
    const size_t S = ((size_t)1 << ilog2_ceil(n_t)) << (spare - 1);       // <= 2^29
    pl->device = ctx->device;
    pl->n_t = n_t;
    pl->smask = (uint32_t)(S - 1);
    pl->hmask = ctx->opt_lookup_hash_bits ? (uint32_t)(((uint64_t)1 << (ctx->opt_lookup_hash_bits - 1)) - 1) : 0xFFFFFFFFu;
    if (hipMalloc((void **)&pl->keys, n_t * 32) != hipSuccess) {
        pl->keys = nullptr;
        return fail(ctx, KZG_ERR_ALLOC, "hipMalloc(lookup keys)");
    }
    if (hipMalloc((void **)&pl->slots, S * 8) != hipSuccess) {
        pl->slots = nullptr;
        return fail(ctx, KZG_ERR_ALLOC, "hipMalloc(lookup slots)");
    }
    pl->bytes = n_t * 32 + S * 8;
    KZG_TRY(lane_reserve(ctx, lane, 65536));
    unsigned int *d_stat = (unsigned int *)lane_alloc(ctx, lane, 256);
    if (!d_stat) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    StreamDrain drain{st};
    const size_t piece = lk_stage(ctx);
    for (size_t o = 0; o < n_t * 32; o += piece) {     // the keys' own memory is the staging buffer
        const size_t len = std::min(piece, n_t * 32 - o);
        KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)pl->keys + o, (const uint8_t *)table + o, len,
                                          (flags & KZG_IN_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    KZG_HIP_CHECK(ctx, hipMemsetAsync(pl->slots, 0xFF, S * 8, st));
    KZG_HIP_CHECK(ctx, hipMemsetAsync(d_stat, 0, 8, st));
    const unsigned blocks = (unsigned)((n_t + 255) / 256);
    KZG_LAUNCH(ctx, st, "k_lookup_reduce", k_lookup_reduce, blocks, 256, 0, pl->keys, n_t, sfmt == KZG_FR_CANONICAL_LE_32 ? 1 : 0);
    KZG_LAUNCH(ctx, st, "k_lookup_build", k_lookup_build, blocks, 256, 0, (const Fr *)pl->keys, (uint32_t)n_t, pl->slots, pl->smask, pl->hmask, d_stat);
    unsigned int stat[2] = {0, 0};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(stat, d_stat, 8, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    if (stat[1]) return fail(ctx, KZG_ERR_INTERNAL, std::string(who) + ": a key found no free slot");
    pl->distinct = stat[0];
    drop.p = nullptr;
    *out = pl;
    return KZG_OK;
}

extern "C" void kzg_lookup_free(kzg_ctx *ctx, kzg_lookup *plan) {
    if (!plan) return;
    if (ctx) hipSetDevice(ctx->device);
    delete plan;
}

extern "C" int kzg_lookup_shape(const kzg_lookup *plan, size_t *n_t, size_t *distinct, size_t *bytes) {
    if (!plan) return KZG_ERR_SHAPE;
    if (n_t) *n_t = plan->n_t;
    if (distinct) *distinct = plan->distinct;
    if (bytes) *bytes = plan->bytes;
    return KZG_OK;
}

extern "C" int kzg_lookup_count(kzg_ctx *ctx, const kzg_lookup *plan, const void *values, size_t n, size_t batch, int sfmt, int flags,
                                void *mult_out, uint32_t *index_out, size_t *missing, size_t *first_missing) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_lookup_count";
    if (!plan) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL plan");
    if (!lk_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (plan->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": the plan is resident on another GPU");
    if (n > LK_MAX_N) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n > 2^28");
    if (batch > (SIZE_MAX >> 6) / std::max<size_t>(n, 1) || batch > (SIZE_MAX >> 6) / plan->n_t)
        return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": batch x n or batch x n_t too large");
    if (batch == 0) return KZG_OK;
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (!mult_out && !index_out && !missing && !first_missing) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": every output is NULL");
    if (!values) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL values");
    const size_t n_t = plan->n_t;
    std::vector<unsigned long long> rep;     // per vector: missing, first missing
    try {  // (no exception may leave through the C ABI)
        rep.resize(2 * batch);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the reports");
    }
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    const size_t stage = lk_stage(ctx);
    // vectors per chunk; elements of one staged piece of a vector (host values larger than a piece go one vector at a time)
    size_t VC = std::min<size_t>({batch, (size_t)65535, std::max<size_t>(1, LK_COUNTERS / n_t)});
    if (ctx->opt_lookup_chunk) VC = std::min<size_t>(VC, (size_t)ctx->opt_lookup_chunk);
    size_t PE = n;
    const bool host_rows = !in_dev || (index_out && !out_dev);    // the probe works on staged rows
    if (host_rows) {
        if (n * 32 > stage) {
            PE = stage / 32;
            VC = 1;
        } else {
            VC = std::min<size_t>(VC, stage / (n * 32));
        }
    }
    const size_t ME = std::min(VC * n_t, stage / 32);            // multiplicities of one staged piece
    const bool st_vals = !in_dev, st_idx = index_out && !out_dev, st_mult = mult_out && !out_dev;
    KZG_TRY(lane_reserve(ctx, lane, (st_vals ? align_up(VC * PE * 32, 256) : 0) + (st_idx ? align_up(VC * PE * 4, 256) : 0) +
                                        (st_mult ? align_up(ME * 32, 256) : 0) + (mult_out ? align_up(VC * n_t * 4, 256) : 0) +
                                        2 * align_up(VC * 8, 256) + 65536));
    Fr *d_vals = st_vals ? (Fr *)lane_alloc(ctx, lane, VC * PE * 32) : nullptr;
    uint32_t *d_idx = st_idx ? (uint32_t *)lane_alloc(ctx, lane, VC * PE * 4) : nullptr;
    Fr *d_mult = st_mult ? (Fr *)lane_alloc(ctx, lane, ME * 32) : nullptr;
    uint32_t *d_cnt = mult_out ? (uint32_t *)lane_alloc(ctx, lane, VC * n_t * 4) : nullptr;
    ProbeArgs a;
    a.miss = (unsigned long long *)lane_alloc(ctx, lane, VC * 8);
    a.first = (unsigned long long *)lane_alloc(ctx, lane, VC * 8);
    if ((st_vals && !d_vals) || (st_idx && !d_idx) || (st_mult && !d_mult) || (mult_out && !d_cnt) || !a.miss || !a.first)
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    a.keys = plan->keys;
    a.slots = plan->slots;
    a.smask = plan->smask;
    a.hmask = plan->hmask;
    a.canon = sfmt == KZG_FR_CANONICAL_LE_32;
    a.counters = d_cnt;
    a.n_t = n_t;
    StreamDrain drain{st};
    for (size_t b0 = 0; b0 < batch; b0 += VC) {
        const size_t G = std::min(VC, batch - b0);
        if (d_cnt) KZG_HIP_CHECK(ctx, hipMemsetAsync(d_cnt, 0, G * n_t * 4, st));
        KZG_HIP_CHECK(ctx, hipMemsetAsync(a.miss, 0, G * 8, st));
        KZG_HIP_CHECK(ctx, hipMemsetAsync(a.first, 0xFF, G * 8, st));
        for (size_t j0 = 0; j0 < n; j0 += PE) {
            const size_t cnt = std::min(PE, n - j0);      // (PE < n: G == 1)
            if (st_vals) {
                KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_vals, (const uint8_t *)values + (b0 * n + j0) * 32, (G - 1) * n * 32 + cnt * 32, hipMemcpyHostToDevice, st));
                a.vals = d_vals;
            } else {
                a.vals = (const Fr *)values + b0 * n + j0;
            }
            a.vstride = n;       // (staged rows keep the caller's layout: whole vectors, or a run of one vector)
            a.cnt = cnt;
            a.j0 = j0;
            a.idx_out = !index_out ? nullptr : st_idx ? d_idx : index_out + b0 * n + j0;
            a.ostride = n;
            KZG_LAUNCH(ctx, st, "k_lookup_probe", k_lookup_probe, dim3((unsigned)((cnt + 256 * LK_E - 1) / (256 * LK_E)), (unsigned)G), 256, 0, a);
            if (st_idx) KZG_HIP_CHECK(ctx, hipMemcpyAsync(index_out + b0 * n + j0, d_idx, ((G - 1) * n + cnt) * 4, hipMemcpyDeviceToHost, st));
        }
        if (mult_out) {
            const int canon = a.canon;
            if (out_dev) {
                KZG_LAUNCH(ctx, st, "k_lookup_emit", k_lookup_emit, (unsigned)((G * n_t + 255) / 256), 256, 0, (const uint32_t *)d_cnt, (Fr *)mult_out + b0 * n_t,
                           G * n_t, canon);
            } else {
                for (size_t e0 = 0; e0 < G * n_t; e0 += ME) {
                    const size_t ce = std::min(ME, G * n_t - e0);
                    KZG_LAUNCH(ctx, st, "k_lookup_emit", k_lookup_emit, (unsigned)((ce + 255) / 256), 256, 0, (const uint32_t *)d_cnt + e0, d_mult, ce, canon);
                    KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)mult_out + (b0 * n_t + e0) * 32, d_mult, ce * 32, hipMemcpyDeviceToHost, st));
                }
            }
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(rep.data() + b0, a.miss, G * 8, hipMemcpyDeviceToHost, st));
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(rep.data() + batch + b0, a.first, G * 8, hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    bool any = false;
    for (size_t b = 0; b < batch; b++) {
        if (missing) missing[b] = (size_t)rep[b];
        if (first_missing) first_missing[b] = rep[b] ? (size_t)rep[batch + b] : SIZE_MAX;
        any = any || rep[b];
    }
    if (any && !missing && !first_missing) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a value is not in the table");
    return KZG_OK;
}

extern "C" int kzg_logup_terms(kzg_ctx *ctx, const void *values, const void *table, const void *mult, const void *beta, size_t n, size_t t,
                               size_t batch, int sfmt, int flags, void *out, int *zero_den) {
    if (!ctx) return KZG_ERR_SHAPE;
    const char *who = "kzg_logup_terms";
    if (!lk_sfmt_ok(sfmt)) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": empty vectors");
    if (n > LK_MAX_N) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": n > 2^28");
    if ((table == nullptr) != (mult == nullptr)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": table and mult go together");
    if (!table && t == 0) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": no columns and no table");
    const size_t t1 = t + (table ? 1 : 0);
    if (t1 > (SIZE_MAX >> 7) / n || batch > (SIZE_MAX >> 7) / (t1 * n)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": batch x t x n too large");
    if (batch == 0) return KZG_OK;
    if ((t && !values) || !beta || !out) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": NULL values, beta or out");
    Fr bw;
    memcpy(bw.v, beta, 32);
    if (!is_canonical(bw)) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": beta is not below r");
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
    // a chunk: at most DEN denominators -- whole vectors, or a run of PE elements of one vector with its t1 columns
    const size_t DEN = std::max<size_t>(1, lk_stage(ctx) / 32);
    const size_t PE = std::min(n, std::max<size_t>(1, DEN / t1));
    size_t VC = PE < n ? 1 : std::min<size_t>({batch, (size_t)65535, std::max<size_t>(1, DEN / (t1 * n))});
    if (ctx->opt_lookup_chunk) VC = std::min<size_t>(VC, (size_t)ctx->opt_lookup_chunk);
    const size_t dens = VC * t1 * PE;
    KZG_TRY(lane_reserve(ctx, lane, 2 * align_up(dens * 32, 256) + (in_dev ? 0 : align_up(VC * t * PE * 32, 256) + (table ? align_up(PE * 32, 256) + align_up(VC * PE * 32, 256) : 0)) +
                                        (out_dev ? 0 : align_up(VC * PE * 32, 256)) + align_up(VC * sizeof(int), 256) + 65536));
    LogupArgs a;
    a.den = (Fr *)lane_alloc(ctx, lane, dens * 32);
    a.inv = (Fr *)lane_alloc(ctx, lane, dens * 32);
    a.zflag = (int *)lane_alloc(ctx, lane, VC * sizeof(int));
    Fr *d_vals = !in_dev && t ? (Fr *)lane_alloc(ctx, lane, VC * t * PE * 32) : nullptr;
    Fr *d_tab = !in_dev && table ? (Fr *)lane_alloc(ctx, lane, PE * 32) : nullptr;
    Fr *d_mult = !in_dev && table ? (Fr *)lane_alloc(ctx, lane, VC * PE * 32) : nullptr;
    Fr *d_out = out_dev ? nullptr : (Fr *)lane_alloc(ctx, lane, VC * PE * 32);
    if (!a.den || !a.inv || !a.zflag || (!in_dev && t && !d_vals) || (!in_dev && table && (!d_tab || !d_mult)) || (!out_dev && !d_out))
        return fail(ctx, KZG_ERR_ALLOC, "workspace");
    a.t = t;
    a.t1 = t1;
    a.canon = sfmt == KZG_FR_CANONICAL_LE_32;
    a.beta = a.canon ? to_mont(bw) : bw;
    StreamDrain drain{st};
    for (size_t b0 = 0; b0 < batch; b0 += VC) {
        const size_t G = std::min(VC, batch - b0);
        KZG_HIP_CHECK(ctx, hipMemsetAsync(a.zflag, 0, G * sizeof(int), st));
        for (size_t i0 = 0; i0 < n; i0 += PE) {
            const size_t cnt = std::min(PE, n - i0);      // (PE < n: G == 1)
            a.cnt = cnt;
            if (in_dev) {
                a.vals = (const Fr *)values + b0 * t * n + i0;
                a.table = table ? (const Fr *)table + i0 : nullptr;
                a.mult = mult ? (const Fr *)mult + b0 * n + i0 : nullptr;
                a.vstride = a.mstride = n;
            } else {
                if (cnt == n) {      // whole vectors: the columns of the chunk are one run
                    if (t) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_vals, (const uint8_t *)values + b0 * t * n * 32, G * t * n * 32, hipMemcpyHostToDevice, st));
                    if (mult) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_mult, (const uint8_t *)mult + b0 * n * 32, G * n * 32, hipMemcpyHostToDevice, st));
                } else {             // a run of one vector: column by column
                    for (size_t j = 0; j < t; j++)
                        KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_vals + j * cnt, (const uint8_t *)values + ((b0 * t + j) * n + i0) * 32, cnt * 32, hipMemcpyHostToDevice, st));
                    if (mult) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_mult, (const uint8_t *)mult + (b0 * n + i0) * 32, cnt * 32, hipMemcpyHostToDevice, st));
                }
                if (table) KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_tab, (const uint8_t *)table + i0 * 32, cnt * 32, hipMemcpyHostToDevice, st));
                a.vals = d_vals;
                a.table = d_tab;
                a.mult = d_mult;
                a.vstride = a.mstride = cnt;
            }
            a.out = out_dev ? (Fr *)out + b0 * n + i0 : d_out;
            a.ostride = out_dev ? n : cnt;
            const unsigned gx = (unsigned)((cnt + 255) / 256);
            KZG_LAUNCH(ctx, st, "k_logup_den", k_logup_den, dim3(gx, (unsigned)std::min<size_t>(t1, 65535), (unsigned)G), 256, 0, a);
            KZG_TRY(batch_inverse(ctx, st, a.den, a.inv, G * t1 * cnt));
            KZG_LAUNCH(ctx, st, "k_logup_combine", k_logup_combine, dim3(gx, (unsigned)G), 256, 0, a);
            if (!out_dev) {
                if (cnt == n) KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out + b0 * n * 32, d_out, G * n * 32, hipMemcpyDeviceToHost, st));
                else KZG_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)out + (b0 * n + i0) * 32, d_out, cnt * 32, hipMemcpyDeviceToHost, st));
            }
        }
        KZG_HIP_CHECK(ctx, hipMemcpyAsync(zf.data() + b0, a.zflag, G * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    bool any = false;
    for (size_t b = 0; b < batch; b++) {     // a vector with a zero denominator: its row is all zero
        if (zf[b]) {
            any = true;
            if (out_dev) KZG_HIP_CHECK(ctx, hipMemsetAsync((uint8_t *)out + b * n * 32, 0, n * 32, st));
            else memset((uint8_t *)out + b * n * 32, 0, n * 32);
        }
        if (zero_den) zero_den[b] = zf[b];
    }
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    if (any && !zero_den) return fail(ctx, KZG_ERR_SHAPE, std::string(who) + ": a zero denominator");
    return KZG_OK;
}
