// fr_program.hip -- constraint expressions over columns of Fr in one pass (not a reference method):
//   kzg_fr_program_setup / _free / _shape   a straight-line program over Fr, validated once and kept
//   kzg_fr_program_run                      the program for every row i < n of a set of columns
//
// The kernel is an interpreter.  One lane owns one row and walks the whole instruction stream; every lane of the grid walks the same
// stream, so the six words of an instruction, the column descriptors, the output pointers and the consts are read at wave-uniform
// addresses (the scalar cache, as k_fr_fold reads gamma) and the dispatch on op and kinds is a wave-uniform branch: no lane diverges.
// Lanes beyond n stay in the loop on the last row and skip only the stores.
//
// Temporaries live in LDS -- a register array indexed by a run-time value would go to scratch memory --, 32 bytes per temporary and
// thread, dynamic, sized by the plan's temporary count.  The four 8-byte limb pairs of a value lie T = blockDim.x slots apart and the
// threads' copies of one pair side by side: a wave's access to one pair of one temporary is 64 consecutive 8-byte words, conflict-free.
// A lane touches its own slots only: no barrier anywhere.
//
// The arithmetic is Montgomery whatever the data's format.  Consts are brought to Montgomery form once per run on the host.  Canonical
// data pays one product per column load (with R^2, which takes any 256-bit word to a residue in Montgomery form) and one per store.
//
// What depends on the run and not on the plan -- the shifts reduced into [0, col_len), the column descriptors, the consts -- is
// written on the host per call and uploaded with the program to the lane's workspace: 24 bytes per instruction.  A full-length
// column then needs one conditional subtract per load, a periodic one a mask; no row performs a division.
#include <algorithm>
#include <new>

#include "common.h"
#include "fr_program.h"

namespace kzg {

constexpr size_t FRP_MAX_N = (size_t)1 << 28;
constexpr size_t FRP_MAX_INSNS = 65536, FRP_MAX_COLS = 4096, FRP_MAX_CONSTS = 4096, FRP_MAX_OUT = 64;
constexpr int FRP_LDS_MAX = KZG_FRP_MAX_TEMPS * 32 * 256;   // sixteen temporaries at 256 threads: 128 KiB of the CU's 160

template <bool CANON>
__device__ __forceinline__ Fr frp_fetch(const FrpCol *__restrict__ cols, const Fr *__restrict__ consts, uint32_t kind, uint32_t idx, uint32_t shift,
                                        uint32_t row, const uint2 *lds) {
    if (kind == KZG_FRP_COL) {
        const FrpCol c = cols[idx];                  // uniform
        uint32_t j = row + shift;                    // row < n <= 2^28, shift < len <= n
        if (c.mask == 0xFFFFFFFFu) j -= j >= c.len ? c.len : 0;
        else j &= c.mask;
        const Fr v = frp_load(c.p + j);
        return CANON ? mul(v, Fr::r2()) : v;
    }
    if (kind == KZG_FRP_CONST) return consts[idx];   // uniform: out of SGPRs
    return frp_get(lds, blockDim.x, idx);
}

// grid ceil(n / blockDim.x); dynamic LDS: 32 bytes x temporaries x blockDim.x.  prog: n_insns x KZG_FRP_WORDS words with the shifts
// already in [0, len); consts: Montgomery.  The four tables are read-only and read at uniform addresses: scalar loads.
template <bool CANON>
__global__ __launch_bounds__(256) void k_fr_program(const uint32_t *__restrict__ prog, const FrpCol *__restrict__ cols, const Fr *__restrict__ consts,
                                                    Fr *const *__restrict__ outs, uint32_t n_insns, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint2 frp_lds[];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const uint32_t row = live ? i : n - 1;
    for (uint32_t pc = 0; pc < n_insns; pc++) {
        const uint32_t *__restrict__ w = prog + pc * KZG_FRP_WORDS;
        const uint32_t head = w[0], dst = w[1];
        const Fr a = frp_fetch<CANON>(cols, consts, (head >> 16) & 0xFF, w[2], w[4], row, frp_lds);
        const Fr b = frp_fetch<CANON>(cols, consts, head >> 24, w[3], w[5], row, frp_lds);
        const uint32_t op = head & 0xFF;
        Fr d;
        if (op == KZG_FRP_MUL) d = mul(a, b);
        else if (op == KZG_FRP_ADD) d = add(a, b);
        else d = sub(a, b);
        if (((head >> 8) & 0xFF) == KZG_FRP_TEMP) {
            frp_put(frp_lds, blockDim.x, dst, d);
        } else {
            if (CANON) d = from_mont(d);
            Fr *o = outs[dst];
            if (live) frp_store(o + i, d);
        }
    }
}

static int frp_attrs(kzg_ctx *ctx) {
    if (ctx->attr_frprog_set) return KZG_OK;
    KZG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_fr_program<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FRP_LDS_MAX));
    KZG_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_fr_program<true>, hipFuncAttributeMaxDynamicSharedMemorySize, FRP_LDS_MAX));
    ctx->attr_frprog_set = true;
    return KZG_OK;
}

// threads of a workgroup: the LDS of a CU (160 KiB) holds 5,120 temporaries of 32 bytes, so up to 4 temporaries leave 1,024 threads
// and more per CU at any block size; above that the smaller block wastes less of the LDS to rounding (16 temporaries: 5 waves a CU at
// 64 threads, 4 at 128 or 256)
static int frp_block(const kzg_ctx *ctx, size_t n_temps) {
    if (ctx->opt_fr_program_block) return ctx->opt_fr_program_block;
    return n_temps <= 4 ? 256 : n_temps <= 8 ? 128 : 64;
}

}  // namespace kzg

using namespace kzg;

extern "C" int kzg_fr_program_setup(kzg_ctx *ctx, const uint32_t *words, size_t n_insns, size_t n_cols, size_t n_consts, size_t n_out,
                                    kzg_fr_program **out) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_fr_program_setup";
    if (!words || !out) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL words or out");
    if (n_insns == 0 || n_insns > FRP_MAX_INSNS) return fail(ctx, KZG_ERR_SHAPE, who + ": 1 <= n_insns <= 65,536");
    if (n_cols > FRP_MAX_COLS || n_consts > FRP_MAX_CONSTS) return fail(ctx, KZG_ERR_SHAPE, who + ": n_cols, n_consts <= 4,096");
    if (n_out == 0 || n_out > FRP_MAX_OUT) return fail(ctx, KZG_ERR_SHAPE, who + ": 1 <= n_out <= 64");
    uint32_t temp_written = 0;
    uint64_t out_written = 0;
    size_t n_temps = 0, n_mul = 0;
    for (size_t k = 0; k < n_insns; k++) {
        const uint32_t *w = words + k * KZG_FRP_WORDS;
        const std::string at = who + ": instruction " + std::to_string(k) + ": ";
        const uint32_t op = w[0] & 0xFF, dk = (w[0] >> 8) & 0xFF, kinds[2] = {(w[0] >> 16) & 0xFF, w[0] >> 24};
        if (op != KZG_FRP_ADD && op != KZG_FRP_SUB && op != KZG_FRP_MUL) return fail(ctx, KZG_ERR_SHAPE, at + "unknown op");
        for (int s = 0; s < 2; s++) {
            const uint32_t idx = w[2 + s];
            if (kinds[s] == KZG_FRP_COL) {
                if (idx >= n_cols) return fail(ctx, KZG_ERR_SHAPE, at + "column index out of range");
            } else if (kinds[s] == KZG_FRP_CONST) {
                if (idx >= n_consts) return fail(ctx, KZG_ERR_SHAPE, at + "const index out of range");
            } else if (kinds[s] == KZG_FRP_TEMP) {
                if (idx >= KZG_FRP_MAX_TEMPS) return fail(ctx, KZG_ERR_SHAPE, at + "temporary index >= 16");
                if (!((temp_written >> idx) & 1)) return fail(ctx, KZG_ERR_SHAPE, at + "a temporary is read before it is written");
            } else {
                return fail(ctx, KZG_ERR_SHAPE, at + (kinds[s] == KZG_FRP_OUT ? "an output is write-only" : "unknown operand kind"));
            }
            if (kinds[s] != KZG_FRP_COL && w[4 + s] != 0) return fail(ctx, KZG_ERR_SHAPE, at + "a shift on an operand that is no column");
        }
        if (dk == KZG_FRP_TEMP) {
            if (w[1] >= KZG_FRP_MAX_TEMPS) return fail(ctx, KZG_ERR_SHAPE, at + "temporary index >= 16");
            temp_written |= 1u << w[1];
            n_temps = std::max<size_t>(n_temps, w[1] + 1);
        } else if (dk == KZG_FRP_OUT) {
            if (w[1] >= n_out) return fail(ctx, KZG_ERR_SHAPE, at + "output index out of range");
            if ((out_written >> w[1]) & 1) return fail(ctx, KZG_ERR_SHAPE, at + "an output is written twice");
            out_written |= (uint64_t)1 << w[1];
        } else {
            return fail(ctx, KZG_ERR_SHAPE, at + (dk == KZG_FRP_COL || dk == KZG_FRP_CONST ? "columns and consts are read-only" : "unknown destination kind"));
        }
        if (op == KZG_FRP_MUL) n_mul++;
    }
    if (out_written != (n_out == 64 ? ~(uint64_t)0 : ((uint64_t)1 << n_out) - 1)) return fail(ctx, KZG_ERR_SHAPE, who + ": an output is never written");
    kzg_fr_program *pl = new (std::nothrow) kzg_fr_program;
    if (!pl) return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    try {  // (no exception may leave through the C ABI)
        pl->words.assign(words, words + n_insns * KZG_FRP_WORDS);
    } catch (const std::bad_alloc &) {
        delete pl;
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the plan");
    }
    pl->device = ctx->device;
    pl->n_cols = n_cols;
    pl->n_consts = n_consts;
    pl->n_out = n_out;
    pl->n_temps = n_temps;
    pl->n_mul = n_mul;
    *out = pl;
    return KZG_OK;
}

extern "C" void kzg_fr_program_free(kzg_ctx *, kzg_fr_program *plan) { delete plan; }

extern "C" int kzg_fr_program_shape(const kzg_fr_program *plan, size_t *n_insns, size_t *n_cols, size_t *n_consts, size_t *n_out,
                                    size_t *n_temps, size_t *n_mul) {
    if (!plan) return KZG_ERR_SHAPE;
    if (n_insns) *n_insns = plan->words.size() / KZG_FRP_WORDS;
    if (n_cols) *n_cols = plan->n_cols;
    if (n_consts) *n_consts = plan->n_consts;
    if (n_out) *n_out = plan->n_out;
    if (n_temps) *n_temps = plan->n_temps;
    if (n_mul) *n_mul = plan->n_mul;
    return KZG_OK;
}

extern "C" int kzg_fr_program_run(kzg_ctx *ctx, const kzg_fr_program *plan, const void *const *cols, const size_t *col_len, const void *consts,
                                  size_t n, int sfmt, int flags, void *const *outs) {
    if (!ctx) return KZG_ERR_SHAPE;
    const std::string who = "kzg_fr_program_run";
    if (!plan) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL plan");
    if (plan->device != ctx->device) return fail(ctx, KZG_ERR_SHAPE, who + ": the plan belongs to another GPU");
    if (sfmt != KZG_FR_MONT_LE_32 && sfmt != KZG_FR_CANONICAL_LE_32) return fail(ctx, KZG_ERR_SHAPE, "unknown scalar format");
    if (n == 0) return fail(ctx, KZG_ERR_SHAPE, who + ": n == 0");
    if (n > FRP_MAX_N) return fail(ctx, KZG_ERR_SHAPE, who + ": n > 2^28");
    const size_t NC = plan->n_cols, NK = plan->n_consts, NO = plan->n_out, NI = plan->words.size() / KZG_FRP_WORDS;
    if ((NC && (!cols || !col_len)) || (NK && !consts) || !outs) return fail(ctx, KZG_ERR_SHAPE, who + ": NULL cols, col_len, consts or outs");
    for (size_t c = 0; c < NC; c++) {
        const size_t len = col_len[c];
        if (len == 0 || (len != n && ((len & (len - 1)) || n % len)))
            return fail(ctx, KZG_ERR_SHAPE, who + ": the length of column " + std::to_string(c) + " is neither n nor a power of two that divides n");
        if (!cols[c]) return fail(ctx, KZG_ERR_SHAPE, who + ": a NULL column");
    }
    for (size_t o = 0; o < NO; o++) {
        if (!outs[o]) return fail(ctx, KZG_ERR_SHAPE, who + ": a NULL output");
        for (size_t c = 0; c < NC; c++)
            if (outs[o] == cols[c]) return fail(ctx, KZG_ERR_SHAPE, who + ": an output is a column (rotations make in-place evaluation a race)");
        for (size_t q = 0; q < o; q++)
            if (outs[o] == outs[q]) return fail(ctx, KZG_ERR_SHAPE, who + ": two outputs are one buffer");
    }
    const bool canon = sfmt == KZG_FR_CANONICAL_LE_32;
    const bool in_dev = (flags & KZG_IN_DEVICE) != 0, out_dev = (flags & KZG_OUT_DEVICE) != 0;
    // what the kernel reads besides the columns, in one host buffer and one upload: program | column descriptors | output pointers | consts
    const size_t off_cols = align_up(NI * KZG_FRP_WORDS * 4, 256), off_outs = off_cols + align_up(NC * sizeof(FrpCol), 256),
                 off_consts = off_outs + align_up(NO * sizeof(Fr *), 256), meta_bytes = off_consts + align_up(NK * 32, 256);
    std::vector<uint8_t> meta;
    try {  // (no exception may leave through the C ABI)
        meta.resize(meta_bytes);
    } catch (const std::bad_alloc &) {
        return fail(ctx, KZG_ERR_ALLOC, "host memory for the program");
    }
    Fr *h_consts = (Fr *)(meta.data() + off_consts);
    for (size_t k = 0; k < NK; k++) {
        Fr x;
        memcpy(x.v, (const uint8_t *)consts + k * 32, 32);
        if (!is_canonical(x)) return fail(ctx, KZG_ERR_SHAPE, who + ": const " + std::to_string(k) + " is not below r");
        h_consts[k] = canon ? to_mont(x) : x;
    }
    uint32_t *h_prog = (uint32_t *)meta.data();
    memcpy(h_prog, plan->words.data(), NI * KZG_FRP_WORDS * 4);
    for (size_t k = 0; k < NI; k++) {     // the shifts into [0, len): all that the kernel adds to a row index
        uint32_t *w = h_prog + k * KZG_FRP_WORDS;
        const uint32_t kinds[2] = {(w[0] >> 16) & 0xFF, w[0] >> 24};
        for (int s = 0; s < 2; s++) {
            if (kinds[s] != KZG_FRP_COL) continue;
            const int64_t len = (int64_t)col_len[w[2 + s]];
            const int64_t m = (int64_t)(int32_t)w[4 + s] % len;
            w[4 + s] = (uint32_t)(m < 0 ? m + len : m);
        }
    }
    Lease ls;
    KZG_TRY(lease_lane(ctx, &ls));
    const int lane = ls.lane;
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->lanes[lane].stream;
    KZG_TRY(frp_attrs(ctx));
    size_t need = meta_bytes + 65536;
    if (!in_dev)
        for (size_t c = 0; c < NC; c++) need += align_up(col_len[c] * 32, 256);
    if (!out_dev) need += NO * align_up(n * 32, 256);
    KZG_TRY(lane_reserve(ctx, lane, need));
    uint8_t *d_meta = (uint8_t *)lane_alloc(ctx, lane, meta_bytes);
    if (!d_meta) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    FrpCol *h_cols = (FrpCol *)(meta.data() + off_cols);
    Fr **h_outs = (Fr **)(meta.data() + off_outs);
    for (size_t c = 0; c < NC; c++) {
        h_cols[c].p = in_dev ? (const Fr *)cols[c] : (const Fr *)lane_alloc(ctx, lane, col_len[c] * 32);
        if (!h_cols[c].p) return fail(ctx, KZG_ERR_ALLOC, "workspace");
        h_cols[c].len = (uint32_t)col_len[c];
        h_cols[c].mask = col_len[c] == n ? 0xFFFFFFFFu : (uint32_t)col_len[c] - 1;
    }
    for (size_t o = 0; o < NO; o++) {
        h_outs[o] = out_dev ? (Fr *)outs[o] : (Fr *)lane_alloc(ctx, lane, n * 32);
        if (!h_outs[o]) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    }
    StreamDrain drain{st};
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(d_meta, meta.data(), meta_bytes, hipMemcpyHostToDevice, st));
    if (!in_dev)
        for (size_t c = 0; c < NC; c++) KZG_HIP_CHECK(ctx, hipMemcpyAsync((void *)h_cols[c].p, cols[c], col_len[c] * 32, hipMemcpyHostToDevice, st));
    const uint32_t *d_prog = (const uint32_t *)d_meta;
    const FrpCol *d_cols = (const FrpCol *)(d_meta + off_cols);
    Fr *const *d_outs = (Fr *const *)(d_meta + off_outs);
    const Fr *d_consts = (const Fr *)(d_meta + off_consts);
    const int T = frp_block(ctx, plan->n_temps);
    const unsigned blocks = (unsigned)((n + T - 1) / T);    // n <= 2^28 and T >= 64: at most 2^22 workgroups, one grid
    const size_t lds = plan->n_temps * 32 * (size_t)T;
    if (canon) KZG_LAUNCH(ctx, st, "k_fr_program", k_fr_program<true>, blocks, T, lds, d_prog, d_cols, d_consts, d_outs, (uint32_t)NI, (uint32_t)n);
    else KZG_LAUNCH(ctx, st, "k_fr_program", k_fr_program<false>, blocks, T, lds, d_prog, d_cols, d_consts, d_outs, (uint32_t)NI, (uint32_t)n);
    if (!out_dev)
        for (size_t o = 0; o < NO; o++) KZG_HIP_CHECK(ctx, hipMemcpyAsync(outs[o], h_outs[o], n * 32, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    if (ctx->prof) prof_collect(ctx);
    return KZG_OK;
}
