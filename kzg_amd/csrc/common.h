// common.h -- context, workspace arena, error handling and profiled kernel launches shared by the
// translation units of libkzg_mi355x.so.
#pragma once
#ifndef KZG_NTT_KERNEL_DEFAULT
#define KZG_NTT_KERNEL_DEFAULT 1
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <array>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "curve.h"
#include "curve30.h"

namespace kzg {

struct ProfEntry {
    uint64_t launches = 0;
    double total_ms = 0.0;
};

struct PendingEvent {
    std::string name;
    hipEvent_t start, stop;
};

#ifndef KZG_ACCUM_WAVES
#define KZG_ACCUM_WAVES 2  // waves per SIMD k_accum_affine is compiled for (VGPR budget 512 / waves)
#endif

// How one MSM is shaped for what else is on the GPU (set per lane by the entry point that submits it).
struct MsmMode {
    int accum_blocks = 256 * KZG_ACCUM_WAVES;  // k_accum_affine grid (a lone MSM: every SIMD holds its KZG_ACCUM_WAVES waves)
    int sort_threads = 1024;                   // threads per k_hist / k_scatter block
    bool tail_quads = true;   // four lanes per point operation in the depth-bound tail kernels (latency mode, msm_tail.hip)
    bool tail_wide = false;   // a pipeline whose lanes never run dry: work-efficient fold width and row/column sums
};

// One independent execution lane: a HIP stream plus a bump-allocated scratch arena in HBM.
// Exclusive calls use lane 0; kzg_msm_g1_batch pipelines independent MSMs over several lanes (two in flight per lane); concurrent
// blocking callers (commit / create_witness / create_witness_batched / fft ... from many host threads) each lease one lane for the
// duration of their call.
struct Lane {
    MsmMode mode;
    hipStream_t stream = nullptr;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    size_t arena_used = 0;
    size_t arena_limit = 0;  // 0 = the whole arena; else lane_alloc fails beyond this offset (two MSMs in flight share the arena as halves)
    uint32_t heavy_seq = 0, heavy_seen = 0;  // MSMs sorted on this lane / the one last looked at (kzg_ctx::d_lane_heavy)
    char *pinned = nullptr;  // small pinned host staging buffer for results
    size_t pinned_bytes = 0;
};

struct NttPlan;
struct FixedBaseTable;
struct EvalDomainTables;

// Who may use the context when.  Two kinds of callers:
//   exclusive  everything that works on all lanes at once or rebuilds shared state (the *_batch / *_many entry points, SRS
//              construction, the pairing verifier, options, profiling, kzg_sync / kzg_dev_free): one at a time.  lock() / unlock() --
//              the type is a BasicLockable, so std::lock_guard<CtxGate> is the old "Guard".
//   shared     every blocking call of the reference that works on ONE lane (KZGProver::commit / create_witness /
//              create_witness_batched, both forms, verify_poly, EvaluationDomain::fft and friends: `&self` methods of Clone types,
//              src/coeff_form.rs:59-124, src/eval_form.rs:114-171, src/ft.rs:111-271).  Each leases a free lane under this short lock
//              (kzg::Lease), submits its kernels there (accumulation kernels on the shared FIFO streams) and waits for its own
//              stream only -- N host threads keep the pipeline as full as kzg_msm_g1_batch does.  The caches such calls share (NTT
//              plans, coset tables, evaluation-domain tables) are guarded by kzg_ctx::cache_mu.
// Exclusive callers wait for the leased lanes to drain and hold new leases off while they wait (no starvation).
struct CtxGate {
    std::mutex m;
    std::condition_variable cv;
    int shared_active = 0;
    int excl_waiting = 0;
    bool exclusive = false;
    uint32_t lane_busy = 0;  // bit l: lane l is leased
    void lock() {
        std::unique_lock<std::mutex> lk(m);
        excl_waiting++;
        cv.wait(lk, [&] { return !exclusive && shared_active == 0; });
        excl_waiting--;
        exclusive = true;
    }
    void unlock() {
        {
            std::lock_guard<std::mutex> lk(m);
            exclusive = false;
        }
        cv.notify_all();
    }
};
constexpr int KZG_HEAVY_WINDOW = 64;  // MSMs for which one oversized sort bin keeps the slice kernels enqueued (kzg_ctx::heavy_last)
constexpr int KZG_MAX_LANES = 24;  // lanes.reserve(): leased lanes are indexed while other threads append
constexpr int KZG_MAX_GROUP = 16;  // MSMs per sort / tail launch of the grouped pipeline, at most (option group_msms)
constexpr int KZG_GROUP_DEPTH = 2;  // groups in flight = halves of the group arena (three measured no faster at 16 MSMs per group)
struct GroupSlot;

}  // namespace kzg

struct kzg_ctx;
namespace kzg {
struct StreamPool;                     // runtime.hip: the process' streams of one device, shared by its contexts
struct PointSetCache;
void point_sets_free(kzg_ctx *ctx);  // witness.hip
void point_set_stats(kzg_ctx *ctx, uint64_t *hits, uint64_t *misses);
}
struct kzg_ctx {
    int device = 0;
    kzg::CtxGate mu;
    std::mutex err_mu;   // err
    std::mutex prof_mu;  // prof_map, prof_pending, event_pool
    std::mutex cache_mu; // ntt_plans, coset_tabs, eval_tabs: built by one leased caller at a time, published after the builder's stream is synchronised
    std::mutex accum_mu; // wait / launch / record on a shared accumulation stream is one unit
    std::atomic<uint32_t> accum_rr{0};  // round robin over the accumulation streams (leased lanes)
    // the last plan of the batched pipeline (plan_pipeline): what was asked for, what the hardware-queue pool of the process allowed.
    // narrowed (plan_lanes < plan_want_lanes or plan_accum < plan_want_accum) = other streams of the process -- a second context, an
    // RCCL communicator, the host's own -- hold queues: reported by kzg_ctx_info / kzg_mctx_info and once on stderr.
    int plan_want_lanes = 0, plan_want_accum = 0, plan_lanes = 0, plan_accum = 0, plan_queues = 0;
    bool plan_warned = false;
    bool pipe_planned = false;          // lanes + accumulation streams created, probed and ordered for concurrent callers
    int pipe_lanes = 1, pipe_accum = 0;
    std::string err;
    std::vector<kzg::Lane> lanes;
    kzg::StreamPool *pool = nullptr;   // where the lanes' and accumulation streams come from (runtime.hip)
    int opt_window_bits = 0;  // 0 = auto
    int opt_streams = 13;  // lanes: depth of the batched pipeline and of the pool concurrent blocking callers lease from (13 + 4
                           // accumulation streams leave an RCCL communicator its ~6 hardware queues of the 24: runtime.hip, StreamPool)
    int opt_accum_blocks = 0;          // k_accum_affine grid for a single MSM (0 = every SIMD holds its KZG_ACCUM_WAVES waves)
    int opt_hw_queues = 0;             // hardware queues to plan the batched pipeline for (0 = measure: probe_queues in runtime.hip)
    int probed_queues = 0;             // hardware queues the probed streams were found on (0 = not measured yet)
    int probed_lanes = 0, probed_accum = 0;  // which streams that measurement covered: lanes [0, probed_lanes), accumulation streams
    std::vector<hipStream_t> probed_order;  // the probed streams, one per queue first
    int opt_window_rows = 0;           // 0 = every window has its table row; r > 0: keep r rows (low-memory SRS, multi-pass MSM)
    int opt_naf_window = 0;            // SRSs created afterwards: 18 = positional tables + width-18 NAF digits (17x the table; measured
                                       // +3.7 % batched throughput at 2^20, nothing below 2^19, +1.3 ms on a lone commit: off by default)
    int opt_trusted_points = 0;        // 1: caller vouches for its points (skip the subgroup check of uploads / verifier inputs)
    int opt_ntt_vec_log = 2;           // NTT passes: 2^v adjacent columns / rows per LDS tile
    int opt_verify_cosets_chunk = 0;   // kzg_verify_cosets: at most this many cells per chunk (0 = the rule min(16384, 2^20 / l) alone)
    int opt_verify_eval_batch_chunk = 0;  // kzg_verify_eval_batch: at most this many openings per chunk (0 = 16384 alone)
    int opt_multiopen_points_chunk = 0;   // kzg_multiopen_eval_commit: at most this many distinct points per chunk (0 = min(16, 2^22 / d) alone)
    int opt_multi_eval_segment = 0;       // kzg_poly_multi_eval: forced segment length, a power of two >= 8 (0 = planned from n, k, batch)
    int opt_multi_eval_points_chunk = 0;  // kzg_poly_multi_eval: at most this many points per pass (0 = 4096 alone); either option takes the kernels at any k
    int opt_poly_divide_base = 0;         // kzg_poly_divide: precision the base kernel of the series inverse produces, a power of two <= 64 (0 = 64)
    int opt_fr_scan_tile = 0;             // kzg_fr_scan / kzg_fr_grand_product: elements one workgroup scans, a power of two in 8..2048 (0 = 2048)
    int opt_fr_scan_stage = 0;            // ... and kzg_fr_batch_inverse: bytes of one staged piece of host data, a multiple of 32 up to 64 MiB (0 = 64 MiB)
    int opt_fr_scan_chunk = 0;            // ... vectors per launch, at most, 1..65535 (0 = the rule min(65535, max(1, 65536 / tiles per vector)) alone)
    int opt_lookup_spare_log = 0;         // kzg_lookup_setup: 1..4 gives next_pow2(n_t) << (v - 1) slots (0 = 2: load <= 0.5)
    int opt_lookup_hash_bits = 0;         // ... 1..32 keeps the low v - 1 bits of a key's hash and tag (0 = all); both are kept by the plan
    int opt_lookup_stage = 0;             // kzg_lookup_* / kzg_logup_terms: bytes of one staged piece of host data, a multiple of 32 up to 64 MiB (0 = 64 MiB)
    int opt_lookup_chunk = 0;             // ... vectors per chunk, at most, 1..65535 (0 = the rule alone)
    int opt_fr_program_block = 0;         // kzg_fr_program_run: threads of a workgroup, 64 / 128 / 256 (0 = the rule: 256 up to 4 temporaries, 128 up to 8, 64 above)
    int opt_sumcheck_block = 0;           // kzg_sumcheck_round: threads of a workgroup, 64 / 128 / 256 (0 = the rule by temporaries + accumulators, as above)
    int opt_sumcheck_grid = 0;            // ... workgroups of the strided grid, at most (0 = what the LDS lets the chip hold at once)
    int opt_mle_block = 0;                // kzg_mle_eq / _bind / _eval: threads of a workgroup of the level kernels, 64 / 128 / 256 (0 = 256)
    int opt_mle_local_log = 0;            // kzg_mle_eq / _eval: 1..10 levels (tables of up to 2^v scalars) inside one workgroup's LDS (0 = 10)
    int opt_mle_eval_chunk = 0;           // kzg_mle_eval: tables per chunk, at most, 1..65535 (0 = the rule min(65535, max(1, 2^21 / n)) alone)
    int opt_point_tree_leaf = 0;          // kzg_point_tree_setup: nodes of up to this many points are multiplied by the schoolbook kernels, a power of two <= 16 (0 = 16)
    int opt_g2_msm_slice = 0;             // kzg_msm_g2_bucket: points one workgroup sorts by digit, a power of two <= 2048 (0 = 2048)
    int opt_g2_msm_slots = 0;             // kzg_msm_g2_bucket: slice slots of the bucket arena = slices per chunk, 1..16 (0 = 16)
    int opt_host_pairing = 1;         // kzg_verify_cosets_batch, kzg_verify_eval_batch: the one pairing check runs on the calling thread (vcb_finish.h); 0 = in a one-thread kernel
    int opt_fk20_cosets_combine = 0;   // the coset combination of kzg_witness_cosets_*: 0 = Straus (shared doublings), 1 = mul256 per term
    int opt_g2_ntt_mul = 0;            // the twiddle products of the G2 DFT: 0 = psi split and one joint chain, 1 = signed digits over the whole scalar
    int opt_group_ntt_chunk_points = 0;   // kzg_ntt_g1 / kzg_ntt_g2: points per chunk of arrays, at most (0 = 2^21 for G1, 2^20 for G2)
    int opt_group_ntt_threads = 0;        // ... threads of one grid-stride launch = scratch slots, a power of two >= 256 (0 = 2^18 for G1, 2^17 for G2)
    int opt_g2_lagrange_dft_from = 2048;  // kzg_srs_lagrange_from_monomial_g2: sizes from this on run the G2 inverse DFT (below: one d-term sum per row)
    int opt_ntt_kernel = KZG_NTT_KERNEL_DEFAULT;  // 0: three-phase passes (k_ntt_pass1/2); 1: load/store fused into the first/last stage pair (k_ntt_tile); 2: 1 + two butterflies per thread
    int opt_ntt_three_from = 23;       // NTT sizes from 2^this on take three passes of <= 2^8 points (ntt_run3); 0 = never
    int opt_ntt_vec2_log = 1;          // pass 2: at most 2^v rows per tile (rows are contiguous: narrow tiles cost no coalescing on the load side)
    int opt_ntt_xcd = 1;               // XCD-aware tile order: bit 0 = pass 1, bit 1 = pass 2 (ntt.hip, xcd_tile)
    int opt_ntt_batch_chunk = 0;       // kzg_ntt_fr_batch: transforms per chunk; 0 = max(1, 2^21 / n)
    int opt_ntt_batch_rows_log = 0;    // ... log_n <= 12: 1 + log2 of the transforms per LDS tile; 0 = the rule (ntt.hip, ntt_rows_log)
    int opt_ntt_batch_loop_from = 0;   // ... sizes from 2^this on run as a loop of ntt_run; 0 = NTT_BATCH_LOOP_FROM
    int opt_accum_blocks_batch = 0;    // batched MSMs (0 = auto): leave 1/16 of the wave slots to the latency-bound tail and sort
                                       // kernels of the neighbouring MSMs in flight (measured +6 % throughput)
    int opt_tail_quads = 1;            // single MSMs: four lanes per point operation in the tail kernels (latency mode, msm_tail.hip)
    // kzg_msm_g1_batch: every k_accum_affine runs on one of this many dedicated streams, in submission order (0 = on its lane's
    // stream).  With the accumulation on the lanes' own streams the lanes fall into a convoy -- all sorting, then up to nine
    // accumulation kernels resident at once, then all in their tails -- and no accumulation kernel is resident 6 % of the time
    // (rocprofv3 kernel trace); two FIFO streams keep exactly the next one or two queued behind the running one: +3.5 %.
    // Needs its own hardware queues (GPU_MAX_HW_QUEUES >= lanes + 2): sharing a queue with a lane serialises them (-10 %).
    int opt_accum_streams = 2;
    // Small MSMs in a pipeline (sorted entries W * n <= opt_small_entries: up to 2^17 points): the per-thread costs of the equal
    // split (a partial sum written and folded per thread and per bucket boundary) weigh more the shorter a thread's chunk, so such
    // an MSM gets a smaller accumulation grid and the pipeline more accumulation streams to keep the chip full -- measured
    // (profiles/r04_small_grid_ab.txt) 160 blocks on 4 streams against 480 on 2: +49 % at 2^14, +39 % at 2^15, +20 % at 2^16, +9 % at
    // 2^17; at 2^20 four streams measure -1 %, so larger MSMs keep two.
    int opt_accum_streams_small = 4;
    int opt_accum_blocks_small = 160;
    int64_t opt_small_entries = 2 << 20;
    int planned_accum = 0;   // accumulation streams of the current plan (plan_pipeline): with fewer than three (a process short of
                             // hardware queues narrows the pipeline) the small grid would leave most of the chip idle, so the rule is off
    bool msm_small(size_t entries) const { return opt_accum_blocks_small > 0 && planned_accum >= 3 && (int64_t)entries <= opt_small_entries; }
    hipStream_t accum_streams[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> sorted_events, accum_events;  // per lane
    int opt_sort_threads = 1024;       // threads per k_hist / k_scatter block for a single MSM (one block per CU: 128 KiB of LDS)
    int opt_sort_threads_batch = 1024; // ... for batched MSMs
    int opt_host_affine = 1;           // a lone result bound for host memory is converted to affine / serialised on the host (emit.h)
    int opt_heavy_bins = 0;            // level 2 of the two-level sorts: 0 = slices for oversized bins once such bins have been seen (below), 1 = always, 2 = never
    bool opt_no_defer_tail = false;    // option defer_tail = 0: kzg_msm_g1_batch enqueues every MSM's tail right behind its accumulation (A/B)
    int opt_sort_single = 0;           // 1: c = 17 sorts in one pass (2^16 cursors, two walks) instead of the two-level sort
    int accum_blocks_single() const { return opt_accum_blocks ? opt_accum_blocks : 256 * KZG_ACCUM_WAVES; }
    int accum_blocks_batch() const { return opt_accum_blocks_batch ? opt_accum_blocks_batch : 240 * KZG_ACCUM_WAVES; }
    int num_cus = 256;
    std::atomic<bool> attr_msm_set{false}, attr_ntt_set{false}, attr_wide_set{false}, attr_sort20_set{false}, attr_horner_set{false}, attr_group_set{false}, attr_frscan_set{false}, attr_frprog_set{false}, attr_sumcheck_set{false};  // > 64 KiB dynamic-LDS opt-in done for this device
    // profiling
    bool prof = false;
    bool prof_only_accum = false;  // events around k_accum_affine only (bench.py's timed region: two events per kernel launch cost 1.4 % there)
    std::map<std::string, kzg::ProfEntry> prof_map;
    std::vector<kzg::PendingEvent> prof_pending;
    std::vector<hipEvent_t> event_pool;
    // caches
    std::map<uint32_t, kzg::NttPlan *> ntt_plans;          // key = log_n * 2 + inverse
    std::map<uint32_t, kzg::EvalDomainTables *> eval_tabs;  // key = log_d
    kzg::FixedBaseTable *fixed_base = nullptr;
    // distribute_powers (coset NTTs): per coset generator g two device tables g^j and g^(1024 j), j < 1024 (witness.hip)
    std::vector<std::pair<std::array<uint32_t, 8>, void *>> coset_tabs;
    // create_witness_batched: what depends on the opening POINTS only (Z, 1 / Z'(x_i), the coset shift, 1 / Z on the coset), kept
    // per point set for callers that open many polynomials at the same points (witness.hip, PointSetCache).  One pool of equal slots,
    // allocated by the first call that can use it; option "witness_cache_slots" (default 16, 0 = off; read before the pool exists).
    kzg::PointSetCache *point_sets = nullptr;
    int opt_witness_cache_slots = 16;
    // Oversized sort bins (msm_wide.hip).  A level-2 block that finds its bin oversized writes the MSM's sequence number (per lane,
    // Lane::heavy_seq) into the lane's word of d_lane_heavy; the host picks the words up with the results (finish_point,
    // batch_end) and notes the context's MSM count at that moment in heavy_last.  The three slice kernels are only enqueued for
    // the next KZG_HEAVY_WINDOW MSMs after such a pick-up (or option heavy_bins = 1): enqueued for nothing they cost uniform
    // scalars 0.8 % of the batched rate.  Setting the option clears the history.
    std::atomic<uint64_t> msm_count{0}, heavy_last{0};
    uint32_t *d_lane_heavy = nullptr;  // KZG_MAX_LANES words, then one per slot of the grouped pipeline (KZG_GROUP_DEPTH x KZG_MAX_GROUP)
    // The grouped shape of the batched pipeline (capi.hip, msm_batch_grouped): four streams carry a batch of the MSMs it covers,
    // whatever the hardware-queue pool of the process.  MSMs per sort / tail launch (option group_msms, 0 = never grouped: lanes).
    int opt_group_msms = 16;
    int plan_group = 0;  // group size of the current plan (plan_pipeline), 0 = the plan runs as lanes
    kzg::GroupSlot *group_tab = nullptr;  // device table, one entry per MSM of the call (grow-only)
    size_t group_tab_count = 0;
    std::vector<hipEvent_t> group_events;  // per arena half: sorted, accumulated on either FIFO stream, tail done
    uint32_t group_heavy_seq = 0;          // calls that took the grouped shape (what their slots' words are compared with)
    void *batch_out = nullptr;  // device staging of kzg_msm_g1_batch results (grow-only)
    size_t batch_out_bytes = 0;
};

struct kzg_srs {
    size_t n = 0;        // points
    size_t npad = 0;     // row stride (points)
    int c = 0;           // window bits (signed digits, 2^(c-1) buckets)
    int W = 0;           // windows = ceil(256 / c) (15 in the c = 17 single-pass mode); table row w holds 2^(c*w) * P_i
    int rows = 0;        // table rows resident (= W unless option window_rows asked for fewer: then an MSM takes ceil(W / rows) passes)
    bool narrow17 = false;  // c = 17: 15 windows, balanced scalars; two-level sort (or, option sort_single_pass, one pass walking the scalars twice)
    bool sort20 = false;    // c = 20: 13 windows, 2^19 buckets, two-level sort (msm_wide.hip); option sort_single_pass: the older two-pass path
    // Positional tables (naf = 18): the table holds 2^j P_i for EVERY bit position j (255 rows) instead of every c-th, and a
    // scalar is recoded in width-18 non-adjacent form: odd digits |d| < 2^17 at arbitrary positions, at least 18 apart -- 13.9
    // non-zero digits per 255-bit scalar on average instead of the 15 of fixed 17-bit windows (-7.4 % bucket additions) into
    // the same 2^16 buckets (bucket (|d| - 1) / 2, weight 2 b + 1).  c = 17 / W = 15 then describe the bucket count and the
    // maximum digits per scalar; rows = 255.  Costs 17x the table (32.6 KiB per point: 34 GB at 2^20), and the random gathers
    // over 34 GB cost 10 % more per entry than over 2 GB (profiles/r03_naf_tables.txt): opt-in (option naf_window = 18).
    int naf = 0;
    int row_shift = 0;   // row w holds 2^(row_shift w) P: c for window tables, 1 for positional tables
    kzg::G1Affine *table = nullptr;  // [W][npad], affine Montgomery
    void *table30 = nullptr;         // [W][npad] G1Affine30 (2 x 13 x 30-bit limbs + pad, KZG_ROW_BYTES = 128 B): what k_accum_affine gathers
    int device = 0;
};

namespace kzg {

struct Guard {  // exclusive use of the context for the scope
    std::lock_guard<CtxGate> lk;
    explicit Guard(kzg_ctx *c) : lk(c->mu) {}
};

// Shared use of the context for the scope: one leased lane (stream + arena).  Every blocking prover / verifier / transform call
// that works on ONE lane takes a Lease instead of a Guard (runtime.hip: lease_lane), so N host threads inside create_witness_batched,
// commit, fft, verify_poly ... run side by side on one context, as the reference's `&self` methods do (src/coeff_form.rs:59-111).
struct Lease {
    kzg_ctx *ctx = nullptr;
    int lane = -1;
    bool pipelined = false;  // others were in flight when the lane was leased: the call's accumulation goes to a FIFO accumulation stream
    uint32_t slot = 0;       // ... which one: slot modulo the number of streams MSMs of its size are spread over (lease_msm)
    ~Lease();
};
int lease_lane(kzg_ctx *ctx, Lease *ls);

struct StreamDrain {  // nothing of the call is in flight once its host-side buffers go out of scope
    hipStream_t st;
    ~StreamDrain() { hipStreamSynchronize(st); }
};

// validation of decoded points (what blstrs' G1Affine / G2Affine deserialisation enforces upstream):
//   POINTS_TRUSTED   nothing (the engine's own intermediate results)
//   POINTS_ON_CURVE  limbs canonical (< q) and on the curve
//   POINTS_SUBGROUP  + in the r-torsion subgroup ([r]P == O)
enum { POINTS_TRUSTED = 0, POINTS_ON_CURVE = 1, POINTS_SUBGROUP = 2 };

#define KZG_HIP_CHECK(ctx, expr)                                                                   \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return kzg::fail((ctx), KZG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define KZG_TRY(expr)                                                                              \
    do {                                                                                           \
        int _s = (expr);                                                                           \
        if (_s != KZG_OK) return _s;                                                               \
    } while (0)

// The message goes to the context (for callers that ask later from another thread) and to the calling thread's own slot:
// with several threads inside one context kzg_last_error returns the failure of the caller's own last call.
struct ThreadErr {
    const kzg_ctx *ctx = nullptr;
    std::string msg;
};
inline ThreadErr &thread_err() {
    static thread_local ThreadErr te;
    return te;
}
inline int fail(kzg_ctx *ctx, int code, const std::string &msg) {
    {
        std::lock_guard<std::mutex> lk(ctx->err_mu);
        ctx->err = msg;
    }
    ThreadErr &te = thread_err();
    te.ctx = ctx;
    te.msg = msg;
    return code;
}

// ---- arena ---------------------------------------------------------------------------------
int lane_reserve(kzg_ctx *ctx, int lane, size_t bytes);  // ensure arena >= bytes and reset it
void *lane_alloc(kzg_ctx *ctx, int lane, size_t bytes);  // 256-B aligned bump allocation (nullptr if exhausted)
int lane_pinned(kzg_ctx *ctx, int lane, size_t bytes);   // ensure pinned staging >= bytes
// runtime.hip: the pipeline plan of a context (lanes + accumulation streams on hardware queues of their own) and the shape of a lane
int ensure_lanes(kzg_ctx *ctx, int want);                                     // exclusive callers only
int plan_pipeline(kzg_ctx *ctx, int want, int *nl_out, int *nas_out);
void set_lane_mode(kzg_ctx *ctx, int lane, bool pipelined, bool deep);
int accum_streams_for(kzg_ctx *ctx, int planned, const kzg_srs *srs, size_t n);  // accumulation streams MSMs of this size are spread over

// ---- profiling -----------------------------------------------------------------------------
struct ProfScope {
    kzg_ctx *ctx;
    hipStream_t stream;
    hipEvent_t start = nullptr, stop = nullptr;
    const char *name;
    ProfScope(kzg_ctx *c, hipStream_t s, const char *n);
    ~ProfScope();
};
void prof_collect(kzg_ctx *ctx);

#define KZG_LAUNCH(ctx, stream, name, kern, grid, block, shmem, ...)                               \
    do {                                                                                           \
        kzg::ProfScope _ps((ctx), (stream), (name));                                               \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), (shmem), (stream), __VA_ARGS__);         \
    } while (0)

inline int untrusted_level(const kzg_ctx *ctx) { return ctx->opt_trusted_points ? POINTS_ON_CURVE : POINTS_SUBGROUP; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int ilog2_ceil(size_t x) {
    int l = 0;
    while (((size_t)1 << l) < x) l++;
    return l;
}

// The point type the MSM pipeline computes in and hands between its kernels: extended Jacobian coordinates in
// the signed 30-bit field representation (curve30.h).  Canonical encodings are produced by emit_point.
typedef G1Xyzz30 MsmPoint;

// ---- cross-TU entry points -------------------------------------------------------------------
// msm.hip
size_t msm_workspace_bytes(const kzg_srs *srs, size_t n);
// one MSM result (device) -> `ofmt` at `out` (host, or device with KZG_OUT_DEVICE); synchronises the lane's stream (capi.hip)
int finish_point(kzg_ctx *ctx, int lane, const MsmPoint *d_pt, void *out, int ofmt, int flags);
// d_scalars: device pointer to n scalars (sfmt); result: one device MsmPoint in the lane arena
// accum_stream (optional): run k_accum_affine there instead of on the lane's stream, ordered by the two caller-owned events
// `defer` (batched pipeline): when the accumulation kernel went to a FIFO stream, the part behind it (wait for it, fold, bucket
// reduction) is NOT enqueued: it is described in *defer and enqueued later by msm_finish -- after the lane's NEXT sort, so that the
// accumulation queue is fed before the lane's latency-bound tail kernels run (two MSMs in flight per lane, two workspaces).
struct MsmPending {
    bool active = false;
    hipStream_t st = nullptr;
    hipEvent_t accum_ev = nullptr;
    MsmMode mm;
    const MsmPoint *part = nullptr;
    MsmPoint *scratch = nullptr, *result = nullptr;
    const uint32_t *s1 = nullptr;
    int B = 0;
    size_t expected = 0;
    void *state = nullptr;
    char *tail_base = nullptr;
    size_t tail_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // TailLayout (msm_internal.h), opaque here
    bool odd = false;
};
int msm_run(kzg_ctx *ctx, int lane, const kzg_srs *srs, size_t offset, const void *d_scalars, size_t n, int sfmt,
            MsmPoint **d_result, hipStream_t accum_stream = nullptr, hipEvent_t sorted_ev = nullptr, hipEvent_t accum_ev = nullptr,
            MsmPending *defer = nullptr);
int msm_finish(kzg_ctx *ctx, MsmPending &pd, MsmPoint **d_result);  // the deferred part of an MSM (its result if it was not deferred)
// The grouped shape of the batched pipeline (capi.hip, msm_batch_grouped): the sort kernels of up to KZG_MAX_GROUP MSMs of a batch
// are ONE launch each, and so are their tail kernels; only k_accum_affine stays one launch per MSM.  A device table with one
// GroupSlot per MSM, written once per call, tells the kernels where each slot's scalars, workspace and result are.
struct GroupSlot {
    const void *scalars;  // the n scalars of the slot's MSM (device)
    char *base;           // the slot's workspace (msm_workspace_bytes; every intermediate array at its usual offset inside)
    void *out;            // where the slot's result goes (device)
    uint32_t *heavy;      // the slot's oversized-bin word (kzg_ctx::d_lane_heavy, behind the lanes' words)
};
bool msm_group_covers(const kzg_ctx *ctx, const kzg_srs *srs, size_t n);  // c = 17 window tables, 4-byte sort records, 2^17 points and more
int msm_group_sort(kzg_ctx *ctx, hipStream_t st, const kzg_srs *srs, size_t offset, size_t n, int sfmt, const GroupSlot *d_tab, int cnt,
                   uint32_t heavy_seq);
int msm_group_accum(kzg_ctx *ctx, hipStream_t st, const kzg_srs *srs, size_t n, char *base);  // one slot's k_accum_affine
int msm_group_tail(kzg_ctx *ctx, hipStream_t st, const kzg_srs *srs, size_t n, const GroupSlot *d_tab, int cnt, int ofmt);  // tail + results
// runtime.hip: one MSM on a leased lane (its accumulation kernel on the lease's FIFO stream when other calls are in flight)
int lease_msm(kzg_ctx *ctx, const Lease &ls, const kzg_srs *srs, size_t offset, const void *d_sc, size_t n, int sfmt, MsmPoint **res);
// d_points: count points -> one point (plain sum)
int sum_points_run(kzg_ctx *ctx, int lane, MsmPoint *d_points, size_t count, MsmPoint *d_scratch, MsmPoint **d_result);
// conversions between the canonical saturated XYZZ form and MsmPoint (device arrays)
int points_to30(kzg_ctx *ctx, hipStream_t st, const G1Xyzz *d_in, MsmPoint *d_out, size_t n);
int points_from30(kzg_ctx *ctx, hipStream_t st, const MsmPoint *d_in, G1Xyzz *d_out, size_t n);
int point_set_infinity(kzg_ctx *ctx, hipStream_t st, MsmPoint *d_pt);
size_t sum_points_scratch_count(size_t count);
// writes one point in `ofmt` (from XYZZ) to d_out (device); single thread incl. the Fq inversion
int emit_point(kzg_ctx *ctx, int lane, const MsmPoint *d_point, void *d_out, int ofmt);
size_t point_format_bytes(int fmt);
// out[g] = sum_i pts[g * gstride + i * istride], written in ofmt
int sum_groups_emit(kzg_ctx *ctx, int lane, const MsmPoint *d_pts, size_t count, size_t groups, size_t gstride, size_t istride,
                    MsmPoint *d_tmp, void *d_out, int ofmt);

// capi.hip
int msm_batch_strided(kzg_ctx *ctx, const kzg_srs *srs, size_t offset, const void *scalars, size_t n, size_t batch,
                      size_t stride_bytes, int sfmt, int flags, void *out, int ofmt, bool may_group = false);  // may_group: kzg_msm_g1_batch (the device group keeps its lanes)
// out[g] = sum_i points[g * gstride + i * istride] (strides in points); points in pfmt, host or device per flags
int g1_sum_batch_strided(kzg_ctx *ctx, const void *points, size_t count, size_t groups, size_t gstride, size_t istride, int pfmt,
                         int flags, void *out, int ofmt, int level = POINTS_ON_CURVE);

// srs.hip
int srs_choose_window(int opt_window_bits, size_t n);
void srs_shape(int opt_window_bits, int opt_window_rows, size_t n, int *c, int *W, int *rows, bool *narrow17, int opt_naf = 0, int *naf = nullptr);
// scalars' digits one MSM pass turns into sorted entries, at most
inline size_t srs_entries_per_scalar(const kzg_srs *s) { return s->naf ? (size_t)s->W : (size_t)s->rows; }
int srs_alloc(kzg_ctx *ctx, size_t n, kzg_srs **out);
int srs_finish_from_xyzz(kzg_ctx *ctx, kzg_srs *srs, G1Xyzz *d_row0_xyzz);  // batch-affine row 0 then precompute rows
int srs_precompute(kzg_ctx *ctx, kzg_srs *srs);                              // rows 1..W-1 from row 0
int batch_to_affine(kzg_ctx *ctx, hipStream_t stream, const G1Xyzz *d_in, G1Affine *d_out, size_t n);
int decode_points(kzg_ctx *ctx, hipStream_t st, const void *d_raw, size_t n, int fmt, G1Xyzz *d_out, int *d_bad,
                  int level = POINTS_SUBGROUP);

int fixed_base_mul(kzg_ctx *ctx, hipStream_t stream, const Fr *d_scalars_mont, size_t n, G1Xyzz *d_out);
int powers_run(kzg_ctx *ctx, hipStream_t st, const Fr &base_mont, size_t first, size_t n, Fr *d_out);  // base^(first+i)
int lagrange_scalars_run(kzg_ctx *ctx, hipStream_t st, const Fr &tau_mont, size_t d, Fr *d_out);      // L_i(tau)

// witness.hip
struct WitnessSink {
    const kzg_srs *srs;    // the SRS (or SRS shard) the quotient MSM runs against
    size_t first, len;     // it holds the points of the quotient coefficients [first, first + len)
    size_t total;          // length of the whole SRS (the reference's slice bound)
    void *d_partial;       // nullptr: witness to the caller; else the 144-byte Jacobian partial goes here (device)
};
int witness_coeff_batched_run(kzg_ctx *ctx, const WitnessSink &sink, const void *coeffs, size_t n, const void *xs, const void *ys,
                              size_t k, int sfmt, int flags, void *out_w, int ofmt, void *out_r, size_t *out_r_len);
int vanishing_poly_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_xs_mont, size_t k, Fr *d_z, Fr *d_tmp);  // k+1 coeffs each
// coset_fft / icoset_fft with shift g (src/ft.rs:142-178): v[i] *= g^i then the transform; the inverse transform then v[i] *= g^-i.
// nnz (forward only): d[nnz ..) is zero, so only d[0, nnz) is scaled
int coset_ntt_run(kzg_ctx *ctx, int lane, Fr *d, uint32_t log_n, int inverse, const Fr &g, size_t nnz = (size_t)-1);
// the same for `batch` vectors, vector b at d + b * stride, on ntt_batch_run: one scaling launch for the whole batch
int coset_ntt_batch_run(kzg_ctx *ctx, int lane, Fr *d, uint32_t log_n, size_t batch, size_t stride, int inverse, const Fr &g);

// cached per-context tables, released by kzg_ctx_destroy
void ntt_plans_free(kzg_ctx *ctx);   // ntt.hip
void eval_tabs_free(kzg_ctx *ctx);   // poly.hip
void fixed_base_free(kzg_ctx *ctx);  // srs.hip

// ntt.hip
int ntt_run(kzg_ctx *ctx, int lane, Fr *d_data, uint32_t log_n, int inverse, size_t nnz = (size_t)-1);  // nnz: d_data[nnz ..) is zero (assumed, not read)
// arena bytes ONE ntt_run of 2^log_n points takes from its lane (never returned before the call ends): the two-pass scratch; above
// 2^24 the transposed copy, the inner transform's scratch and the outer twiddle tables
inline size_t ntt_workspace_bytes(uint32_t log_n) {
    const size_t n = (size_t)1 << log_n;
    return log_n > 24 ? n * 32 + ((size_t)1 << 24) * 32 + (2 << 20) : n * 32 + 4096;
}
bool ntt_short_input_ok(uint32_t log_n, size_t nnz);  // ntt_run(..., nnz) will not read d_data[nnz ..)
// `batch` transforms of 2^log_n points in place, transform b at d_data + b * stride (stride >= n, in elements); chunked, see ntt.hip
constexpr uint32_t NTT_BATCH_LOOP_FROM = 20;  // from this size on the batch is a loop of ntt_run (measured: DESIGN.md, batched NTT)
int ntt_batch_run(kzg_ctx *ctx, int lane, Fr *d_data, uint32_t log_n, size_t batch, size_t stride, int inverse);
bool ntt_batch_looped(const kzg_ctx *ctx, uint32_t log_n);                             // ... as one ntt_run per transform
size_t ntt_batch_chunk(const kzg_ctx *ctx, uint32_t log_n);                            // transforms per chunk
size_t ntt_batch_workspace_bytes(const kzg_ctx *ctx, uint32_t log_n, size_t batch);  // arena bytes one ntt_batch_run takes from its lane
int pow_table(kzg_ctx *ctx, hipStream_t stream, const Fr &base_mont, const Fr &scale_mont, size_t count, Fr *d_out);
Fr host_omega(uint32_t exp);  // Montgomery-form 2^exp-th root of unity per compute_omega (src/ft.rs:73)

// poly.hip
int fr_convert(kzg_ctx *ctx, hipStream_t stream, Fr *d_data, size_t n, int to_mont);  // in place
int batch_inverse(kzg_ctx *ctx, hipStream_t stream, const Fr *d_in, Fr *d_out, size_t n);
// kzg_fr_batch_inverse: the same kernel with the running products at d_pre (d_out, or scratch when d_in == d_out), canonical words
// in and out if canon, and the zeros counted into *d_zeros
int batch_inverse_pub(kzg_ctx *ctx, hipStream_t stream, const Fr *d_in, Fr *d_out, Fr *d_pre, size_t n, bool canon, unsigned long long *d_zeros);
// d_a[i] *= 1 / d_c[i] (zeros of c: a[i] = 0 and *d_flag |= 1); d_tmp: n elements of scratch
int batch_inverse_mul(kzg_ctx *ctx, hipStream_t stream, const Fr *d_c, Fr *d_a, Fr *d_tmp, size_t n, int *d_flag);
// Horner machinery: eval and linear quotient. d_coeffs in Montgomery or canonical form (linear ops:
// the result is in the same form provided x_mont is Montgomery).
int poly_eval_run(kzg_ctx *ctx, int lane, const Fr *d_coeffs, size_t n, const Fr &x_mont, Fr *d_y_out);
int eval_tables_ready(kzg_ctx *ctx, int lane, uint32_t log_d);
int quotient_linear_run(kzg_ctx *ctx, int lane, const Fr *d_coeffs, size_t n, const Fr &x_mont, Fr *d_q_out,
                        Fr *d_px_out);
int quotient_eval_run(kzg_ctx *ctx, int lane, const Fr *d_evals, uint32_t log_d, size_t m, int sfmt, Fr *d_q_out);

// open_eval.hip: evaluation-form polynomials at any point of Fr
constexpr int OE_MAX_CHUNK = 16;  // polynomials per chunk (the most lanes option "streams" allows)
struct OpenPoint {                // an opening point, classified on the host
    Fr z;                         // Montgomery
    Fr c;                         // (z^d - 1) / d; zero on the domain
    bool on_domain;               // z = w^m
    size_t m;
};
int open_point_classify(uint32_t log_d, const Fr &z_mont, OpenPoint *pt);  // KZG_ERR_INTERNAL: the walk over the bits of m broke down
size_t open_eval_fr_workspace_bytes(size_t d, size_t B);                   // arena bytes one open_eval_fr_run of B polynomials takes
size_t open_eval_fr_workspace_bytes(size_t d, size_t B, size_t nz);        // ... when they have at most nz distinct points
// y (d_y + b) and, unless d_q is null, the quotient (d_q + b d) of B <= OE_MAX_CHUNK polynomials (d_evals + b d) at pts[b], on the lane's stream
int open_eval_fr_run(kzg_ctx *ctx, int lane, const Fr *d_evals, uint32_t log_d, size_t B, const OpenPoint *pts, int sfmt, Fr *d_y, Fr *d_q);

// the evaluation stage with the polynomial of a claim named by an index (kzg_multiopen_eval_commit): the power table of the domain
// (open_powtab_bytes(d) bytes at d_tab), the inverses d_inv[u d + i] = 1 / (w^i - z_u) of nz <= OE_MAX_CHUNK off-domain points (d_den:
// scratch of the same nz x d scalars), and y[b] = p_{vidx[b]}(z_{pu[b]}) for B claims from them; every table is device memory
size_t open_powtab_bytes(size_t d);
int open_powtab_run(kzg_ctx *ctx, hipStream_t st, uint32_t log_d, Fr *d_tab);
int open_inverses_run(kzg_ctx *ctx, hipStream_t st, uint32_t log_d, const Fr *d_tab, const Fr *z_mont, int nz, Fr *d_den, Fr *d_inv);
int open_eval_values_idx_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_evals, uint32_t log_d, const Fr *d_inv, const uint32_t *d_vidx,
                             const uint32_t *d_pu, const Fr *d_z, const Fr *d_c, size_t B, Fr *d_partial, Fr *d_y);

// fold.hip: d_out[g d + j] = sum_{i < t} gamma_g^i d_v[g gstride + i d + j], g < groups (gammas Montgomery, on the device); with carry
// the sum starts from d_out[g d + j] gamma_g^t: pieces of a group folded from the last one down
int fold_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, size_t t, size_t gstride, size_t groups, const Fr *d_gammas_mont,
             bool carry, Fr *d_out);

// multiopen.hip: d_out[j] (+)= sum_{k < count} d_weight[k] d_v[d_idx[k] d + j], j < d (weights Montgomery; the output has the inputs' form)
int lincomb_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const Fr *d_weight, size_t count, bool carry,
                Fr *d_out);
// d_y[s] = d_v[d_idx[s] d + d_at[s]] for s < count (the values at points of the domain, as they are stored)
int multiopen_gather_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const uint32_t *d_at, size_t count, Fr *d_y);
// One chunk of nz <= OE_MAX_CHUNK distinct off-domain points: d_Y[u] = sum_{k in u} d_w[k] d_y[k] on the device, then
// d_g[j] += sum_u (sum_{k in u} d_w[k] d_v[d_idx[k] d + j] - d_Y[u]) d_inv[u d + j]; the claims of point u are [d_pstart[u], d_pstart[u + 1])
int multiopen_accum_run(kzg_ctx *ctx, hipStream_t st, const Fr *d_v, size_t d, const uint32_t *d_idx, const Fr *d_w, const uint32_t *d_pstart,
                        int nz, const Fr *d_y, Fr *d_Y, const Fr *d_inv, Fr *d_g);

// poly_divide.hip: d_g[0, m) = 1 / f mod X^m (f: fl_all <= m Montgomery coefficients, f[0] != 0) by a schoolbook base of
// min(base, 64, m) coefficients and Newton doubling through ntt_run.  d_A, d_G: scratch of 2^ilog2_ceil(2 m - 1) elements each; the
// lane's arena must have ntt_workspace_bytes(ilog2_ceil(2 m - 1)) left.  Behind kzg_poly_divide and kzg_point_tree_setup.
int series_inverse_run(kzg_ctx *ctx, int lane, const Fr *d_f, size_t fl_all, size_t m, size_t base, Fr *d_g, Fr *d_A, Fr *d_G);
// The division by ONE divisor b (nb >= 2 coefficients) as stages on device memory, behind kzg_poly_divide and kzg_witness_coeff_tree:
// poly_divisor_shape fills the sizes for dividends of na coefficients; the caller provides the buffers (elements): f fl_all, g m,
// G and A Tq each and, for remainders, B, af, qf N each, tmp0 t0, tmp1 t1; the lane's arena must have
// ntt_workspace_bytes(max(log_tq, log_N)) left.  poly_divisor_run (m >= 1) once per divisor -- bd on the device, converted to
// Montgomery form if to_m --, poly_dividend_run per dividend: q and r keep the dividend's form, *flag is cleared at a non-zero
// remainder coefficient.  poly_pad_run: a dividend shorter than the divisor, reduced and zero-padded, is its own remainder.
struct PolyDivisor {
    size_t na, nb, m, nr, Tq, N, fl_all, t0, t1;
    uint32_t log_tq, log_N;
    Fr *f, *g, *G, *A, *B, *af, *qf, *tmp0, *tmp1;
};
void poly_divisor_shape(size_t na, size_t nb, PolyDivisor *d);
int poly_divisor_run(kzg_ctx *ctx, int lane, const Fr *bd, int to_m, bool want_r, const PolyDivisor &d);
int poly_dividend_run(kzg_ctx *ctx, int lane, const PolyDivisor &d, const Fr *ai, Fr *qi, bool want_r, Fr *ri, int *flag);
int poly_pad_run(kzg_ctx *ctx, hipStream_t st, const Fr *src, size_t cnt, Fr *dst, size_t total);

// point_tree.hip: batched transforms of 2^log_t points over `total` contiguous elements (total a multiple of 2^log_t), in place.
// dit = 0: natural order in, bit-reversed spectrum out (decimation in frequency); dit = 1: bit-reversed in, natural out.  tw is
// the table w^j, j < 2^(log_tw - 1), of a 2^log_tw-th root w (or of 1 / w), log_tw >= log_t: no scaling is applied.
int pt_ntt_run(kzg_ctx *ctx, hipStream_t st, Fr *d, size_t total, uint32_t log_t, int dit, const Fr *tw, uint32_t log_tw);
// a kzg_point_tree as the prover and the verifier on a plan (witness_tree.hip) read it: product = M, k + 1 Montgomery coefficients
// resident on `device`; K: the padded size; distinct = 0: two points coincide
struct PointTreeView {
    int device;
    size_t k, K;
    int distinct;
    const Fr *product;
};
void point_tree_view(const kzg_point_tree *plan, PointTreeView *v);
// the interpolation of kzg_point_tree_interpolate on device memory: d_out[u k + j] = coefficient j of the polynomial through
// (x_i, d_ys[u k + i]) for `units` vectors, in the values' form; d_R: units x 2K, d_A: units x K elements of scratch (distinct plans only)
int point_tree_interpolate_run(kzg_ctx *ctx, hipStream_t st, const kzg_point_tree *plan, const Fr *d_ys, size_t units, Fr *d_R, Fr *d_A, Fr *d_out);


}  // namespace kzg
