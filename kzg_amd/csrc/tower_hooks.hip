// tower_hooks.hip -- kzg_test_tower (include/kzg_mi355x_test.h): the device twin of ht_tower_op of tests/host_tower.cpp.  Linked into
// libkzg_mi355x_hooks.so only, and compiled the way pairing.hip is (a plain hipcc -c, not the assembly post-processing of the MSM
// kernels), so the tests see tower.h as the verifier kernels run it: out-of-line functions on operands in scratch memory, one thread
// per record, 64 threads per block.  The record-level bodies are tower_hooks.h, the same source the host shim compiles.
#include "common.h"
#include "tower_hooks.h"

namespace kzg {
namespace {

template <int OP>
__global__ __launch_bounds__(64) void k_test_tower(const uint32_t *in, size_t n, uint32_t *out, Fq2 *tabs) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr size_t IN = kTowerShapes[OP].in_rec / 4, OUT = kTowerShapes[OP].out_rec / 4;  // records are whole words on a 256-B base
    tower_record<OP>(in + i * IN, out + i * OUT, tabs ? tabs + i * TT_TABS_PER_RECORD : nullptr);
}

// the kernel of a run-time op: k_test_tower<op>
template <int OP>
int launch_tower(kzg_ctx *ctx, hipStream_t st, int op, const uint32_t *din, size_t n, uint32_t *dout, Fq2 *tabs) {
    if (op == OP) {
        KZG_LAUNCH(ctx, st, "k_test_tower", k_test_tower<OP>, (unsigned)((n + 63) / 64), 64, 0, din, n, dout, tabs);
        return KZG_OK;
    }
    if constexpr (OP + 1 < KZG_TOWER_NUM_OPS) return launch_tower<OP + 1>(ctx, st, op, din, n, dout, tabs);
    return fail(ctx, KZG_ERR_SHAPE, "kzg_test_tower: unknown op");
}

}  // namespace
}  // namespace kzg

using namespace kzg;

extern "C" int kzg_test_tower(kzg_ctx *ctx, int op, const void *in, size_t in_rec, size_t n, void *out, size_t out_rec) {
    if (!ctx || !in || !out || !n || n > ((size_t)1 << 12)) return KZG_ERR_SHAPE;
    if (op < 0 || op >= KZG_TOWER_NUM_OPS) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_tower: unknown op");
    if (in_rec != kTowerShapes[op].in_rec || out_rec != kTowerShapes[op].out_rec) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_tower: record size");
    for (size_t i = 0; i < n; i++) {
        uint32_t w[290];  // the longest input record (MILLER_LOOP)
        memcpy(w, (const uint8_t *)in + i * in_rec, in_rec);
        if (!tower_record_ok(op, w)) return fail(ctx, KZG_ERR_SHAPE, "kzg_test_tower: record out of contract");
    }
    Guard g(ctx);
    KZG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t tab_bytes = tower_op_needs_tabs(op) ? n * TT_TABS_PER_RECORD * sizeof(Fq2) : 0;
    KZG_TRY(lane_reserve(ctx, 0, n * (in_rec + out_rec) + tab_bytes + 65536));
    hipStream_t st = ctx->lanes[0].stream;
    void *din = lane_alloc(ctx, 0, n * in_rec), *dout = lane_alloc(ctx, 0, n * out_rec);
    Fq2 *tabs = tab_bytes ? (Fq2 *)lane_alloc(ctx, 0, tab_bytes) : nullptr;
    if (!din || !dout || (tab_bytes && !tabs)) return fail(ctx, KZG_ERR_ALLOC, "workspace");
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(din, in, n * in_rec, hipMemcpyHostToDevice, st));
    KZG_TRY(launch_tower<0>(ctx, st, op, (const uint32_t *)din, n, (uint32_t *)dout, tabs));
    KZG_HIP_CHECK(ctx, hipGetLastError());
    KZG_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, n * out_rec, hipMemcpyDeviceToHost, st));
    KZG_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return KZG_OK;
}
