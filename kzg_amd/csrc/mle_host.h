// mle_host.h -- the host-only parts of mle.hip, free of HIP so that a plain C++ program can test them (tests/cpp_mle_test.cpp):
// the degree bound of a program's outputs, the shape rules of kzg_sumcheck_round and the aliasing rules of kzg_mle_bind.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/kzg_mi355x.h"

namespace kzg {

// degrees[o], o < n_out: an upper bound of the total degree of output o in the columns of a VALIDATED program (kzg_fr_program_setup):
// a const counts 0, a column 1, add / sub the maximum, mul the sum; saturating at 2^32 - 1
inline void frp_degrees(const uint32_t *words, size_t n_insns, size_t n_out, size_t *degrees) {
    const uint64_t SAT = 0xFFFFFFFFull;
    uint64_t temp[KZG_FRP_MAX_TEMPS] = {0};
    for (size_t o = 0; o < n_out; o++) degrees[o] = 0;
    for (size_t k = 0; k < n_insns; k++) {
        const uint32_t *w = words + k * KZG_FRP_WORDS;
        const uint32_t op = w[0] & 0xFF, dk = (w[0] >> 8) & 0xFF, kinds[2] = {(w[0] >> 16) & 0xFF, w[0] >> 24};
        uint64_t d[2];
        for (int s = 0; s < 2; s++)
            d[s] = kinds[s] == KZG_FRP_COL ? 1 : kinds[s] == KZG_FRP_TEMP ? temp[w[2 + s] % KZG_FRP_MAX_TEMPS] : 0;
        uint64_t r = op == KZG_FRP_MUL ? d[0] + d[1] : d[0] > d[1] ? d[0] : d[1];
        if (r > SAT) r = SAT;
        if (dk == KZG_FRP_TEMP) temp[w[1] % KZG_FRP_MAX_TEMPS] = r;
        else if (w[1] < n_out) degrees[w[1]] = (size_t)r;
    }
}

// a column operand with a non-zero shift: a rotation has no meaning on the hypercube
inline bool frp_has_shift(const uint32_t *words, size_t n_insns) {
    for (size_t k = 0; k < n_insns; k++) {
        const uint32_t *w = words + k * KZG_FRP_WORDS;
        if ((((w[0] >> 16) & 0xFF) == KZG_FRP_COL && w[4]) || ((w[0] >> 24) == KZG_FRP_COL && w[5])) return true;
    }
    return false;
}

// kzg_sumcheck_round: 1 <= n_eval <= 16 points and at most 32 accumulators
inline bool sumcheck_shape_ok(size_t n_out, size_t n_eval) {
    return n_eval >= 1 && n_eval <= (size_t)KZG_SUMCHECK_MAX_EVAL && n_out >= 1 && n_out <= (size_t)KZG_SUMCHECK_MAX_ACC &&
           n_out * n_eval <= (size_t)KZG_SUMCHECK_MAX_ACC;
}

inline bool mle_ranges_meet(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// kzg_mle_bind: the first output that breaks the aliasing rules, or -1.  Output c covers n / 2 scalars; it may BE column c (in place)
// and otherwise meets no column and no other output.  same_space = false: columns and outputs lie in different memories (one of
// KZG_IN_DEVICE / KZG_OUT_DEVICE), so only the outputs are compared with each other.
inline long mle_bind_alias(const void *const *cols, void *const *outs, size_t n_cols, size_t n, bool same_space) {
    const size_t col_bytes = n * 32, out_bytes = n / 2 * 32;
    for (size_t c = 0; c < n_cols; c++) {
        const uintptr_t o = (uintptr_t)outs[c];
        if (same_space)
            for (size_t k = 0; k < n_cols; k++) {
                if (k == c && outs[c] == cols[c]) continue;
                if (mle_ranges_meet(o, out_bytes, (uintptr_t)cols[k], col_bytes)) return (long)c;
            }
        for (size_t q = 0; q < c; q++)
            if (mle_ranges_meet(o, out_bytes, (uintptr_t)outs[q], out_bytes)) return (long)c;
    }
    return -1;
}

}  // namespace kzg
