// The host-only parts of kzg_amd/csrc/mle.hip (mle_host.h): the degree bound behind kzg_fr_program_degree, the shape rules of
// kzg_sumcheck_round and the aliasing rules of kzg_mle_bind, on hand-computed cases.  No GPU and no library: this program includes the
// header alone, so it is also the place for a -fsanitize=address,undefined build.  The exit status names the failed step.
#include <cstdio>
#include <vector>

#include "../kzg_amd/csrc/mle_host.h"
using namespace kzg;

static void push(std::vector<uint32_t> &w, int op, int dk, uint32_t dst, int ak, uint32_t a, int bk, uint32_t b, int32_t sa = 0, int32_t sb = 0) {
    const uint32_t i[KZG_FRP_WORDS] = {(uint32_t)op | (uint32_t)dk << 8 | (uint32_t)ak << 16 | (uint32_t)bk << 24, dst, a, b, (uint32_t)sa, (uint32_t)sb};
    w.insert(w.end(), i, i + KZG_FRP_WORDS);
}

int main() {
    const int C = KZG_FRP_COL, K = KZG_FRP_CONST, T = KZG_FRP_TEMP, O = KZG_FRP_OUT, A = KZG_FRP_ADD, S = KZG_FRP_SUB, M = KZG_FRP_MUL;
    {   // const + const: 0; col - const: 1; (col col)^2 + col: 4; the same times a const: 4
        std::vector<uint32_t> w;
        push(w, A, O, 0, K, 0, K, 0);
        push(w, S, O, 1, C, 0, K, 0);
        push(w, M, T, 0, C, 0, C, 1);
        push(w, M, T, 0, T, 0, T, 0);
        push(w, A, O, 2, T, 0, C, 0);
        push(w, M, O, 3, T, 0, K, 0);
        size_t d[5] = {9, 9, 9, 9, 77};
        frp_degrees(w.data(), w.size() / KZG_FRP_WORDS, 4, d);
        if (d[0] != 0 || d[1] != 1 || d[2] != 4 || d[3] != 4 || d[4] != 77) return 1;
        if (frp_has_shift(w.data(), w.size() / KZG_FRP_WORDS)) return 2;
        push(w, M, T, 1, C, 0, K, 0, 0, 0);
        push(w, M, T, 1, C, 0, C, 1, 0, -1);
        if (!frp_has_shift(w.data(), w.size() / KZG_FRP_WORDS)) return 3;
    }
    {   // forty squarings: 2^41 saturates at 2^32 - 1, and a sum keeps the maximum
        std::vector<uint32_t> w;
        push(w, M, T, 15, C, 0, C, 0);
        for (int k = 0; k < 40; k++) push(w, M, T, 15, T, 15, T, 15);
        push(w, A, O, 0, T, 15, C, 0);
        push(w, M, O, 1, T, 15, T, 15);
        size_t d[2] = {0, 0};
        frp_degrees(w.data(), w.size() / KZG_FRP_WORDS, 2, d);
        if (d[0] != 0xFFFFFFFFull || d[1] != 0xFFFFFFFFull) return 4;
    }
    // the accumulator rule: 1 <= n_eval <= 16 and n_out n_eval <= 32
    if (!sumcheck_shape_ok(1, 1) || !sumcheck_shape_ok(1, 16) || !sumcheck_shape_ok(2, 16) || !sumcheck_shape_ok(32, 1) || !sumcheck_shape_ok(3, 10)) return 5;
    if (sumcheck_shape_ok(1, 0) || sumcheck_shape_ok(1, 17) || sumcheck_shape_ok(3, 11) || sumcheck_shape_ok(33, 1) || sumcheck_shape_ok(0, 1) ||
        sumcheck_shape_ok(64, (size_t)-1 / 2))
        return 6;
    {   // aliasing: two columns of n = 8 scalars (256 bytes) in one arena, outputs of 4 scalars (128 bytes)
        static unsigned char arena[2048];
        const size_t n = 8;
        const void *cols[2] = {arena, arena + 256};
        void *in_place[2] = {arena, arena + 256};
        if (mle_bind_alias(cols, in_place, 2, n, true) != -1) return 7;
        void *apart[2] = {arena + 512, arena + 640};                       // back to back
        if (mle_bind_alias(cols, apart, 2, n, true) != -1) return 8;
        void *mixed[2] = {arena, arena + 512};                             // one in place, one not
        if (mle_bind_alias(cols, mixed, 2, n, true) != -1) return 9;
        void *upper[2] = {arena + 128, arena + 512};                       // the upper half of its own column
        if (mle_bind_alias(cols, upper, 2, n, true) != 0) return 10;
        void *other[2] = {arena + 512, arena};                             // another column
        if (mle_bind_alias(cols, other, 2, n, true) != 1) return 11;
        void *tail[2] = {arena + 512, arena + 511};                        // the last byte of a column
        if (mle_bind_alias(cols, tail, 2, n, true) != 1) return 12;
        void *same[2] = {arena + 512, arena + 512};
        if (mle_bind_alias(cols, same, 2, n, true) != 1) return 13;
        void *lapped[2] = {arena + 512, arena + 639};                      // one byte of another output
        if (mle_bind_alias(cols, lapped, 2, n, true) != 1) return 14;
        const void *twice[2] = {arena, arena};                             // one column twice, both in place
        void *twice_out[2] = {arena, arena};
        if (mle_bind_alias(twice, twice_out, 2, n, true) != 0) return 15;   // (output 0 already meets column 1)
        const void *shifted[2] = {arena, arena + 32};                      // in place under another column's feet
        void *shifted_out[2] = {arena, arena + 1024};
        if (mle_bind_alias(shifted, shifted_out, 2, n, true) != 0) return 16;
        // different memories: addresses of columns and outputs may coincide, the outputs still may not
        if (mle_bind_alias(cols, other, 2, n, false) != -1 || mle_bind_alias(cols, same, 2, n, false) != 1) return 17;
    }
    printf("ok\n");
    return 0;
}
