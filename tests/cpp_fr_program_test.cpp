// Exercises FrProgram and fr_program_run of include/kzg_mi355x.hpp on the GPU: the standard gate q_L a + q_R b + q_O c + q_M a b + q_C
// with a rotated and a periodic column on small integers against values worked out by hand (the Python suite pins the bytes to the
// integer model).  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> ints(std::initializer_list<uint64_t> xs) {
    std::vector<Scalar> v;
    for (uint64_t x : xs) v.push_back(Scalar::from_u64(x));
    return v;
}

static void push(std::vector<uint32_t> &w, const std::array<uint32_t, KZG_FRP_WORDS> &i) { w.insert(w.end(), i.begin(), i.end()); }

int main() {
    Engine e(0);
    const int C = KZG_FRP_COL, K = KZG_FRP_CONST, T = KZG_FRP_TEMP, O = KZG_FRP_OUT;
    // columns 0..2: a, b, c; 3..7: q_L q_R q_O q_M q_C; column 8: two periodic values; const 0: a challenge
    std::vector<uint32_t> w;
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 0, C, 3, C, 0));        // t0 = q_L a
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 1, C, 4, C, 1));        // t1 = q_R b
    push(w, FrProgram::instruction(KZG_FRP_ADD, T, 0, T, 0, T, 1));
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 1, C, 5, C, 2));        // t1 = q_O c
    push(w, FrProgram::instruction(KZG_FRP_ADD, T, 0, T, 0, T, 1));
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 1, C, 0, C, 1));        // t1 = a b
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 1, T, 1, C, 6));
    push(w, FrProgram::instruction(KZG_FRP_ADD, T, 0, T, 0, T, 1));
    push(w, FrProgram::instruction(KZG_FRP_ADD, O, 0, T, 0, C, 7));        // out0 = the gate
    push(w, FrProgram::instruction(KZG_FRP_SUB, T, 2, C, 0, C, 0, 1, -1)); // t2 = a[i + 1] - a[i - 1]
    push(w, FrProgram::instruction(KZG_FRP_MUL, T, 2, T, 2, C, 8));
    push(w, FrProgram::instruction(KZG_FRP_ADD, O, 1, T, 2, K, 0));        // out1 = (a[i + 1] - a[i - 1]) p[i mod 2] + k
    FrProgram plan(e, w, 9, 1, 2);
    if (plan.instructions() != 12 || plan.columns() != 9 || plan.consts() != 1 || plan.outputs() != 2 || plan.temps() != 3 || plan.multiplications() != 6) return 1;
    const size_t n = 4;
    const std::vector<std::vector<Scalar>> cols = {ints({1, 2, 3, 4}),     ints({5, 6, 7, 8}), ints({9, 10, 11, 12}), ints({2, 0, 1, 3}), ints({0, 3, 1, 1}),
                                                   ints({1, 1, 0, 2}),     ints({1, 2, 0, 1}), ints({7, 0, 5, 1}),   ints({2, 3})};
    const std::vector<std::vector<Scalar>> got = fr_program_run(plan, cols, ints({100}), n);
    // gate: 2*1 + 0 + 9 + 5 + 7 = 23; 0 + 18 + 10 + 24 + 0 = 52; 3 + 7 + 0 + 0 + 5 = 15; 12 + 8 + 24 + 32 + 1 = 77
    if (got.size() != 2 || !(got[0] == ints({23, 52, 15, 77}))) return 2;
    // rows 1 and 2: (3 - 1) * 3 + 100, (4 - 2) * 2 + 100; row 3 wraps forward: (1 - 3) * 3 + 100 = 94; row 0 wraps back: (2 - 4) * 2 + 100 = 96
    if (!(got[1] == ints({96, 106, 104, 94}))) return 3;
    try {
        fr_program_run(plan, cols, ints({100}), 3);                        // four rows are neither n = 3 nor a power of two dividing it
        return 4;
    } catch (const ReferencePanic &) {
    }
    try {
        std::vector<uint32_t> bad;
        push(bad, FrProgram::instruction(KZG_FRP_ADD, O, 0, T, 0, C, 0));  // a temporary nobody wrote
        FrProgram p2(e, bad, 1, 0, 1);
        return 5;
    } catch (const ReferencePanic &) {
    }
    FrProgram moved(std::move(plan));
    if (moved.outputs() != 2 || plan.handle() != nullptr) return 6;
    printf("ok\n");
    return 0;
}
