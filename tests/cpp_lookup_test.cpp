// Exercises LookupTable, lookup_count and logup_terms of include/kzg_mi355x.hpp on the GPU: owners and multiplicities of small
// integers against counts worked out by hand, the terms through identities checked with kzg_fr_vec_mul and fr_scan (the Python
// suite pins the bytes to the integer model).  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> ints(std::initializer_list<uint64_t> xs) {
    std::vector<Scalar> v;
    for (uint64_t x : xs) v.push_back(Scalar::from_u64(x));
    return v;
}

int main() {
    Engine e(0);
    const Scalar one = Scalar::from_u64(1);
    // row 3 repeats row 1: row 1 owns the value 20
    LookupTable plan(e, ints({10, 20, 30, 20}));
    if (plan.len() != 4 || plan.distinct() != 3 || plan.bytes() < 4 * 32) return 1;
    const std::vector<Scalar> values = ints({20, 30, 30, 99, 10, 10, 10, 30, 20, 10});    // two vectors of five
    std::vector<uint32_t> idx;
    std::vector<size_t> missing, first;
    std::vector<Scalar> m = lookup_count(plan, values, 5, &idx, &missing, &first);
    if (!(m == ints({1, 1, 2, 0, 3, 1, 1, 0}))) return 2;
    if (idx != std::vector<uint32_t>{1, 2, 2, 0xFFFFFFFFu, 0, 0, 0, 2, 1, 0}) return 3;
    if (missing != std::vector<size_t>{1, 0} || first != std::vector<size_t>{3, SIZE_MAX}) return 4;
    try {
        lookup_count(plan, values, 5);  // 99 is in no row and nobody asked where
        return 5;
    } catch (const ReferencePanic &) {
    }
    if (!(lookup_count(plan, ints({10, 20, 30}), 3) == ints({1, 1, 1, 0}))) return 6;
    try {
        lookup_count(plan, values, 3);  // ten scalars are no whole number of vectors of three
        return 7;
    } catch (const ReferencePanic &) {
    }
    LookupTable moved(std::move(plan));
    if (moved.len() != 4 || plan.handle() != nullptr) return 8;
    // the sum alone: term * (beta + w) = 1
    const uint64_t beta = 1000;
    const size_t n = 4;
    const std::vector<Scalar> table = ints({10, 20, 30, 40}), column = ints({20, 30, 30, 10});
    std::vector<Scalar> inv = logup_terms(e, column, {}, {}, Scalar::from_u64(beta), n, 1);
    const std::vector<Scalar> den = ints({beta + 20, beta + 30, beta + 30, beta + 10});
    e.check(kzg_fr_vec_mul(e.ctx(), inv.data(), den.data(), n, KZG_FR_CANONICAL_LE_32, 0));
    for (const Scalar &x : inv)
        if (!(x == one)) return 9;
    // the whole argument: multiplicities from the plan, the terms, their running sum ends at zero
    LookupTable tplan(e, table);
    const std::vector<Scalar> mult = lookup_count(tplan, column, n);
    if (!(mult == ints({1, 1, 2, 0}))) return 10;
    std::vector<int> zd;
    const std::vector<Scalar> terms = logup_terms(e, column, table, mult, Scalar::from_u64(beta), n, 1, &zd);
    std::vector<Scalar> tot;
    const std::vector<Scalar> acc = fr_scan(e, terms, n, KZG_SCAN_SUM, true, &tot);
    if (zd[0] != 0 || !acc[0].is_zero() || acc[1].is_zero() || !tot[0].is_zero()) return 11;
    // the second term alone, and a wrong multiplicity
    std::vector<Scalar> wrong = mult;
    wrong[3] = one;
    const std::vector<Scalar> side = logup_terms(e, {}, table, wrong, Scalar::from_u64(beta), n, 0);
    std::vector<Scalar> chk = {side[3]};
    const std::vector<Scalar> d3 = ints({beta + 40});
    e.check(kzg_fr_vec_mul(e.ctx(), chk.data(), d3.data(), 1, KZG_FR_CANONICAL_LE_32, 0));
    const std::vector<Scalar> sum = fr_scan(e, {chk[0], one}, 2, KZG_SCAN_SUM);
    if (!sum[1].is_zero()) return 12;                    // -1 / (beta + 40) * (beta + 40) + 1 = 0
    // a zero denominator: beta = 0 meets the value 0
    const std::vector<Scalar> withzero = ints({5, 0, 7, 9});
    const std::vector<Scalar> z = logup_terms(e, withzero, {}, {}, Scalar(), n, 1, &zd);
    if (zd[0] != 1) return 13;
    for (const Scalar &x : z)
        if (!x.is_zero()) return 14;
    try {
        logup_terms(e, withzero, {}, {}, Scalar(), n, 1);
        return 15;
    } catch (const ReferencePanic &) {
    }
    try {
        logup_terms(e, column, table, {}, Scalar::from_u64(beta), n, 1);  // a table without multiplicities
        return 16;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
