// Exercises poly_divide and Polynomial::long_division of include/kzg_mi355x.hpp on the GPU.  Dividends are built as q0 b + r0 from small
// integers with a monic divisor, so every coefficient stays far below r and the expected quotient and remainder are q0 and r0 themselves.
// The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> scalars(const std::vector<uint64_t> &v) {
    std::vector<Scalar> s;
    for (uint64_t x : v) s.push_back(Scalar::from_u64(x));
    return s;
}
// q b + r over the integers
static std::vector<uint64_t> combine(const std::vector<uint64_t> &q, const std::vector<uint64_t> &b, const std::vector<uint64_t> &r) {
    std::vector<uint64_t> a(q.size() + b.size() - 1, 0);
    for (size_t i = 0; i < q.size(); i++)
        for (size_t j = 0; j < b.size(); j++) a[i + j] += q[i] * b[j];
    for (size_t i = 0; i < r.size(); i++) a[i] += r[i];
    return a;
}

int main() {
    Engine e(0);
    const std::vector<uint64_t> b = {4, 3, 2, 1}, q0 = {5, 6, 7, 8, 9}, q1 = {0, 11, 0, 0, 13}, r0 = {1, 2, 3}, r1 = {7, 0, 0}, none = {};
    const std::vector<uint64_t> a0 = combine(q0, b, r0), a1 = combine(q1, b, r1), a2 = combine(q0, b, none);
    // three dividends against one divisor
    std::vector<Scalar> a = scalars(a0), more = scalars(a1), exact_one = scalars(a2), q, r;
    a.insert(a.end(), more.begin(), more.end());
    a.insert(a.end(), exact_one.begin(), exact_one.end());
    std::vector<int> exact;
    poly_divide(e, a, a0.size(), 3, scalars(b), q, r, &exact);
    std::vector<Scalar> wq = scalars(q0), wq1 = scalars(q1), wr = scalars(r0), wr1 = scalars(r1);
    wq.insert(wq.end(), wq1.begin(), wq1.end());
    std::vector<Scalar> wq2 = scalars(q0);
    wq.insert(wq.end(), wq2.begin(), wq2.end());
    wr.insert(wr.end(), wr1.begin(), wr1.end());
    wr.insert(wr.end(), 3, Scalar());
    if (!(q == wq)) return 1;
    if (!(r == wr)) return 2;
    if (exact != std::vector<int>({0, 0, 1})) return 3;
    // the mirror: quotient of degree deg a - deg b, remainder with its degree fixed up, None for an exact division
    Polynomial divisor = Polynomial::make(scalars({4, 3, 2, 1, 0}));  // slice_coeffs drops the zero top
    Polynomial::Division d = Polynomial::make(scalars(a1)).long_division(e, divisor);
    if (!(d.quotient.coeffs == scalars(q1)) || d.quotient.degree != 4) return 4;
    if (!d.has_remainder || !(d.remainder.coeffs == scalars(r1)) || d.remainder.degree != 0) return 5;
    d = Polynomial::make(scalars(a2)).long_division(e, divisor);
    if (!(d.quotient.coeffs == scalars(q0)) || d.has_remainder) return 6;
    // the reference's early returns
    Polynomial zero = Polynomial::make(scalars({0, 0}));
    d = zero.long_division(e, divisor);
    if (d.has_remainder || d.quotient.degree != 0 || !d.quotient.coeffs[0].is_zero()) return 7;
    d = Polynomial::make(scalars({9, 8})).long_division(e, divisor);
    if (!d.has_remainder || d.remainder.degree != 1 || !(d.remainder.coeffs == scalars({9, 8})) || !d.quotient.is_zero()) return 8;
    try {
        divisor.long_division(e, zero);
        return 9;
    } catch (const ReferencePanic &) {
    }
    // a dividend shorter than the divisor through the flat call: no quotient, the dividend as remainder
    poly_divide(e, scalars({9, 8}), 2, 1, scalars(b), q, r, &exact);
    if (!q.empty() || !(r == scalars({9, 8, 0})) || exact[0] != 0) return 10;
    try {
        poly_divide(e, scalars({9, 8}), 2, 1, scalars({1, 0}), q, r);  // a zero top coefficient
        return 11;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
