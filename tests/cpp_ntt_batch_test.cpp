// Exercises ntt_batch and EvaluationDomain::fft_many / ifft_many of include/kzg_mi355x.hpp on the GPU against the per-vector calls of the same
// header (EvaluationDomain::fft / ifft, which the Python suite pins to the oracle).  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> ramp(size_t n, uint64_t seed) {
    std::vector<Scalar> s;
    uint64_t x = seed;
    for (size_t i = 0; i < n; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        s.push_back(Scalar::from_u64(x >> 8));
    }
    return s;
}

int main() {
    Engine e(0);
    // ntt_batch at 2^5 x 3, strided by 40 elements, against three fft calls; the words between the vectors stay
    const size_t n = 32, stride = 40;
    std::vector<Scalar> data = ramp(2 * stride + n, 7), before = data;
    ntt_batch(e, data, 5, 3, stride);
    for (size_t b = 0; b < 3; b++) {
        EvaluationDomain d = EvaluationDomain::from_coeffs(std::vector<Scalar>(before.begin() + b * stride, before.begin() + b * stride + n));
        d.fft(e);
        if (!std::equal(d.coeffs.begin(), d.coeffs.end(), data.begin() + b * stride)) return 1;
        if (b < 2 && !std::equal(before.begin() + b * stride + n, before.begin() + (b + 1) * stride, data.begin() + b * stride + n)) return 2;
    }
    ntt_batch(e, data, 5, 3, stride, true);
    if (!(data == before)) return 3;
    try {
        ntt_batch(e, data, 5, 4, stride);  // a fourth vector does not fit
        return 4;
    } catch (const ReferencePanic &) {
    }
    // fft_many / ifft_many on three domains of 64 against fft per domain
    std::vector<EvaluationDomain> ds, single;
    for (uint64_t b = 0; b < 3; b++) ds.push_back(EvaluationDomain::from_coeffs(ramp(64, 100 + b)));
    single = ds;
    const std::vector<EvaluationDomain> start = ds;
    std::vector<EvaluationDomain *> ptrs = {&ds[0], &ds[1], &ds[2]};
    EvaluationDomain::fft_many(e, ptrs);
    for (size_t b = 0; b < 3; b++) {
        single[b].fft(e);
        if (!(ds[b].coeffs == single[b].coeffs)) return 5;
    }
    EvaluationDomain::ifft_many(e, ptrs);
    for (size_t b = 0; b < 3; b++)
        if (!(ds[b].coeffs == start[b].coeffs)) return 6;
    EvaluationDomain::coset_fft_many(e, ptrs);
    for (size_t b = 0; b < 3; b++) {
        single[b] = start[b];
        single[b].coset_fft(e);
        if (!(ds[b].coeffs == single[b].coeffs)) return 7;
    }
    EvaluationDomain::icoset_fft_many(e, ptrs);
    for (size_t b = 0; b < 3; b++)
        if (!(ds[b].coeffs == start[b].coeffs)) return 8;
    EvaluationDomain other = EvaluationDomain::from_coeffs(ramp(32, 5));
    try {
        EvaluationDomain::fft_many(e, {&ds[0], &other});
        return 9;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
