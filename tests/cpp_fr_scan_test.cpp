// Exercises batch_inverse, fr_scan and grand_product of include/kzg_mi355x.hpp on the GPU: scans of small integers against 64-bit host
// arithmetic, the inverses and the accumulator through identities checked with kzg_fr_vec_mul (the Python suite pins the bytes to the
// integer model).  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> mul(const Engine &e, std::vector<Scalar> a, const std::vector<Scalar> &b) {
    e.check(kzg_fr_vec_mul(e.ctx(), a.data(), b.data(), a.size(), KZG_FR_CANONICAL_LE_32, 0));
    return a;
}

int main() {
    Engine e(0);
    const Scalar one = Scalar::from_u64(1);
    // two vectors of 20 small integers: 20! < 2^64
    const size_t n = 20;
    std::vector<Scalar> v;
    for (uint64_t b = 0; b < 2; b++)
        for (uint64_t i = 0; i < n; i++) v.push_back(Scalar::from_u64(b ? n - i : i + 1));
    std::vector<Scalar> tot;
    std::vector<Scalar> p = fr_scan(e, v, n, KZG_SCAN_PRODUCT, false, &tot);
    std::vector<Scalar> px = fr_scan(e, v, n, KZG_SCAN_PRODUCT, true);
    std::vector<Scalar> s = fr_scan(e, v, n, KZG_SCAN_SUM);
    std::vector<Scalar> sx = fr_scan(e, v, n, KZG_SCAN_SUM, true);
    for (uint64_t b = 0; b < 2; b++) {
        uint64_t prod = 1, sum = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (!(px[b * n + i] == Scalar::from_u64(prod))) return 1;
            if (!(sx[b * n + i] == Scalar::from_u64(sum))) return 2;
            const uint64_t x = b ? n - i : i + 1;
            prod *= x;
            sum += x;
            if (!(p[b * n + i] == Scalar::from_u64(prod))) return 3;
            if (!(s[b * n + i] == Scalar::from_u64(sum))) return 4;
        }
        if (!(tot[b] == Scalar::from_u64(prod))) return 5;
    }
    try {
        fr_scan(e, v, 7);  // 40 scalars are no whole number of vectors of 7
        return 6;
    } catch (const ReferencePanic &) {
    }
    // v * (1 / v) = 1, and a zero maps to zero and is counted
    std::vector<Scalar> w = v;
    w[3] = Scalar();
    size_t zeros = 99;
    std::vector<Scalar> iv = batch_inverse(e, w, &zeros);
    if (zeros != 1 || !iv[3].is_zero()) return 7;
    std::vector<Scalar> id = mul(e, w, iv);
    for (size_t i = 0; i < id.size(); i++)
        if (!(id[i] == (i == 3 ? Scalar() : one))) return 8;
    // the accumulator of a permutation: den is num rotated, so the total is 1, and z[i + 1] den[i] = z[i] num[i] (t = 1)
    std::vector<Scalar> num(v.begin(), v.begin() + n), den(n);
    for (size_t i = 0; i < n; i++) den[i] = num[(i + 7) % n];
    std::vector<int> zd;
    std::vector<Scalar> z = grand_product(e, num, den, n, 1, &tot, &zd);
    if (!(z[0] == one) || !(tot[0] == one) || zd[0] != 0) return 9;
    std::vector<Scalar> zn = mul(e, z, num), zs(z.begin() + 1, z.end());
    zs.push_back(tot[0]);
    if (!(mul(e, zs, den) == zn)) return 10;
    // a zero denominator: flagged, or a ReferencePanic without the flags
    den[5] = Scalar();
    z = grand_product(e, num, den, n, 1, &tot, &zd);
    if (zd[0] != 1 || !tot[0].is_zero()) return 11;
    for (const Scalar &x : z)
        if (!x.is_zero()) return 12;
    try {
        grand_product(e, num, den, n, 1);
        return 13;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
