// Exercises ntt_g1 and ntt_g2 of include/kzg_mi355x.hpp on the GPU under a known secret: the inverse DFT of the monomial powers is the
// Lagrange basis (kzg_srs_setup_lagrange_g1 / _g2), the forward DFT goes back, a batch of two arrays equals two calls, and a shape
// that is no whole number of arrays throws (the Python suite pins the bytes to the integer model).  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

template <class Pt, class Srs, class Dl>
static std::vector<Pt> download(const Engine &e, const Srs *s, size_t n, Dl dl, int fmt) {
    std::vector<Pt> v(n);
    e.check(dl(e.ctx(), s, 0, n, v.data(), fmt));
    return v;
}

int main() {
    Engine e(0);
    const Scalar tau = Scalar::from_u64(0x5EED0F71A5ull);
    const uint32_t log_n = 4;
    const size_t d = (size_t)1 << log_n;
    {
        kzg_srs *mono = nullptr, *lag = nullptr;
        e.check(kzg_srs_setup_g1(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, d, &mono));
        e.check(kzg_srs_setup_lagrange_g1(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, d, &lag));
        const std::vector<G1Affine> gs = download<G1Affine>(e, mono, d, kzg_srs_download_g1, KZG_G1_AFFINE_MONT_96);
        const std::vector<G1Affine> ls = download<G1Affine>(e, lag, d, kzg_srs_download_g1, KZG_G1_AFFINE_MONT_96);
        kzg_srs_free(e.ctx(), mono);
        kzg_srs_free(e.ctx(), lag);
        if (!(ntt_g1(e, gs, log_n, true) == ls)) return 1;
        if (!(ntt_g1(e, ls, log_n) == gs)) return 2;
        std::vector<G1Affine> two(gs);
        two.insert(two.end(), ls.begin(), ls.end());
        std::vector<G1Affine> a = ntt_g1(e, gs, log_n), b = ntt_g1(e, ls, log_n);
        a.insert(a.end(), b.begin(), b.end());
        if (!(ntt_g1(e, two, log_n) == a)) return 3;
        if (!(ntt_g1(e, gs, 0) == gs)) return 4;  // d arrays of one point: a copy
        try {
            ntt_g1(e, gs, 5);  // 16 points are no whole number of arrays of 32
            return 5;
        } catch (const ReferencePanic &) {
        }
    }
    {
        kzg_srs_g2 *mono = nullptr, *lag = nullptr;
        e.check(kzg_srs_setup_g2(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, d, &mono));
        e.check(kzg_srs_setup_lagrange_g2(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, d, &lag));
        const std::vector<G2Affine> hs = download<G2Affine>(e, mono, d, kzg_srs_download_g2, KZG_G2_AFFINE_MONT_192);
        const std::vector<G2Affine> ls = download<G2Affine>(e, lag, d, kzg_srs_download_g2, KZG_G2_AFFINE_MONT_192);
        kzg_srs_g2_free(e.ctx(), mono);
        kzg_srs_g2_free(e.ctx(), lag);
        if (!(ntt_g2(e, hs, log_n, true) == ls)) return 6;
        if (!(ntt_g2(e, ls, log_n) == hs)) return 7;
        std::vector<G2Affine> two(hs);
        two.insert(two.end(), ls.begin(), ls.end());
        std::vector<G2Affine> a = ntt_g2(e, hs, log_n), b = ntt_g2(e, ls, log_n);
        a.insert(a.end(), b.begin(), b.end());
        if (!(ntt_g2(e, two, log_n) == a)) return 8;
        if (!ntt_g2(e, {}, log_n).empty()) return 9;
        try {
            ntt_g2(e, hs, 5);
            return 10;
        } catch (const ReferencePanic &) {
        }
    }
    printf("ok\n");
    return 0;
}
