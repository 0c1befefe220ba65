// Exercises fr_fold, KZGProver::open_fold_batch, KZGProverEvalForm::open_fold_batch and KZGVerifier::verify_fold of
// include/kzg_mi355x.hpp on the GPU: two groups of three polynomials in both forms, the fold of their values against fr_fold, the
// folded witness against create_witness of the folded polynomial, honest and tampered verdicts.  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;
int main() {
    Engine e(0);
    const size_t n = 16, t = 3, groups = 2;
    const Scalar tau = Scalar::from_u64(0x1234567);
    KZGParams params = setup(e, tau, n);
    KZGProver prover(params);
    KZGVerifier verifier(params);
    std::vector<Scalar> coeffs(groups * t * n);
    for (size_t k = 0; k < coeffs.size(); k++) coeffs[k] = Scalar::from_u64(1000 + 17 * k * k);
    std::vector<Scalar> zs = {Scalar::from_u64(11), Scalar::from_u64(0x9E3779B97F4A7C15ull)};
    std::vector<Scalar> gammas = {Scalar::from_u64(3), Scalar::from_u64(0xC2B2AE3D27D4EB4Full)};
    const Scalar r = Scalar::from_u64(0x165667B19E3779F9ull);
    auto opened = prover.open_fold_batch(coeffs, n, t, zs, gammas);
    if (opened.first.size() != groups * t || opened.second.size() != groups) return 1;
    // the values are Polynomial::eval's, the witness is create_witness of the folded polynomial at (z, folded value)
    std::vector<Scalar> folded = fr_fold(e, coeffs, n, t, gammas), folded_y = fr_fold(e, opened.first, 1, t, gammas);
    std::vector<KZGCommitment> cm;
    for (size_t g = 0; g < groups; g++) {
        for (size_t i = 0; i < t; i++) {
            Polynomial p = Polynomial::make(std::vector<Scalar>(coeffs.begin() + (g * t + i) * n, coeffs.begin() + (g * t + i + 1) * n));
            if (!(p.eval(e, zs[g]).le == opened.first[g * t + i].le)) return 2;
            cm.push_back(prover.commit(p));
        }
        Polynomial F = Polynomial::make(std::vector<Scalar>(folded.begin() + g * n, folded.begin() + (g + 1) * n));
        if (!(F.eval(e, zs[g]).le == folded_y[g].le)) return 3;
        if (!(prover.create_witness(F, zs[g], folded_y[g]).bytes == opened.second[g].bytes)) return 4;
        if (!verifier.verify_eval(zs[g], folded_y[g], prover.commit(F), opened.second[g])) return 5;
    }
    if (!verifier.verify_fold(zs, opened.first, cm, {}, opened.second, t, gammas, r)) return 6;
    std::vector<uint32_t> idx = {0, 1, 2, 3, 4, 5};
    if (!verifier.verify_fold(zs, opened.first, cm, idx, opened.second, t, gammas, r)) return 7;
    if (!verifier.verify_fold({}, {}, {}, {}, {}, t, {}, r)) return 8;
    std::vector<Scalar> bad = opened.first;
    bad[4] = Scalar::from_u64(1);
    if (verifier.verify_fold(zs, bad, cm, {}, opened.second, t, gammas, r)) return 9;
    std::vector<Scalar> other = gammas;
    other[1] = Scalar::from_u64(5);
    if (verifier.verify_fold(zs, opened.first, cm, idx, opened.second, t, other, r)) return 10;
    try {
        verifier.verify_fold(zs, opened.first, cm, {}, opened.second, t, {gammas[0], Scalar::from_u64(0)}, r);
        return 11;
    } catch (const ReferencePanic &) {
    }
    try {
        verifier.verify_fold(zs, opened.first, cm, {0, 1}, opened.second, t, gammas, r);
        return 12;
    } catch (const ReferencePanic &) {
    }
    // evaluation form: the same two groups as evaluation vectors over the size-n domain
    kzg_srs *lag = nullptr;
    if (kzg_srs_setup_lagrange_g1(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, n, &lag) != KZG_OK) return 13;
    {
        KZGProverEvalForm eprover(params, lag);
        std::vector<Scalar> evals(coeffs.size());
        for (size_t k = 0; k < coeffs.size(); k++) evals[k] = Scalar::from_u64(7 + 3 * k);
        auto eo = eprover.open_fold_batch(evals, t, zs, gammas);
        std::vector<Scalar> ef = fr_fold(e, evals, n, t, gammas);
        std::vector<KZGCommitment> ecm;
        for (size_t g = 0; g < groups; g++) {
            EvaluationDomain F = EvaluationDomain::from_coeffs(std::vector<Scalar>(ef.begin() + g * n, ef.begin() + (g + 1) * n));
            auto one = eprover.open_at(F, zs[g]);
            if (!(one.second.bytes == eo.second[g].bytes)) return 14;
            for (size_t i = 0; i < t; i++)
                ecm.push_back(eprover.commit(
                    EvaluationDomain::from_coeffs(std::vector<Scalar>(evals.begin() + (g * t + i) * n, evals.begin() + (g * t + i + 1) * n))));
        }
        if (!verifier.verify_fold(zs, eo.first, ecm, {}, eo.second, t, gammas, r)) return 15;
        eo.first[0] = Scalar::from_u64(2);
        if (verifier.verify_fold(zs, eo.first, ecm, {}, eo.second, t, gammas, r)) return 16;
    }
    kzg_srs_free(e.ctx(), lag);
    std::puts("ok");
    return 0;
}
