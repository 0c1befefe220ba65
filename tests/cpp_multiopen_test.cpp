// Exercises fr_lincomb, KZGProver::multiopen_commit / multiopen_finish, the same on KZGProverEvalForm, and KZGVerifier::verify_multiopen of
// include/kzg_mi355x.hpp on the GPU: three polynomials, seven claims at three points in both forms, D against the commitment of g,
// honest and tampered verdicts.  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;
int main() {
    Engine e(0);
    const size_t n = 16, n_polys = 3;
    const Scalar tau = Scalar::from_u64(0x1234567);
    KZGParams params = setup(e, tau, n);
    KZGProver prover(params);
    KZGVerifier verifier(params);
    std::vector<Scalar> coeffs(n_polys * n);
    for (size_t k = 0; k < coeffs.size(); k++) coeffs[k] = Scalar::from_u64(1000 + 17 * k * k);
    const std::vector<Scalar> pts = {Scalar::from_u64(11), Scalar::from_u64(0x9E3779B97F4A7C15ull), Scalar::from_u64(5)};
    const std::vector<uint32_t> idx = {0, 1, 2, 0, 1, 2, 1};
    std::vector<Scalar> zs;
    for (size_t k = 0; k < idx.size(); k++) zs.push_back(pts[(k * 2) % 3]);
    const Scalar r = Scalar::from_u64(0x165667B19E3779F9ull), t = Scalar::from_u64(0xC2B2AE3D27D4EB4Full);
    // fr_lincomb: 2 v_0 + 3 v_2
    std::vector<Scalar> lc = fr_lincomb(e, coeffs, n, {0, 2}, {Scalar::from_u64(2), Scalar::from_u64(3)});
    for (size_t j = 0; j < n; j++)
        if (!(lc[j].le == Scalar::from_u64(2 * (1000 + 17 * j * j) + 3 * (1000 + 17 * (2 * n + j) * (2 * n + j))).le)) return 1;
    std::vector<KZGCommitment> cm;
    std::vector<Polynomial> polys;
    for (size_t m = 0; m < n_polys; m++) {
        polys.push_back(Polynomial::make(std::vector<Scalar>(coeffs.begin() + m * n, coeffs.begin() + (m + 1) * n)));
        cm.push_back(prover.commit(polys[m]));
    }
    KZGMultiopenCommit c = prover.multiopen_commit(coeffs, n, idx, zs, r);
    if (c.ys.size() != idx.size() || c.g.size() != n - 1) return 2;
    for (size_t k = 0; k < idx.size(); k++)
        if (!(polys[idx[k]].eval(e, zs[k]).le == c.ys[k].le)) return 3;
    if (!(prover.commit(Polynomial::make(c.g)).bytes == c.d.bytes)) return 4;
    auto fin = prover.multiopen_finish(coeffs, n, idx, zs, r, t, c.g);
    if (!verifier.verify_multiopen(zs, c.ys, cm, idx, r, t, c.d, fin.first)) return 5;
    std::vector<Scalar> bad = c.ys;
    bad[4] = Scalar::from_u64(1);
    if (verifier.verify_multiopen(zs, bad, cm, idx, r, t, c.d, fin.first)) return 6;
    if (verifier.verify_multiopen(zs, c.ys, cm, idx, r, Scalar::from_u64(77), c.d, fin.first)) return 7;
    if (verifier.verify_multiopen(zs, c.ys, cm, idx, r, t, fin.first, c.d)) return 8;
    if (!verifier.verify_multiopen({}, {}, {}, {}, r, t, c.d, fin.first)) return 9;
    try {
        verifier.verify_multiopen(zs, c.ys, cm, idx, r, zs[3], c.d, fin.first);  // t equal to a z_k
        return 10;
    } catch (const ReferencePanic &) {
    }
    try {
        verifier.verify_multiopen(zs, c.ys, cm, {0, 1}, r, t, c.d, fin.first);
        return 11;
    } catch (const ReferencePanic &) {
    }
    // identity indices: one claim per polynomial
    {
        std::vector<Scalar> z3 = {pts[0], pts[0], pts[1]};
        KZGMultiopenCommit c3 = prover.multiopen_commit(coeffs, n, {}, z3, r);
        auto f3 = prover.multiopen_finish(coeffs, n, {}, z3, r, t, c3.g);
        if (!verifier.verify_multiopen(z3, c3.ys, cm, {}, r, t, c3.d, f3.first)) return 12;
    }
    // evaluation form: the same claims on evaluation vectors over the size-n domain
    kzg_srs *lag = nullptr;
    if (kzg_srs_setup_lagrange_g1(e.ctx(), tau.le.data(), KZG_FR_CANONICAL_LE_32, n, &lag) != KZG_OK) return 13;
    {
        KZGProverEvalForm eprover(params, lag);
        std::vector<Scalar> evals(coeffs.size());
        for (size_t k = 0; k < coeffs.size(); k++) evals[k] = Scalar::from_u64(7 + 3 * k);
        std::vector<KZGCommitment> ecm;
        for (size_t m = 0; m < n_polys; m++)
            ecm.push_back(eprover.commit(EvaluationDomain::from_coeffs(std::vector<Scalar>(evals.begin() + m * n, evals.begin() + (m + 1) * n))));
        KZGMultiopenCommit ec = eprover.multiopen_commit(evals, idx, zs, r);
        if (!(eprover.commit(EvaluationDomain::from_coeffs(ec.g)).bytes == ec.d.bytes)) return 14;
        auto ef = eprover.multiopen_finish(evals, idx, zs, r, t, ec.g);
        if (!verifier.verify_multiopen(zs, ec.ys, ecm, idx, r, t, ec.d, ef.first)) return 15;
        ec.ys[0] = Scalar::from_u64(2);
        if (verifier.verify_multiopen(zs, ec.ys, ecm, idx, r, t, ec.d, ef.first)) return 16;
    }
    kzg_srs_free(e.ctx(), lag);
    std::puts("ok");
    return 0;
}
