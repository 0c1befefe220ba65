// Exercises msm_g2_bucket and PointTree::verify of include/kzg_mi355x.hpp on the GPU: the bucket sum against kzg_msm_g2 on the same
// inputs, and a batched opening made by KZGProver::create_witness_batched checked at the tree's points.  The exit status names the
// failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;

static std::vector<Scalar> scalars(const std::vector<uint64_t> &v) {
    std::vector<Scalar> s;
    for (uint64_t x : v) s.push_back(Scalar::from_u64(x));
    return s;
}

int main() {
    Engine e(0);
    KZGParams params = setup(e, Scalar::from_u64(0x5eed), 16, 8);
    // the G2 sum both ways, with an offset and without terms
    const std::vector<Scalar> sc = scalars({3, 0, 1, 0xffffffffffffffffull, 7});
    G2Affine want;
    e.check(kzg_msm_g2(e.ctx(), params.hs, 2, sc.data(), sc.size(), KZG_FR_CANONICAL_LE_32, want.bytes.data(), KZG_G2_AFFINE_MONT_192));
    if (!(msm_g2_bucket(e, params.hs, sc, 2) == want)) return 1;
    if (!(msm_g2_bucket(e, params.hs, {}) == G2Affine())) return 2;
    try {
        msm_g2_bucket(e, params.hs, sc, 4);  // 4 + 5 > 8 points
        return 3;
    } catch (const ReferencePanic &) {
    }
    // 3 + 2 X^2 + X^5 opened at 1, 2, 3
    const Polynomial p = Polynomial::make(scalars({3, 0, 2, 0, 0, 1}));
    const std::vector<Scalar> xs = scalars({1, 2, 3}), ys = scalars({6, 43, 264});
    KZGProver prover(params);
    const KZGCommitment c = prover.commit(p);
    const KZGBatchWitness w = prover.create_witness_batched(p, xs, ys);
    PointTree tree(e, xs);
    if (!tree.verify(params, c, w.r, w.w)) return 4;
    if (tree.verify(params, c, w.r, c)) return 5;  // the commitment is no witness
    Polynomial bent = w.r;
    bent.coeffs[0] = Scalar::from_u64(1);
    if (tree.verify(params, c, bent, w.w)) return 6;
    PointTree other(e, scalars({1, 2, 4}));
    if (other.verify(params, c, w.r, w.w)) return 7;
    if (KZGVerifier(params).verify_eval_batched(xs, c, w) != tree.verify(params, c, w.r, w.w)) return 8;
    // the prover on the tree: the bytes of create_witness_batched, accepted by the verifier on the tree; a wrong claim is refused
    Polynomial tr;
    const KZGWitness tw = tree.create_witness(params, p, ys, &tr);
    if (!(tw == w.w)) return 10;
    if (tr.num_coeffs() != w.r.num_coeffs()) return 11;
    for (size_t i = 0; i < tr.num_coeffs(); i++)
        if (!(tr.coeffs[i] == w.r.coeffs[i])) return 12;
    if (!tree.verify(params, c, tr, tw)) return 13;
    if (!(tree.create_witness(params, p, {}, nullptr) == tw)) return 14;  // no claim
    try {
        tree.create_witness(params, p, scalars({6, 43, 265}), nullptr);
        return 15;
    } catch (const KZGError &) {
    }
    PointTree wide(e, scalars({1, 2, 3, 4, 5, 6, 7, 8}));  // 8 + 1 > the 8 points of hs
    try {
        wide.verify(params, c, w.r, w.w);
        return 9;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
