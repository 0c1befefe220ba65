// Exercises KZGVerifier::verify_eval_batch of include/kzg_mi355x.hpp on the GPU: honest openings of two polynomials with and without
// commitment indices, one tampered value, and a challenge the call rejects.  The exit status names the failed step.
#include <cstdio>
#include "../include/kzg_mi355x.hpp"
using namespace kzg;
int main() {
    Engine e(0);
    KZGParams params = setup(e, Scalar::from_u64(0x1234567), 13);
    KZGProver prover(params);
    KZGVerifier verifier(params);
    std::vector<Scalar> c1(13), c2(13);
    for (int i = 0; i < 7; i++) c1[i] = Scalar::from_u64(1000 + 17 * i);
    for (int i = 0; i < 3; i++) c2[i] = Scalar::from_u64(5 + i);
    Polynomial p1 = Polynomial::make(c1), p2 = Polynomial::make(c2);
    std::vector<KZGCommitment> cm = {prover.commit(p1), prover.commit(p2)};
    std::vector<uint32_t> idx = {0, 1, 0, 0, 1};
    std::vector<Scalar> xs, ys;
    std::vector<KZGWitness> ws;
    std::vector<KZGCommitment> each;
    for (size_t k = 0; k < idx.size(); k++) {
        const Polynomial &p = idx[k] ? p2 : p1;
        xs.push_back(Scalar::from_u64(11 + (k == 3 ? 0 : k)));  // opening 3 repeats the point of opening 0
        ys.push_back(p.eval(e, xs[k]));
        ws.push_back(prover.create_witness(p, xs[k], ys[k]));
        each.push_back(cm[idx[k]]);
    }
    const Scalar r = Scalar::from_u64(0x9E3779B97F4A7C15ull);
    if (!verifier.verify_eval_batch(xs, ys, cm, idx, ws, r)) return 1;
    if (!verifier.verify_eval_batch(xs, ys, each, {}, ws, r)) return 2;  // one commitment per opening
    if (!verifier.verify_eval_batch({}, {}, {}, {}, {}, r)) return 3;
    std::vector<Scalar> bad = ys;
    bad[2] = Scalar::from_u64(1);
    if (verifier.verify_eval_batch(xs, bad, cm, idx, ws, r)) return 4;
    if (verifier.verify_eval_batch(xs, bad, each, {}, ws, r)) return 5;
    if (verifier.verify_eval(xs[2], bad[2], cm[0], ws[2])) return 6;
    try {
        verifier.verify_eval_batch(xs, ys, cm, idx, ws, Scalar::from_u64(0));
        return 7;
    } catch (const ReferencePanic &) {
    }
    try {
        verifier.verify_eval_batch(xs, ys, cm, {0, 1, 0}, ws, r);
        return 8;
    } catch (const ReferencePanic &) {
    }
    std::puts("ok");
    return 0;
}
