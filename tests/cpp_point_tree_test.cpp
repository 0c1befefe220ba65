// Exercises PointTree and Polynomial::lagrange_interpolation_with_tree of include/kzg_mi355x.hpp on the GPU.  Points and values are
// small integers chosen so that every expected number is a small integer too.  The exit status names the failed step.
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
    const std::vector<Scalar> xs = scalars({1, 2, 3, 4, 5});
    PointTree tree = PointTree::new_from_points(e, xs);
    if (tree.len() != 5 || !tree.distinct() || tree.bytes() == 0) return 1;
    // 3 + 2 X^2 at 1 .. 5, and with a second polynomial, X^9 (ten coefficients: more than the eight points of the padded tree), in one call
    const Polynomial p = Polynomial::make(scalars({3, 0, 2}));
    if (!(tree.eval(p) == scalars({5, 11, 21, 35, 53}))) return 2;
    std::vector<Scalar> two = scalars({3, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1});
    if (!(tree.eval_batch(two, 10, 2) == scalars({5, 11, 21, 35, 53, 1, 512, 19683, 262144, 1953125}))) return 3;
    // the product (X - 1) .. (X - 5): monic of degree 5, 120 at X = 6
    const Polynomial m = tree.product();
    if (m.degree != 5 || m.coeffs.size() != 6 || !(m.coeffs[5] == Scalar::from_u64(1))) return 4;
    if (!(m.eval(e, Scalar::from_u64(6)) == Scalar::from_u64(120))) return 5;
    // sum_i M / (X - x_i) at X = 6: 120 / 5 + 120 / 4 + 120 / 3 + 120 / 2 + 120 / 1
    const Polynomial c = tree.linear_mod_combination(scalars({1, 1, 1, 1, 1}));
    if (c.degree != 4 || !(c.eval(e, Scalar::from_u64(6)) == Scalar::from_u64(274))) return 6;
    // interpolation gives the polynomial back, zero-padded; two value vectors in one call
    if (!(tree.interpolate(scalars({5, 11, 21, 35, 53, 1, 2, 3, 4, 5})) == scalars({3, 0, 2, 0, 0, 0, 1, 0, 0, 0}))) return 7;
    const Polynomial f = Polynomial::lagrange_interpolation_with_tree(e, xs, scalars({5, 11, 21, 35, 53}), tree);
    if (f.degree != 2 || !(f.coeffs == scalars({3, 0, 2, 0, 0}))) return 8;
    if (!(f.coeffs == Polynomial::lagrange_interpolation(e, xs, scalars({5, 11, 21, 35, 53})).coeffs)) return 9;
    // one point: the tree gives the constant, the mirror the reference's X + (y - x)
    PointTree one(e, scalars({7}));
    if (!(one.interpolate(scalars({9})) == scalars({9}))) return 10;
    const Polynomial quirk = Polynomial::lagrange_interpolation_with_tree(e, scalars({7}), scalars({9}), one);
    if (quirk.degree != 1 || !(quirk.coeffs == scalars({2, 1}))) return 11;
    // repeated points: values still right, interpolation refused
    PointTree twice(e, scalars({2, 2, 3}));
    if (twice.distinct() || !(twice.eval(p) == scalars({11, 11, 21}))) return 12;
    try {
        twice.interpolate(scalars({1, 1, 1}));
        return 13;
    } catch (const ReferencePanic &) {
    }
    try {
        PointTree none(e, {});
        return 14;
    } catch (const ReferencePanic &) {
    }
    printf("ok\n");
    return 0;
}
