// kzg_mi355x.hpp -- header-only C++ host mirror of the reference's prover surface over the C ABI
// (include/kzg_mi355x.h).  Same names, argument meaning and error behaviour as proxima-one/kzg:
//   setup / KZGParams            src/lib.rs:14-55           Polynomial          src/polynomial.rs:24-165
//   EvaluationDomain             src/ft.rs:17-140           KZGProver           src/coeff_form.rs:37-112
//   KZGProverEvalForm            src/eval_form.rs:39-147    KZGVerifier         src/coeff_form.rs:114-183
// Result<_, KZGError> becomes a thrown kzg::KZGError; a reference panic becomes kzg::ReferencePanic.
// Scalars are 32-byte canonical little-endian (kzg::Scalar), points 96-byte affine Montgomery (kzg::G1Affine).
#pragma once
#include <array>
#include <cstring>
#include <stdexcept>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "kzg_mi355x.h"

namespace kzg {

struct Scalar {
    std::array<uint8_t, 32> le{};  // canonical, < r
    static Scalar from_u64(uint64_t v) {
        Scalar s;
        for (int i = 0; i < 8; i++) s.le[i] = (uint8_t)(v >> (8 * i));
        return s;
    }
    bool operator==(const Scalar &o) const { return le == o.le; }
    bool is_zero() const {
        for (auto b : le) if (b) return false;
        return true;
    }
};
struct G1Affine {
    std::array<uint8_t, 96> bytes{};  // blst_p1_affine; identity = all zero
    bool operator==(const G1Affine &o) const { return bytes == o.bytes; }
};
using KZGCommitment = G1Affine;  // src/lib.rs:22
using KZGWitness = G1Affine;     // src/lib.rs:24

struct KZGError : std::runtime_error {  // src/lib.rs:26-36
    enum Kind { PointNotOnPolynomial = 1, PolynomialDegreeTooLarge = 2 } kind;
    KZGError(Kind k, const std::string &m) : std::runtime_error(m), kind(k) {}
};
struct ReferencePanic : std::runtime_error { using std::runtime_error::runtime_error; };
struct EngineError : std::runtime_error { using std::runtime_error::runtime_error; };

class Engine {
  public:
    explicit Engine(int device = 0) {
        if (int rc = kzg_ctx_create(device, &ctx_)) throw EngineError("kzg_ctx_create failed (no CPU fallback): " + std::to_string(rc));
    }
    ~Engine() { kzg_ctx_destroy(ctx_); }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    kzg_ctx *ctx() const { return ctx_; }
    // the batched pipeline's plan and whether the process' hardware-queue pool narrowed it (kzg_ctx_info)
    std::string info() const {
        char buf[512];
        check(kzg_ctx_info(ctx_, buf, sizeof buf));
        return buf;
    }
    void check(int rc) const {
        if (rc == KZG_OK) return;
        std::string msg = kzg_last_error(ctx_);
        if (rc == KZG_ERR_POINT_NOT_ON_POLY) throw KZGError(KZGError::PointNotOnPolynomial, "point not on polynomial!");
        if (rc == KZG_ERR_DEGREE_TOO_LARGE) throw KZGError(KZGError::PolynomialDegreeTooLarge, "polynomial degree too large");
        if (rc == KZG_ERR_SHAPE) throw ReferencePanic(msg);
        throw EngineError("kzg_mi355x error " + std::to_string(rc) + ": " + msg);
    }

  private:
    kzg_ctx *ctx_ = nullptr;
};

// KZGParams: `gs` (G1 powers) and `hs` (G2 powers, read by the verifier only) live on the GPU.
struct KZGParams {
    const Engine *engine = nullptr;
    kzg_srs *gs = nullptr;
    kzg_srs_g2 *hs = nullptr;
    size_t len() const { return kzg_srs_len(gs); }
    KZGParams() = default;
    KZGParams(const KZGParams &) = delete;
    KZGParams &operator=(const KZGParams &) = delete;
    KZGParams(KZGParams &&o) noexcept : engine(o.engine), gs(o.gs), hs(o.hs) { o.gs = nullptr; o.hs = nullptr; }
    ~KZGParams() {
        if (gs) kzg_srs_free(engine->ctx(), gs);
        if (hs) kzg_srs_g2_free(engine->ctx(), hs);
    }
};

// src/lib.rs:38-55.  The reference builds num_coeffs G2 powers too; only the verifier reads them (hs[0], hs[1] and
// hs[..k+1] for a k-point batched opening), so `g2_len` caps that half (SIZE_MAX = min(num_coeffs, 257)).
inline KZGParams setup(const Engine &e, const Scalar &s, size_t num_coeffs, size_t g2_len = (size_t)-1) {
    KZGParams p;
    p.engine = &e;
    e.check(kzg_srs_setup_g1(e.ctx(), s.le.data(), KZG_FR_CANONICAL_LE_32, num_coeffs, &p.gs));
    if (g2_len == (size_t)-1) g2_len = num_coeffs < 257 ? num_coeffs : 257;
    if (g2_len) e.check(kzg_srs_setup_g2(e.ctx(), s.le.data(), KZG_FR_CANONICAL_LE_32, g2_len, &p.hs));
    return p;
}

// sum scalars[i] * hs[offset + i] by the bucket method (kzg_msm_g2_bucket): the affine Montgomery bytes kzg_msm_g2 gives
struct G2Affine {
    std::array<uint8_t, 192> bytes{};  // blst_p2_affine; identity = all zero
    bool operator==(const G2Affine &o) const { return bytes == o.bytes; }
};
inline G2Affine msm_g2_bucket(const Engine &e, const kzg_srs_g2 *hs, const std::vector<Scalar> &scalars, size_t offset = 0) {
    if (!hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
    G2Affine out;
    Scalar none;
    e.check(kzg_msm_g2_bucket(e.ctx(), hs, offset, scalars.empty() ? &none : scalars.data(), scalars.size(), KZG_FR_CANONICAL_LE_32, 0,
                              out.bytes.data(), KZG_G2_AFFINE_MONT_192));
    return out;
}

// kzg_ntt_g1 / kzg_ntt_g2: the DFT over the group of points.size() / 2^log_n arrays of 2^log_n affine points back to back, over
// compute_omega(2^log_n): out[m] = sum_j [w^(jm)] P[j], or with `inverse` out[j] = [1/d] sum_m [w^(-jm)] P[m] (the two undo each
// other).  Natural order in and out.  Not a reference method.
inline std::vector<G1Affine> ntt_g1(const Engine &e, const std::vector<G1Affine> &points, uint32_t log_n, bool inverse = false) {
    static_assert(sizeof(G1Affine) == 96, "G1Affine is the 96-byte affine Montgomery encoding");
    const size_t d = (size_t)1 << log_n;
    if (log_n > 22 || points.size() % d != 0) throw ReferencePanic("ntt_g1: shape");
    std::vector<G1Affine> out(points.size());
    if (points.empty()) return out;
    e.check(kzg_ntt_g1(e.ctx(), points.data(), log_n, points.size() / d, inverse ? 1 : 0, KZG_G1_AFFINE_MONT_96, 0, out.data(), KZG_G1_AFFINE_MONT_96));
    return out;
}
inline std::vector<G2Affine> ntt_g2(const Engine &e, const std::vector<G2Affine> &points, uint32_t log_n, bool inverse = false) {
    static_assert(sizeof(G2Affine) == 192, "G2Affine is the 192-byte affine Montgomery encoding");
    const size_t d = (size_t)1 << log_n;
    if (log_n > 20 || points.size() % d != 0) throw ReferencePanic("ntt_g2: shape");
    std::vector<G2Affine> out(points.size());
    if (points.empty()) return out;
    e.check(kzg_ntt_g2(e.ctx(), points.data(), log_n, points.size() / d, inverse ? 1 : 0, KZG_G2_AFFINE_MONT_192, 0, out.data(), KZG_G2_AFFINE_MONT_192));
    return out;
}

class PointTree;
struct Polynomial {  // src/polynomial.rs:24-27
    size_t degree = 0;
    std::vector<Scalar> coeffs;
    static size_t compute_degree(const std::vector<Scalar> &c, size_t upper) {  // :94-105
        size_t i = upper;
        while (i > 0 && c[i].is_zero()) i--;
        return i;
    }
    static Polynomial make(std::vector<Scalar> c) {  // Polynomial::new, :83-87
        Polynomial p;
        p.degree = compute_degree(c, c.size() - 1);
        p.coeffs = std::move(c);
        return p;
    }
    static Polynomial new_from_coeffs(std::vector<Scalar> c, size_t degree) {  // :89-92
        Polynomial p;
        p.degree = degree;
        p.coeffs = std::move(c);
        return p;
    }
    size_t num_coeffs() const { return degree + 1; }  // :135-137
    Scalar eval(const Engine &e, const Scalar &x) const {  // :156-165
        Scalar y;
        e.check(kzg_poly_eval(e.ctx(), coeffs.data(), num_coeffs(), x.le.data(), KZG_FR_CANONICAL_LE_32, 0, y.le.data()));
        return y;
    }
    // :229-233 (the reference asserts xs.len() > degree; its values are p(xs[i]) either way)
    std::vector<Scalar> multi_eval(const Engine &e, const std::vector<Scalar> &xs) const;
    // :266-293; one point: X + (y - x), as the reference returns it
    static Polynomial lagrange_interpolation(const Engine &e, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys);
    // :237-264 on a PointTree built from xs (below); one point: X + (y - x), as the reference returns it
    static Polynomial lagrange_interpolation_with_tree(const Engine &e, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys, const PointTree &tree);
    bool is_zero() const { return degree == 0 && coeffs[0].is_zero(); }  // :45-47
    // :193-227: (quotient, Option<remainder>); the remainder is valid iff has_remainder (the reference's Some)
    struct Division;
    Division long_division(const Engine &e, const Polynomial &divisor) const;
};
struct Polynomial::Division {
    Polynomial quotient;
    bool has_remainder = false;
    Polynomial remainder;
};

// kzg_poly_multi_eval: ys[b k + i] = p_b(xs[i]) for `batch` polynomials of n coefficients each (coeffs: batch x n scalars back to
// back) at the k = xs.size() points
inline std::vector<Scalar> poly_multi_eval(const Engine &e, const std::vector<Scalar> &coeffs, size_t n, size_t batch, const std::vector<Scalar> &xs) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (n == 0 || coeffs.size() / n != batch || coeffs.size() != batch * n) throw ReferencePanic("poly_multi_eval: shape");
    std::vector<Scalar> ys(batch * xs.size());
    Scalar none;
    e.check(kzg_poly_multi_eval(e.ctx(), coeffs.data(), n, batch, xs.empty() ? &none : xs.data(), xs.size(), KZG_FR_CANONICAL_LE_32, 0,
                                ys.empty() ? &none : ys.data()));
    return ys;
}

// kzg_interpolate: out[b k + j] = coefficient j of the polynomial of degree < k through (xs[i], ys[b k + i]), k = xs.size(); one point
// gives the constant
inline std::vector<Scalar> interpolate(const Engine &e, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys) {
    const size_t k = xs.size();
    if (k == 0 || ys.size() % k) throw ReferencePanic("interpolate: shape");
    std::vector<Scalar> out(ys.size());
    Scalar none;
    e.check(kzg_interpolate(e.ctx(), xs.data(), ys.empty() ? &none : ys.data(), k, ys.size() / k, KZG_FR_CANONICAL_LE_32, 0, ys.empty() ? &none : out.data()));
    return out;
}

// kzg_poly_divide: `batch` dividends of na coefficients each (a: batch x na scalars back to back) by the one divisor b (b.back() != 0):
// q receives batch x (na - nb + 1) and r batch x (nb - 1) scalars, zero-padded; exact[bi] = 1 iff remainder bi is zero.  na < nb: q is
// empty and r holds the dividends.
inline void poly_divide(const Engine &e, const std::vector<Scalar> &a, size_t na, size_t batch, const std::vector<Scalar> &b, std::vector<Scalar> &q,
                        std::vector<Scalar> &r, std::vector<int> *exact = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    const size_t nb = b.size();
    if (na == 0 || nb == 0 || a.size() / na != batch || a.size() != batch * na) throw ReferencePanic("poly_divide: shape");
    q.assign(na >= nb ? batch * (na - nb + 1) : 0, Scalar());
    r.assign(batch * (nb - 1), Scalar());
    if (exact) exact->assign(batch, 0);
    Scalar none;
    e.check(kzg_poly_divide(e.ctx(), a.data(), na, batch, b.data(), nb, KZG_FR_CANONICAL_LE_32, 0, q.empty() ? &none : q.data(),
                            r.empty() ? &none : r.data(), exact && batch ? exact->data() : nullptr));
}

inline Polynomial::Division Polynomial::long_division(const Engine &e, const Polynomial &divisor) const {
    Division d;
    d.quotient = Polynomial::make({Scalar()});  // new_zero
    if (is_zero()) return d;
    if (divisor.is_zero()) throw ReferencePanic("divisor must not be zero!");
    if (degree < divisor.degree) {
        d.has_remainder = true;
        d.remainder = *this;
        return d;
    }
    std::vector<Scalar> a(coeffs.begin(), coeffs.begin() + num_coeffs()), b(divisor.coeffs.begin(), divisor.coeffs.begin() + divisor.num_coeffs());
    std::vector<Scalar> q, r;
    std::vector<int> exact;
    poly_divide(e, a, a.size(), 1, b, q, r, &exact);
    d.quotient = Polynomial::new_from_coeffs(std::move(q), degree - divisor.degree);
    if (!exact[0]) {
        d.has_remainder = true;
        d.remainder = Polynomial::make(std::move(r));  // the degree fixed up, as shrink_degree leaves it
    }
    return d;
}

inline std::vector<Scalar> Polynomial::multi_eval(const Engine &e, const std::vector<Scalar> &xs) const {
    if (xs.size() <= degree) throw ReferencePanic("assert!(xs.len() > self.degree())");
    std::vector<Scalar> c(coeffs.begin(), coeffs.begin() + num_coeffs());
    return poly_multi_eval(e, c, num_coeffs(), 1, xs);
}

inline Polynomial Polynomial::lagrange_interpolation(const Engine &e, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys) {
    if (xs.size() != ys.size()) throw ReferencePanic("assert_eq!(xs.len(), ys.len())");
    std::vector<Scalar> c = interpolate(e, xs, ys);
    if (xs.size() != 1) return Polynomial::make(std::move(c));
    Scalar d = ys[0];  // X + (y - x): the subtraction is the engine's, on one element
    e.check(kzg_fr_vec_sub(e.ctx(), d.le.data(), xs[0].le.data(), 1, KZG_FR_CANONICAL_LE_32, 0));
    return Polynomial::new_from_coeffs({d, Scalar::from_u64(1)}, 1);
}

// SubProductTree (src/polynomial.rs:303-365) as a device-resident plan (kzg_point_tree): built once from a point set, kept by the
// caller, every method O(k log^2 k).  The engine must outlive the tree.
class PointTree {
  public:
    PointTree(const Engine &e, const std::vector<Scalar> &xs) : e_(&e), k_(xs.size()) {  // new_from_points, :310-327
        static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
        Scalar none;
        e.check(kzg_point_tree_setup(e.ctx(), xs.empty() ? &none : xs.data(), xs.size(), KZG_FR_CANONICAL_LE_32, &h_));
    }
    static PointTree new_from_points(const Engine &e, const std::vector<Scalar> &xs) { return PointTree(e, xs); }
    ~PointTree() {
        if (h_) kzg_point_tree_free(e_->ctx(), h_);
    }
    PointTree(const PointTree &) = delete;
    PointTree &operator=(const PointTree &) = delete;
    PointTree(PointTree &&o) noexcept : e_(o.e_), h_(o.h_), k_(o.k_) { o.h_ = nullptr; }
    const kzg_point_tree *handle() const { return h_; }
    size_t len() const { return k_; }
    size_t bytes() const {
        size_t b = 0;
        kzg_point_tree_shape(h_, nullptr, nullptr, &b, nullptr);
        return b;
    }
    bool distinct() const {
        int d = 0;
        kzg_point_tree_shape(h_, nullptr, nullptr, nullptr, &d);
        return d != 0;
    }
    Polynomial product() const {  // tree.product: prod (X - x_i)
        std::vector<Scalar> c(k_ + 1);
        e_->check(kzg_point_tree_product(e_->ctx(), h_, KZG_FR_CANONICAL_LE_32, 0, c.data()));
        return Polynomial::new_from_coeffs(std::move(c), k_);
    }
    // ys[b k + i] = p_b(xs[i]) for `batch` polynomials of n coefficients each (coeffs: batch x n scalars back to back)
    std::vector<Scalar> eval_batch(const std::vector<Scalar> &coeffs, size_t n, size_t batch) const {
        if (n == 0 || coeffs.size() / n != batch || coeffs.size() != batch * n) throw ReferencePanic("PointTree::eval_batch: shape");
        std::vector<Scalar> ys(batch * k_);
        Scalar none;
        e_->check(kzg_point_tree_eval(e_->ctx(), h_, coeffs.data(), n, batch, KZG_FR_CANONICAL_LE_32, 0, ys.empty() ? &none : ys.data()));
        return ys;
    }
    std::vector<Scalar> eval(const Polynomial &f) const {  // :329-348, without its panic on a zero remainder
        std::vector<Scalar> c(f.coeffs.begin(), f.coeffs.begin() + f.num_coeffs());
        return eval_batch(c, c.size(), 1);
    }
    Polynomial linear_mod_combination(const std::vector<Scalar> &cs) const {  // :350-364
        if (cs.size() != k_) throw ReferencePanic("PointTree::linear_mod_combination: one scalar per point");
        std::vector<Scalar> out(k_);
        e_->check(kzg_point_tree_combine(e_->ctx(), h_, cs.data(), 1, KZG_FR_CANONICAL_LE_32, 0, out.data()));
        return Polynomial::make(std::move(out));
    }
    // out[b k + j] = coefficient j of the polynomial of degree < k through (xs[i], ys[b k + i]); one point gives the constant
    std::vector<Scalar> interpolate(const std::vector<Scalar> &ys) const {
        if (ys.size() % k_) throw ReferencePanic("PointTree::interpolate: shape");
        std::vector<Scalar> out(ys.size());
        Scalar none;
        e_->check(kzg_point_tree_interpolate(e_->ctx(), h_, ys.empty() ? &none : ys.data(), ys.size() / k_, KZG_FR_CANONICAL_LE_32, 0,
                                             ys.empty() ? &none : out.data()));
        return out;
    }
    // create_witness_batched (src/coeff_form.rs:83-111) at the tree's points, any number of them (kzg_witness_coeff_tree): returns w =
    // [p / M]_1 and, through r, p mod M -- the two halves of a KZGBatchWitness.  ys: the claimed values (KZGError if one is wrong), or
    // empty for no claim.  One point gives r as the constant; the reference's X + (y - x) is the caller's to form.
    KZGWitness create_witness(const KZGParams &params, const Polynomial &p, const std::vector<Scalar> &ys, Polynomial *r) const {
        if (!ys.empty() && ys.size() != k_) throw ReferencePanic("assert_eq!(xs.len(), ys.len())");
        G1Affine w;
        std::vector<Scalar> rc(k_);
        e_->check(kzg_witness_coeff_tree(e_->ctx(), params.gs, h_, p.coeffs.data(), p.num_coeffs(), 1, ys.empty() ? nullptr : ys.data(),
                                         KZG_FR_CANONICAL_LE_32, 0, w.bytes.data(), KZG_G1_AFFINE_MONT_96, rc.data(), nullptr));
        if (r) *r = Polynomial::make(std::move(rc));
        return w;
    }
    // verify_eval_batched (src/coeff_form.rs:144-182) at the tree's points, any number of them (kzg_verify_eval_tree): r and w are
    // the two halves of a KZGBatchWitness
    bool verify(const KZGParams &params, const KZGCommitment &c, const Polynomial &r, const KZGWitness &w) const {
        if (!params.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        if (r.num_coeffs() > k_) throw ReferencePanic("PointTree::verify: witness.r has more coefficients than the tree has points");
        std::vector<Scalar> rc(r.coeffs.begin(), r.coeffs.begin() + r.num_coeffs());
        rc.resize(k_);
        uint8_t ok = 0;
        e_->check(kzg_verify_eval_tree(e_->ctx(), params.gs, params.hs, h_, rc.data(), KZG_FR_CANONICAL_LE_32, c.bytes.data(), w.bytes.data(),
                                       KZG_G1_AFFINE_MONT_96, 1, &ok));
        return ok != 0;
    }

  private:
    const Engine *e_;
    kzg_point_tree *h_ = nullptr;
    size_t k_;
};

inline Polynomial Polynomial::lagrange_interpolation_with_tree(const Engine &e, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys,
                                                               const PointTree &tree) {
    if (xs.size() != ys.size()) throw ReferencePanic("assert_eq!(xs.len(), ys.len())");
    if (tree.len() != xs.size()) throw ReferencePanic("lagrange_interpolation_with_tree: the tree was built from another point set");
    if (xs.size() != 1) return Polynomial::make(tree.interpolate(ys));
    Scalar d = ys[0];  // X + (y - x): the subtraction is the engine's, on one element
    e.check(kzg_fr_vec_sub(e.ctx(), d.le.data(), xs[0].le.data(), 1, KZG_FR_CANONICAL_LE_32, 0));
    return Polynomial::new_from_coeffs({d, Scalar::from_u64(1)}, 1);
}

struct EvaluationDomain {  // src/ft.rs:17-25
    std::vector<Scalar> coeffs;
    size_t d = 0;
    uint32_t exp = 0;
    Scalar omega;
    static EvaluationDomain from_coeffs(std::vector<Scalar> c) {  // :94-109
        EvaluationDomain e;
        int rc = kzg_compute_omega(c.size(), &e.d, &e.exp, e.omega.le.data(), KZG_FR_CANONICAL_LE_32);
        if (rc == KZG_ERR_DEGREE_TOO_LARGE) throw KZGError(KZGError::PolynomialDegreeTooLarge, "polynomial degree too large");
        c.resize(e.d);
        e.coeffs = std::move(c);
        return e;
    }
    size_t len() const { return coeffs.size(); }
    void fft(const Engine &e) { e.check(kzg_ntt_fr(e.ctx(), coeffs.data(), exp, 0, 0)); }   // :111-113
    void ifft(const Engine &e) { e.check(kzg_ntt_fr(e.ctx(), coeffs.data(), exp, 1, 0)); }  // :115-140
    void coset_fft(const Engine &e) { e.check(kzg_coset_ntt_fr(e.ctx(), coeffs.data(), exp, 0, KZG_FR_CANONICAL_LE_32, 0)); }
    void icoset_fft(const Engine &e) { e.check(kzg_coset_ntt_fr(e.ctx(), coeffs.data(), exp, 1, KZG_FR_CANONICAL_LE_32, 0)); }
    // the same four for many domains of ONE size in one kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch call (not reference methods)
    static void fft_many(const Engine &e, const std::vector<EvaluationDomain *> &ds) { many(e, ds, false, 0); }
    static void ifft_many(const Engine &e, const std::vector<EvaluationDomain *> &ds) { many(e, ds, false, 1); }
    static void coset_fft_many(const Engine &e, const std::vector<EvaluationDomain *> &ds) { many(e, ds, true, 0); }
    static void icoset_fft_many(const Engine &e, const std::vector<EvaluationDomain *> &ds) { many(e, ds, true, 1); }
    Scalar z(const Scalar &tau) const {  // :182-187
        Scalar out;
        if (kzg_domain_z(coeffs.size(), tau.le.data(), KZG_FR_CANONICAL_LE_32, out.le.data())) throw ReferencePanic("z");
        return out;
    }
    void divide_by_z_on_coset(const Engine &e) { e.check(kzg_divide_by_z_on_coset(e.ctx(), coeffs.data(), exp, KZG_FR_CANONICAL_LE_32, 0)); }
    void mul_assign(const Engine &e, const EvaluationDomain &o) {  // :220-244
        if (o.coeffs.size() != coeffs.size()) throw ReferencePanic("assert_eq!(self.coeffs.len(), other.coeffs.len())");
        e.check(kzg_fr_vec_mul(e.ctx(), coeffs.data(), o.coeffs.data(), coeffs.size(), KZG_FR_CANONICAL_LE_32, 0));
    }
    void sub_assign(const Engine &e, const EvaluationDomain &o) {  // :247-271
        if (o.coeffs.size() != coeffs.size()) throw ReferencePanic("assert_eq!(self.coeffs.len(), other.coeffs.len())");
        e.check(kzg_fr_vec_sub(e.ctx(), coeffs.data(), o.coeffs.data(), coeffs.size(), KZG_FR_CANONICAL_LE_32, 0));
    }

  private:
    static void many(const Engine &e, const std::vector<EvaluationDomain *> &ds, bool coset, int inverse);
};

// kzg_ntt_fr_batch / kzg_coset_ntt_fr_batch on host vectors: data holds `batch` vectors of 2^log_n scalars, vector b at element
// b * stride (stride 0: back to back); transformed in place.  Not reference methods.
inline void ntt_batch(const Engine &e, std::vector<Scalar> &data, uint32_t log_n, size_t batch, size_t stride = 0, bool inverse = false) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    const size_t n = (size_t)1 << log_n;
    if (log_n < 32 && batch && data.size() < (batch - 1) * (stride ? stride : n) + n) throw ReferencePanic("ntt_batch: shape");
    e.check(kzg_ntt_fr_batch(e.ctx(), data.data(), log_n, batch, stride, inverse ? 1 : 0, 0));
}
inline void coset_ntt_batch(const Engine &e, std::vector<Scalar> &data, uint32_t log_n, size_t batch, size_t stride = 0, bool inverse = false) {
    const size_t n = (size_t)1 << log_n;
    if (log_n < 32 && batch && data.size() < (batch - 1) * (stride ? stride : n) + n) throw ReferencePanic("coset_ntt_batch: shape");
    e.check(kzg_coset_ntt_fr_batch(e.ctx(), data.data(), log_n, batch, stride, inverse ? 1 : 0, KZG_FR_CANONICAL_LE_32, 0));
}

inline void EvaluationDomain::many(const Engine &e, const std::vector<EvaluationDomain *> &ds, bool coset, int inverse) {
    if (ds.empty()) return;
    for (const EvaluationDomain *d : ds)
        if (d->exp != ds[0]->exp || d->coeffs.size() != ds[0]->coeffs.size()) throw ReferencePanic("the domains of one batched transform must have one size");
    const size_t n = ds[0]->coeffs.size();
    std::vector<Scalar> all;
    all.reserve(n * ds.size());
    for (const EvaluationDomain *d : ds) all.insert(all.end(), d->coeffs.begin(), d->coeffs.end());
    if (coset) coset_ntt_batch(e, all, ds[0]->exp, ds.size(), 0, inverse != 0);
    else ntt_batch(e, all, ds[0]->exp, ds.size(), 0, inverse != 0);
    for (size_t b = 0; b < ds.size(); b++) std::copy(all.begin() + b * n, all.begin() + (b + 1) * n, ds[b]->coeffs.begin());
}

// kzg_recover_cosets: the polynomial of at most n coefficients whose values on the cosets `coset_ids` (coset i = { w^(i + tK) },
// K = N / l, cells[j] = the l values on coset_ids[j]) are `cells`; evals (optional) receives its N evaluations.  Not a reference method.
inline Polynomial recover_cosets(const Engine &e, uint32_t log_n, uint32_t log_l, size_t n, const std::vector<size_t> &coset_ids,
                                 const std::vector<Scalar> &cells, std::vector<Scalar> *evals = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (log_l > log_n || log_n > 22 || cells.size() != (coset_ids.size() << log_l)) throw ReferencePanic("recover_cosets: shape");
    std::vector<Scalar> c(n ? n : 1);
    if (evals) evals->resize((size_t)1 << log_n);
    e.check(kzg_recover_cosets(e.ctx(), log_n, log_l, n, coset_ids.data(), coset_ids.size(), cells.data(), 1, KZG_FR_CANONICAL_LE_32, 0,
                               c.data(), evals ? evals->data() : nullptr, nullptr));
    return Polynomial::make(std::move(c));
}

// kzg_eval_form_eval: p_b(zs[b]) for zs.size() polynomials given by their evaluations over the size-d domain (evals: zs.size() x d
// scalars back to back), at any points of Fr.  Not a reference method.
inline std::vector<Scalar> eval_form_eval(const Engine &e, const std::vector<Scalar> &evals, size_t d, const std::vector<Scalar> &zs) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (evals.size() != zs.size() * d) throw ReferencePanic("eval_form_eval: shape");
    std::vector<Scalar> ys(zs.size());
    e.check(kzg_eval_form_eval(e.ctx(), evals.data(), d, zs.size(), zs.data(), KZG_FR_CANONICAL_LE_32, 0, ys.data()));
    return ys;
}

// kzg_fr_fold: out[g d + j] = sum_{i < t} gammas[g]^i vecs[(g t + i) d + j] for gammas.size() groups of t vectors of d scalars (vecs:
// groups x t x d scalars back to back).  Not a reference method.
inline std::vector<Scalar> fr_fold(const Engine &e, const std::vector<Scalar> &vecs, size_t d, size_t t, const std::vector<Scalar> &gammas) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (d == 0 || t == 0 || vecs.size() / d / t != gammas.size() || vecs.size() != gammas.size() * t * d) throw ReferencePanic("fr_fold: shape");
    std::vector<Scalar> out(gammas.size() * d);
    e.check(kzg_fr_fold(e.ctx(), vecs.data(), d, t, gammas.size(), gammas.data(), KZG_FR_CANONICAL_LE_32, 0, out.data()));
    return out;
}

// kzg_fr_lincomb: out[j] = sum_k weights[k] vecs[idx[k] d + j], j < d (vecs: n_vecs x d scalars back to back).  Not a reference method.
inline std::vector<Scalar> fr_lincomb(const Engine &e, const std::vector<Scalar> &vecs, size_t d, const std::vector<uint32_t> &idx,
                                      const std::vector<Scalar> &weights) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (d == 0 || vecs.size() % d != 0 || idx.size() != weights.size()) throw ReferencePanic("fr_lincomb: shape");
    std::vector<Scalar> out(d);
    e.check(kzg_fr_lincomb(e.ctx(), vecs.data(), d, vecs.size() / d, idx.data(), weights.data(), idx.size(), KZG_FR_CANONICAL_LE_32, 0, out.data()));
    return out;
}

// kzg_fr_batch_inverse: 1 / v for every v; a zero maps to zero, *zeros (optional) counts them.  Not a reference method.
inline std::vector<Scalar> batch_inverse(const Engine &e, const std::vector<Scalar> &values, size_t *zeros = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (values.empty()) throw ReferencePanic("batch_inverse: no values");
    std::vector<Scalar> out(values.size());
    e.check(kzg_fr_batch_inverse(e.ctx(), values.data(), values.size(), KZG_FR_CANONICAL_LE_32, 0, out.data(), zeros));
    return out;
}

// kzg_fr_scan: the running products (op = KZG_SCAN_PRODUCT) or sums (KZG_SCAN_SUM) of vecs.size() / n vectors of n scalars back to back;
// exclusive: a vector's scan starts from the identity and leaves its last element out.  totals (optional): every vector's total.  Not a
// reference method.
inline std::vector<Scalar> fr_scan(const Engine &e, const std::vector<Scalar> &vecs, size_t n, int op = KZG_SCAN_PRODUCT, bool exclusive = false,
                                   std::vector<Scalar> *totals = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (n == 0 || vecs.size() % n != 0) throw ReferencePanic("fr_scan: shape");
    const size_t batch = vecs.size() / n;
    std::vector<Scalar> out(vecs.size());
    if (totals) totals->resize(batch);
    e.check(kzg_fr_scan(e.ctx(), vecs.data(), n, batch, op, exclusive ? 1 : 0, KZG_FR_CANONICAL_LE_32, 0, out.data(), totals ? totals->data() : nullptr));
    return out;
}

// kzg_fr_grand_product: z[b n] = 1, z[b n + i] = prod_{k < i} prod_j num[b][j][k] / den[b][j][k] for num.size() / (t n) vectors of t columns of n
// scalars (column j of vector b at element (b t + j) n).  totals (optional): every vector's full product.  zero_den (optional): the vectors
// with a zero denominator are flagged there and have zero rows and totals; without it such a vector throws ReferencePanic.  Not a
// reference method.
inline std::vector<Scalar> grand_product(const Engine &e, const std::vector<Scalar> &num, const std::vector<Scalar> &den, size_t n, size_t t,
                                         std::vector<Scalar> *totals = nullptr, std::vector<int> *zero_den = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (n == 0 || t == 0 || num.size() != den.size() || num.size() % n != 0 || (num.size() / n) % t != 0) throw ReferencePanic("grand_product: shape");
    const size_t batch = num.size() / n / t;
    std::vector<Scalar> z(batch * n);
    if (totals) totals->resize(batch);
    if (zero_den) zero_den->resize(batch);
    e.check(kzg_fr_grand_product(e.ctx(), num.data(), den.data(), n, t, batch, KZG_FR_CANONICAL_LE_32, 0, z.data(), totals ? totals->data() : nullptr,
                                 zero_den ? zero_den->data() : nullptr));
    return z;
}

// A table of scalars prepared for membership queries (kzg_lookup): built once, kept by the caller, queried by any number of threads.  The
// table may hold duplicates; a value's owner is the lowest row that holds it.  The engine must outlive the table.  Not a reference type.
class LookupTable {
  public:
    LookupTable(const Engine &e, const std::vector<Scalar> &table) : e_(&e) {
        static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
        Scalar none;
        e.check(kzg_lookup_setup(e.ctx(), table.empty() ? &none : table.data(), table.size(), KZG_FR_CANONICAL_LE_32, 0, &h_));
    }
    ~LookupTable() {
        if (h_) kzg_lookup_free(e_->ctx(), h_);
    }
    LookupTable(const LookupTable &) = delete;
    LookupTable &operator=(const LookupTable &) = delete;
    LookupTable(LookupTable &&o) noexcept : e_(o.e_), h_(o.h_) { o.h_ = nullptr; }
    const kzg_lookup *handle() const { return h_; }
    const Engine &engine() const { return *e_; }
    size_t len() const { return shape(0); }
    size_t distinct() const { return shape(1); }
    size_t bytes() const { return shape(2); }

  private:
    size_t shape(int which) const {
        size_t v[3] = {0, 0, 0};
        kzg_lookup_shape(h_, &v[0], &v[1], &v[2]);
        return v[which];
    }
    const Engine *e_;
    kzg_lookup *h_ = nullptr;
};

// kzg_lookup_count: values is values.size() / n vectors of n scalars back to back.  Returns the multiplicities, plan.len() per vector (the
// number of values each row owns).  indices (optional): every value's owner row, 0xFFFFFFFF for a value that is not in the table.  missing,
// first_missing (optional): per vector how many values are not in the table and the position of the first (SIZE_MAX if none); without
// either a missing value throws ReferencePanic.  Not a reference method.
inline std::vector<Scalar> lookup_count(const LookupTable &plan, const std::vector<Scalar> &values, size_t n, std::vector<uint32_t> *indices = nullptr,
                                        std::vector<size_t> *missing = nullptr, std::vector<size_t> *first_missing = nullptr) {
    if (n == 0 || values.size() % n != 0) throw ReferencePanic("lookup_count: shape");
    const size_t batch = values.size() / n;
    std::vector<Scalar> mult(batch * plan.len());
    if (indices) indices->resize(values.size());
    if (missing) missing->resize(batch);
    if (first_missing) first_missing->resize(batch);
    const Engine &e = plan.engine();
    e.check(kzg_lookup_count(e.ctx(), plan.handle(), values.data(), n, batch, KZG_FR_CANONICAL_LE_32, 0, mult.data(), indices ? indices->data() : nullptr,
                             missing ? missing->data() : nullptr, first_missing ? first_missing->data() : nullptr));
    return mult;
}

// kzg_logup_terms: out[b n + i] = sum_{j < t} 1 / (beta + values[b][j][i]) - mult[b][i] / (beta + table[i]) for vectors of t columns of n
// scalars (column j of vector b at element (b t + j) n); table (n scalars) and mult (batch x n) may both be empty: only the sum; t may be 0
// when they are given.  zero_den (optional): the vectors with a zero denominator are flagged there and have zero rows; without it such a
// vector throws ReferencePanic.  fr_scan(e, out, n, KZG_SCAN_SUM, true) is then the logUp accumulator.  Not a reference method.
inline std::vector<Scalar> logup_terms(const Engine &e, const std::vector<Scalar> &values, const std::vector<Scalar> &table, const std::vector<Scalar> &mult,
                                       const Scalar &beta, size_t n, size_t t, std::vector<int> *zero_den = nullptr) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    const bool side = !table.empty() || !mult.empty();
    if (n == 0 || (t == 0 && !side) || (side && (table.size() != n || mult.size() % n != 0)) || values.size() % n != 0 || (t && (values.size() / n) % t != 0) ||
        (!t && !values.empty()))
        throw ReferencePanic("logup_terms: shape");
    const size_t batch = t ? values.size() / n / t : mult.size() / n;
    if (side && mult.size() != batch * n) throw ReferencePanic("logup_terms: one multiplicity per vector and row");
    std::vector<Scalar> out(batch * n);
    if (zero_den) zero_den->resize(batch);
    e.check(kzg_logup_terms(e.ctx(), t ? values.data() : nullptr, side ? table.data() : nullptr, side ? mult.data() : nullptr, beta.le.data(), n, t, batch,
                            KZG_FR_CANONICAL_LE_32, 0, out.data(), zero_den ? zero_den->data() : nullptr));
    return out;
}

// A straight-line program over Fr (kzg_fr_program), validated once and kept: the constraint expressions of a quotient round, run for
// every row of a set of columns in one pass (fr_program_run).  words: KZG_FRP_WORDS per instruction (instruction() builds them).  The
// engine must outlive the program.  Not a reference type.
class FrProgram {
  public:
    FrProgram(const Engine &e, const std::vector<uint32_t> &words, size_t n_cols, size_t n_consts, size_t n_out) : e_(&e) {
        if (words.size() % KZG_FRP_WORDS) throw ReferencePanic("FrProgram: whole instructions of six words");
        const uint32_t none = 0;
        e.check(kzg_fr_program_setup(e.ctx(), words.empty() ? &none : words.data(), words.size() / KZG_FRP_WORDS, n_cols, n_consts, n_out, &h_));
    }
    ~FrProgram() {
        if (h_) kzg_fr_program_free(e_->ctx(), h_);
    }
    FrProgram(const FrProgram &) = delete;
    FrProgram &operator=(const FrProgram &) = delete;
    FrProgram(FrProgram &&o) noexcept : e_(o.e_), h_(o.h_) { o.h_ = nullptr; }
    static std::array<uint32_t, KZG_FRP_WORDS> instruction(int op, int dst_kind, uint32_t dst, int a_kind, uint32_t a, int b_kind, uint32_t b,
                                                           int32_t a_shift = 0, int32_t b_shift = 0) {
        return {(uint32_t)op | (uint32_t)dst_kind << 8 | (uint32_t)a_kind << 16 | (uint32_t)b_kind << 24, dst, a, b, (uint32_t)a_shift, (uint32_t)b_shift};
    }
    const kzg_fr_program *handle() const { return h_; }
    const Engine &engine() const { return *e_; }
    size_t instructions() const { return shape(0); }
    size_t columns() const { return shape(1); }
    size_t consts() const { return shape(2); }
    size_t outputs() const { return shape(3); }
    size_t temps() const { return shape(4); }
    size_t multiplications() const { return shape(5); }
    // kzg_fr_program_degree: per output an upper bound of its total degree in the columns (a sumcheck needs degree + 1 points)
    std::vector<size_t> degrees() const {
        std::vector<size_t> d(outputs());
        e_->check(kzg_fr_program_degree(h_, d.data()));
        return d;
    }

  private:
    size_t shape(int which) const {
        size_t v[6] = {0, 0, 0, 0, 0, 0};
        kzg_fr_program_shape(h_, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
        return v[which];
    }
    const Engine *e_;
    kzg_fr_program *h_ = nullptr;
};

// kzg_fr_program_run on host vectors: one vector per column -- n elements, or a power of two that divides n (a periodic column) --,
// one scalar per const; returns one vector of n scalars per output.  Not a reference method.
inline std::vector<std::vector<Scalar>> fr_program_run(const FrProgram &plan, const std::vector<std::vector<Scalar>> &cols, const std::vector<Scalar> &consts,
                                                       size_t n) {
    static_assert(sizeof(Scalar) == 32, "Scalar is the 32-byte canonical encoding");
    if (cols.size() != plan.columns() || consts.size() != plan.consts()) throw ReferencePanic("fr_program_run: the plan's columns and consts");
    std::vector<const void *> cp;
    std::vector<size_t> cl;
    for (const std::vector<Scalar> &c : cols) {
        cp.push_back(c.data());
        cl.push_back(c.size());
    }
    std::vector<std::vector<Scalar>> outs(plan.outputs(), std::vector<Scalar>(n));
    std::vector<void *> op;
    for (std::vector<Scalar> &o : outs) op.push_back(o.data());
    const Engine &e = plan.engine();
    e.check(kzg_fr_program_run(e.ctx(), plan.handle(), cp.data(), cl.data(), consts.data(), n, KZG_FR_CANONICAL_LE_32, 0, op.data()));
    return outs;
}

// Sumcheck rounds over multilinear tables on host vectors (kzg_mle_eq / _bind / _eval, kzg_sumcheck_round; the conventions are the C
// header's: f[i] at the corner whose coordinate x_j is bit j of i, rounds bind the top variable).  Not reference methods.
inline std::vector<Scalar> mle_eq(const Engine &e, const std::vector<Scalar> &point) {
    std::vector<Scalar> out((size_t)1 << point.size());
    e.check(kzg_mle_eq(e.ctx(), point.data(), point.size(), KZG_FR_CANONICAL_LE_32, 0, out.data()));
    return out;
}

// every column (n scalars each) folded with rho: lo + rho (hi - lo), n / 2 scalars each
inline std::vector<std::vector<Scalar>> mle_bind(const Engine &e, const std::vector<std::vector<Scalar>> &cols, const Scalar &rho) {
    const size_t n = cols.empty() ? 0 : cols[0].size();
    std::vector<const void *> cp;
    for (const std::vector<Scalar> &c : cols) {
        if (c.size() != n) throw ReferencePanic("mle_bind: columns of one length");
        cp.push_back(c.data());
    }
    std::vector<std::vector<Scalar>> outs(cols.size(), std::vector<Scalar>(n / 2));
    std::vector<void *> op;
    for (std::vector<Scalar> &o : outs) op.push_back(o.data());
    e.check(kzg_mle_bind(e.ctx(), cp.data(), cols.size(), n, rho.le.data(), KZG_FR_CANONICAL_LE_32, 0, op.data()));
    return outs;
}

// f_b(point) for the tables.size() / 2^m tables of 2^m scalars; quotients (optional): per table the n - 1 Zeromorph quotient values
inline std::vector<Scalar> mle_eval(const Engine &e, const std::vector<Scalar> &tables, const std::vector<Scalar> &point,
                                    std::vector<Scalar> *quotients = nullptr) {
    const size_t n = (size_t)1 << point.size();
    if (tables.size() % n) throw ReferencePanic("mle_eval: whole tables of 2^m scalars");
    const size_t batch = tables.size() / n;
    std::vector<Scalar> ys(batch);
    if (quotients) quotients->resize(batch * (n - 1));
    e.check(kzg_mle_eval(e.ctx(), tables.data(), point.size(), batch, point.data(), KZG_FR_CANONICAL_LE_32, 0, ys.data(),
                         quotients && !quotients->empty() ? quotients->data() : nullptr));
    return ys;
}

// sums[o * n_eval + X]: output o of the plan at X over the pairs (i, i + n / 2) of the columns, summed
inline std::vector<Scalar> sumcheck_round(const FrProgram &plan, const std::vector<std::vector<Scalar>> &cols, const std::vector<Scalar> &consts,
                                          size_t n_eval) {
    if (cols.size() != plan.columns() || consts.size() != plan.consts() || cols.empty()) throw ReferencePanic("sumcheck_round: the plan's columns and consts");
    std::vector<const void *> cp;
    for (const std::vector<Scalar> &c : cols) {
        if (c.size() != cols[0].size()) throw ReferencePanic("sumcheck_round: columns of one length");
        cp.push_back(c.data());
    }
    std::vector<Scalar> sums(plan.outputs() * n_eval);
    const Engine &e = plan.engine();
    e.check(kzg_sumcheck_round(e.ctx(), plan.handle(), cp.data(), consts.data(), cols[0].size(), n_eval, KZG_FR_CANONICAL_LE_32, 0, sums.data()));
    return sums;
}

struct KZGBatchWitness {  // src/coeff_form.rs:12-35
    Polynomial r;
    G1Affine w;
    const G1Affine &elem() const { return w; }
    const Polynomial &polynomial() const { return r; }
};

// The first phase of the two-element multiproof (kzg_multiopen_*_commit): the claimed values, the quotient polynomial g the caller
// carries to the second phase, and its commitment D.  The second phase returns (pi, v(t)).  Not reference methods.
struct KZGMultiopenCommit {
    std::vector<Scalar> ys, g;
    KZGCommitment d;
};

class KZGProver {  // src/coeff_form.rs:37-112
  public:
    explicit KZGProver(const KZGParams &params) : params_(params), e_(*params.engine) {}
    const KZGParams &parameters() const { return params_; }
    KZGCommitment commit(const Polynomial &p) const {  // :59-64
        G1Affine out;
        e_.check(kzg_commit_coeff(e_.ctx(), params_.gs, p.coeffs.data(), p.num_coeffs(), KZG_FR_CANONICAL_LE_32, 0,
                                  out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }
    KZGWitness create_witness(const Polynomial &p, const Scalar &x, const Scalar &y) const {  // :66-81
        G1Affine out;
        e_.check(kzg_witness_coeff(e_.ctx(), params_.gs, p.coeffs.data(), p.num_coeffs(), x.le.data(), y.le.data(),
                                   KZG_FR_CANONICAL_LE_32, 0, out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }
    // Not a reference method: `xs.size()` calls of create_witness on one polynomial, pipelined on the GPU.  ok[j] == false
    // where the reference would return Err(PointNotOnPolynomial) for opening j.
    std::vector<KZGWitness> create_witness_many(const Polynomial &p, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys,
                                                std::vector<bool> *ok = nullptr) const {
        if (xs.size() != ys.size()) throw ReferencePanic("assert_eq!(xs.len(), ys.len())");
        std::vector<KZGWitness> out(xs.size());
        std::vector<int> status(xs.size() ? xs.size() : 1, 0);
        static_assert(sizeof(KZGWitness) == 96, "KZGWitness is the 96-byte affine encoding");
        e_.check(kzg_witness_coeff_many(e_.ctx(), params_.gs, p.coeffs.data(), p.num_coeffs(), xs.data(), ys.data(), xs.size(),
                                        KZG_FR_CANONICAL_LE_32, 0, out.data(), KZG_G1_AFFINE_MONT_96, status.data()));
        if (ok) {
            ok->assign(xs.size(), true);
            for (size_t j = 0; j < xs.size(); j++) (*ok)[j] = status[j] == 0;
        }
        return out;
    }
    // kzg_open_fold_coeff: zs.size() groups of t polynomials of n coefficients each (coeffs: groups x t x n scalars back to back, padded
    // by the caller), group g opened at zs[g]: the groups x t values and ONE witness per group, the witness of sum_i gammas[g]^i p_{g,i}.
    // KZGVerifier::verify_fold checks it.  Not a reference method.
    std::pair<std::vector<Scalar>, std::vector<KZGWitness>> open_fold_batch(const std::vector<Scalar> &coeffs, size_t n, size_t t,
                                                                              const std::vector<Scalar> &zs, const std::vector<Scalar> &gammas) const {
        static_assert(sizeof(Scalar) == 32 && sizeof(G1Affine) == 96, "packed encodings");
        if (n == 0 || t == 0 || gammas.size() != zs.size() || coeffs.size() / n / t != zs.size() || coeffs.size() != zs.size() * t * n)
            throw ReferencePanic("open_fold_batch: groups x t polynomials of n coefficients, one point and one challenge per group");
        std::pair<std::vector<Scalar>, std::vector<KZGWitness>> r{std::vector<Scalar>(zs.size() * t), std::vector<KZGWitness>(zs.size())};
        e_.check(kzg_open_fold_coeff(e_.ctx(), params_.gs, coeffs.data(), n, t, zs.size(), zs.data(), gammas.data(), KZG_FR_CANONICAL_LE_32, 0,
                                     r.first.data(), r.second.data(), KZG_G1_AFFINE_MONT_96));
        return r;
    }
    // kzg_multiopen_coeff_commit / _finish: claim k is polynomial poly_idx[k] (empty poly_idx: k) of the coeffs.size() / n polynomials of n
    // coefficients (back to back, padded by the caller) at zs[k].  t MUST be drawn after D exists (a hash that includes D): see the header.
    KZGMultiopenCommit multiopen_commit(const std::vector<Scalar> &coeffs, size_t n, const std::vector<uint32_t> &poly_idx, const std::vector<Scalar> &zs,
                                        const Scalar &r) const {
        static_assert(sizeof(Scalar) == 32 && sizeof(G1Affine) == 96, "packed encodings");
        if (n == 0 || coeffs.size() % n != 0 || (!poly_idx.empty() && poly_idx.size() != zs.size())) throw ReferencePanic("multiopen_commit: shape");
        KZGMultiopenCommit c{std::vector<Scalar>(zs.size()), std::vector<Scalar>(n - 1), KZGCommitment{}};
        std::vector<Scalar> g(n);  // (never an empty buffer)
        e_.check(kzg_multiopen_coeff_commit(e_.ctx(), params_.gs, coeffs.data(), n, coeffs.size() / n, poly_idx.empty() ? nullptr : poly_idx.data(),
                                            zs.data(), zs.size(), r.le.data(), KZG_FR_CANONICAL_LE_32, 0, c.ys.data(), g.data(), &c.d, KZG_G1_AFFINE_MONT_96));
        std::copy(g.begin(), g.begin() + (n - 1), c.g.begin());
        return c;
    }
    std::pair<KZGWitness, Scalar> multiopen_finish(const std::vector<Scalar> &coeffs, size_t n, const std::vector<uint32_t> &poly_idx,
                                                   const std::vector<Scalar> &zs, const Scalar &r, const Scalar &t, const std::vector<Scalar> &g) const {
        if (n == 0 || coeffs.size() % n != 0 || g.size() != n - 1 || (!poly_idx.empty() && poly_idx.size() != zs.size()))
            throw ReferencePanic("multiopen_finish: shape");
        std::pair<KZGWitness, Scalar> out;
        std::vector<Scalar> gp(g);
        gp.resize(n);
        e_.check(kzg_multiopen_coeff_finish(e_.ctx(), params_.gs, coeffs.data(), n, coeffs.size() / n, poly_idx.empty() ? nullptr : poly_idx.data(),
                                            zs.data(), zs.size(), r.le.data(), t.le.data(), gp.data(), KZG_FR_CANONICAL_LE_32, 0, &out.second, &out.first,
                                            KZG_G1_AFFINE_MONT_96));
        return out;
    }
    KZGBatchWitness create_witness_batched(const Polynomial &p, const std::vector<Scalar> &xs,
                                           const std::vector<Scalar> &ys) const {  // :83-111
        if (xs.size() != ys.size()) throw ReferencePanic("assert_eq!(xs.len(), ys.len())");
        KZGBatchWitness wit;
        std::vector<Scalar> r(xs.size() < 2 ? 2 : xs.size());
        size_t rlen = 0;
        e_.check(kzg_witness_coeff_batched(e_.ctx(), params_.gs, p.coeffs.data(), p.num_coeffs(), xs.data(), ys.data(),
                                           xs.size(), KZG_FR_CANONICAL_LE_32, 0, wit.w.bytes.data(), KZG_G1_AFFINE_MONT_96,
                                           r.data(), &rlen));
        r.resize(rlen);
        wit.r = Polynomial::new_from_coeffs(std::move(r), rlen - 1);
        return wit;
    }
    bool verify_poly(const KZGCommitment &c, const Polynomial &p) const {  // KZGVerifier::verify_poly, :119-124
        int ok = 0;
        e_.check(kzg_verify_poly_coeff(e_.ctx(), params_.gs, c.bytes.data(), KZG_G1_AFFINE_MONT_96, p.coeffs.data(),
                                       p.num_coeffs(), KZG_FR_CANONICAL_LE_32, 0, &ok));
        return ok != 0;
    }

  private:
    const KZGParams &params_;
    const Engine &e_;
};

class KZGVerifier {  // src/coeff_form.rs:114-183; the pairing checks run on the GPU
  public:
    explicit KZGVerifier(const KZGParams &params) : params_(params), e_(*params.engine) {}
    bool verify_poly(const KZGCommitment &c, const Polynomial &p) const {  // :119-124
        int ok = 0;
        e_.check(kzg_verify_poly_coeff(e_.ctx(), params_.gs, c.bytes.data(), KZG_G1_AFFINE_MONT_96, p.coeffs.data(),
                                       p.num_coeffs(), KZG_FR_CANONICAL_LE_32, 0, &ok));
        return ok != 0;
    }
    bool verify_eval(const Scalar &x, const Scalar &y, const KZGCommitment &c, const KZGWitness &w) const {  // :126-142
        if (!params_.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        uint8_t ok = 0;
        e_.check(kzg_verify_eval(e_.ctx(), params_.gs, params_.hs, x.le.data(), y.le.data(), KZG_FR_CANONICAL_LE_32,
                                 c.bytes.data(), w.bytes.data(), KZG_G1_AFFINE_MONT_96, 1, &ok));
        return ok != 0;
    }
    // kzg_verify_eval_batch: true iff ALL the openings verify, from one pairing check of their combination with the weights r^k.
    // Opening k claims p(xs[k]) = ys[k] for commitments[commitment_idx[k]]; an empty commitment_idx means one commitment per opening.
    // r must be unpredictable to whoever produced the openings (drawn after they arrived, or the hash of all inputs): see the header.
    // false says nothing about which opening is bad: verify_eval() does.
    bool verify_eval_batch(const std::vector<Scalar> &xs, const std::vector<Scalar> &ys, const std::vector<KZGCommitment> &commitments,
                           const std::vector<uint32_t> &commitment_idx, const std::vector<KZGWitness> &witnesses, const Scalar &r) const {
        if (!params_.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        const size_t count = xs.size();
        if (ys.size() != count || witnesses.size() != count || (!commitment_idx.empty() && commitment_idx.size() != count))
            throw ReferencePanic("verify_eval_batch: shape");
        std::vector<uint8_t> cb(commitments.size() * 96), wb(count * 96);
        for (size_t i = 0; i < commitments.size(); i++) std::memcpy(cb.data() + 96 * i, commitments[i].bytes.data(), 96);
        for (size_t i = 0; i < count; i++) std::memcpy(wb.data() + 96 * i, witnesses[i].bytes.data(), 96);
        int ok = 0;
        e_.check(kzg_verify_eval_batch(e_.ctx(), params_.gs, params_.hs, xs.data(), ys.data(), KZG_FR_CANONICAL_LE_32, cb.data(),
                                       commitments.size(), commitment_idx.empty() ? nullptr : commitment_idx.data(), wb.data(),
                                       KZG_G1_AFFINE_MONT_96, count, r.le.data(), &ok));
        return ok != 0;
    }
    // kzg_verify_fold: true iff ALL zs.size() folded openings verify, from one pairing check.  Group g claims the t values
    // ys[g t .. g t + t) at zs[g] for commitments[commitment_idx[g t + i]] (empty commitment_idx: commitments[g t + i]) with the ONE
    // witness witnesses[g], folded with gammas[g]; the groups are combined with the weights r^g.  gammas[g] must be unpredictable to
    // whoever chose the polynomials and the claimed values, r to whoever produced everything: see the header.
    bool verify_fold(const std::vector<Scalar> &zs, const std::vector<Scalar> &ys, const std::vector<KZGCommitment> &commitments,
                     const std::vector<uint32_t> &commitment_idx, const std::vector<KZGWitness> &witnesses, size_t t,
                     const std::vector<Scalar> &gammas, const Scalar &r) const {
        if (!params_.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        const size_t groups = zs.size();
        if (t == 0 || ys.size() / t != groups || ys.size() != groups * t || witnesses.size() != groups || gammas.size() != groups ||
            (!commitment_idx.empty() && commitment_idx.size() != ys.size()))
            throw ReferencePanic("verify_fold: shape");
        std::vector<uint8_t> cb(commitments.size() * 96), wb(groups * 96);
        for (size_t i = 0; i < commitments.size(); i++) std::memcpy(cb.data() + 96 * i, commitments[i].bytes.data(), 96);
        for (size_t i = 0; i < groups; i++) std::memcpy(wb.data() + 96 * i, witnesses[i].bytes.data(), 96);
        int ok = 0;
        e_.check(kzg_verify_fold(e_.ctx(), params_.gs, params_.hs, zs.data(), ys.data(), KZG_FR_CANONICAL_LE_32, cb.data(), commitments.size(),
                                 commitment_idx.empty() ? nullptr : commitment_idx.data(), wb.data(), KZG_G1_AFFINE_MONT_96, t, groups,
                                 gammas.data(), r.le.data(), &ok));
        return ok != 0;
    }
    // kzg_verify_multiopen: true iff the two elements (d, pi) answer ALL claims p_{m(k)}(zs[k]) = ys[k], m(k) = commitment_idx[k] (empty:
    // k), from one pairing check.  r as the prover used it; t MUST have been drawn after d was received: see the header.
    bool verify_multiopen(const std::vector<Scalar> &zs, const std::vector<Scalar> &ys, const std::vector<KZGCommitment> &commitments,
                          const std::vector<uint32_t> &commitment_idx, const Scalar &r, const Scalar &t, const KZGCommitment &d,
                          const KZGWitness &pi) const {
        if (!params_.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        if (ys.size() != zs.size() || (!commitment_idx.empty() && commitment_idx.size() != zs.size())) throw ReferencePanic("verify_multiopen: shape");
        std::vector<uint8_t> cb(commitments.size() * 96);
        for (size_t i = 0; i < commitments.size(); i++) std::memcpy(cb.data() + 96 * i, commitments[i].bytes.data(), 96);
        int ok = 0;
        e_.check(kzg_verify_multiopen(e_.ctx(), params_.gs, params_.hs, zs.data(), ys.data(), KZG_FR_CANONICAL_LE_32, cb.data(), commitments.size(),
                                      commitment_idx.empty() ? nullptr : commitment_idx.data(), zs.size(), r.le.data(), t.le.data(), d.bytes.data(),
                                      pi.bytes.data(), KZG_G1_AFFINE_MONT_96, &ok));
        return ok != 0;
    }
    bool verify_eval_batched(const std::vector<Scalar> &xs, const KZGCommitment &c, const KZGBatchWitness &w) const {  // :144-182
        if (!params_.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        int ok = 0;
        e_.check(kzg_verify_eval_batched(e_.ctx(), params_.gs, params_.hs, xs.data(), xs.size(), w.r.coeffs.data(),
                                         w.r.num_coeffs(), KZG_FR_CANONICAL_LE_32, c.bytes.data(), w.w.bytes.data(),
                                         KZG_G1_AFFINE_MONT_96, &ok));
        return ok != 0;
    }

  private:
    const KZGParams &params_;
    const Engine &e_;
};

// kzg_cosets_verifier: bulk verification of coset openings (coset i = { w^(i + tK) }, K = N / l, l = 2^log_l <= 256) for one
// KZGParams, one domain and one coset size.  verify(): cell k belongs to commitments[commitment_idx[k]] and coset coset_ids[k],
// with its l values at cells[k l ..) and its proof proofs[k]; one verdict per cell.  Not a reference type.
class CosetVerifier {
  public:
    CosetVerifier(const KZGParams &params, uint32_t log_n, uint32_t log_l) : e_(*params.engine), log_l_(log_l) {
        if (!params.hs) throw ReferencePanic("KZGParams.hs is empty (index out of bounds)");
        e_.check(kzg_cosets_verifier_setup(e_.ctx(), params.gs, params.hs, log_n, log_l, &plan_));
    }
    ~CosetVerifier() { kzg_cosets_verifier_free(e_.ctx(), plan_); }
    CosetVerifier(const CosetVerifier &) = delete;
    CosetVerifier &operator=(const CosetVerifier &) = delete;
    size_t domain() const { return shape(0); }
    size_t coset_size() const { return shape(1); }
    size_t table_bytes() const { return shape(2); }  // the window table's size in HBM
    std::vector<bool> verify(const std::vector<KZGCommitment> &commitments, const std::vector<uint32_t> &commitment_idx,
                             const std::vector<size_t> &coset_ids, const std::vector<Scalar> &cells,
                             const std::vector<KZGWitness> &proofs) const {
        const size_t count = proofs.size();
        if (commitment_idx.size() != count || coset_ids.size() != count || cells.size() != (count << log_l_))
            throw ReferencePanic("verify_cosets: shape");
        std::vector<uint8_t> cb(commitments.size() * 96), pb(count * 96), ok(count ? count : 1);
        for (size_t i = 0; i < commitments.size(); i++) std::memcpy(cb.data() + 96 * i, commitments[i].bytes.data(), 96);
        for (size_t i = 0; i < count; i++) std::memcpy(pb.data() + 96 * i, proofs[i].bytes.data(), 96);
        e_.check(kzg_verify_cosets(e_.ctx(), plan_, cb.data(), commitments.size(), commitment_idx.data(), coset_ids.data(), cells.data(),
                                   pb.data(), count, KZG_FR_CANONICAL_LE_32, KZG_G1_AFFINE_MONT_96, 0, ok.data()));
        return std::vector<bool>(ok.begin(), ok.begin() + count);
    }
    // kzg_verify_cosets_batch: true iff ALL the cells verify, from one pairing check of their combination with the weights r^k.
    // r must be unpredictable to whoever produced the cells (drawn after they arrived, or the hash of all inputs): see the header.
    // false says nothing about which cell is bad: verify() does.
    bool verify_batch(const std::vector<KZGCommitment> &commitments, const std::vector<uint32_t> &commitment_idx,
                      const std::vector<size_t> &coset_ids, const std::vector<Scalar> &cells, const std::vector<KZGWitness> &proofs,
                      const Scalar &r) const {
        const size_t count = proofs.size();
        if (commitment_idx.size() != count || coset_ids.size() != count || cells.size() != (count << log_l_))
            throw ReferencePanic("verify_cosets_batch: shape");
        std::vector<uint8_t> cb(commitments.size() * 96), pb(count * 96);
        for (size_t i = 0; i < commitments.size(); i++) std::memcpy(cb.data() + 96 * i, commitments[i].bytes.data(), 96);
        for (size_t i = 0; i < count; i++) std::memcpy(pb.data() + 96 * i, proofs[i].bytes.data(), 96);
        int ok = 0;
        e_.check(kzg_verify_cosets_batch(e_.ctx(), plan_, cb.data(), commitments.size(), commitment_idx.data(), coset_ids.data(), cells.data(),
                                         pb.data(), count, r.le.data(), KZG_FR_CANONICAL_LE_32, KZG_G1_AFFINE_MONT_96, 0, &ok));
        return ok != 0;
    }

  private:
    size_t shape(int which) const {
        size_t v[3] = {0, 0, 0};
        e_.check(kzg_cosets_verifier_shape(plan_, &v[0], &v[1], &v[2]));
        return v[which];
    }
    const Engine &e_;
    uint32_t log_l_;
    kzg_cosets_verifier *plan_ = nullptr;
};

// ---- multi-GPU: KZGParams.gs sharded over a group of GPUs, KZGProver::commit / create_witness over the group ----
// (the seam is the multi_exp call, src/coeff_form.rs:61,78; partial points are combined over RCCL inside the library)
// What a ONE-NODE host exports before the first RCCL call of the process (values already exported are kept): RCCL bootstraps every
// communicator over TCP on the first non-loopback interface it finds, which stalls formation for minutes on a host whose interface
// swallows packets; the library bounds formation (KZG_COMM_TIMEOUT_MS / "comm_timeout_ms") but the environment is the host's.
inline void single_node_rccl_env() {
    setenv("NCCL_SOCKET_IFNAME", "lo", 0);
    setenv("NCCL_RAS_ENABLE", "0", 0);
    setenv("NCCL_IB_DISABLE", "1", 0);
    setenv("NCCL_NET_PLUGIN", "none", 0);
}

class DeviceGroup {
  public:
    explicit DeviceGroup(const std::vector<int> &devices) {  // one process drives all GPUs
        single_node_rccl_env();
        if (int rc = kzg_mctx_create(devices.data(), (int)devices.size(), &m_))
            throw EngineError("kzg_mctx_create failed: " + std::to_string(rc) + ": " + kzg_mctx_create_error());
    }
    DeviceGroup(int device, int rank, int world, const void *unique_id) {  // one process per GPU
        single_node_rccl_env();
        if (int rc = kzg_mctx_create_rank(device, rank, world, unique_id, &m_))
            throw EngineError("kzg_mctx_create_rank failed: " + std::to_string(rc) + ": " + kzg_mctx_create_error());
    }
    ~DeviceGroup() { kzg_mctx_destroy(m_); }
    DeviceGroup(const DeviceGroup &) = delete;
    DeviceGroup &operator=(const DeviceGroup &) = delete;
    kzg_mctx *handle() const { return m_; }
    int world() const { return kzg_mctx_world(m_); }
    // which RCCL the group runs on, what forming its communicator cost per phase, each local context's pipeline plan (kzg_mctx_info)
    std::string info() const {
        char buf[2048];
        check(kzg_mctx_info(m_, buf, sizeof buf));
        return buf;
    }
    void check(int rc) const {
        if (rc == KZG_OK) return;
        std::string msg = kzg_mctx_last_error(m_);
        if (rc == KZG_ERR_POINT_NOT_ON_POLY) throw KZGError(KZGError::PointNotOnPolynomial, "point not on polynomial!");
        if (rc == KZG_ERR_SHAPE) throw ReferencePanic(msg);
        throw EngineError("kzg_mi355x error " + std::to_string(rc) + ": " + msg);
    }

  private:
    kzg_mctx *m_ = nullptr;
};

struct ShardedParams {  // KZGParams.gs held as one contiguous shard per GPU
    const DeviceGroup *group = nullptr;
    kzg_msrs *gs = nullptr;
    ShardedParams() = default;
    ShardedParams(const ShardedParams &) = delete;
    ShardedParams &operator=(const ShardedParams &) = delete;
    ShardedParams(ShardedParams &&o) noexcept : group(o.group), gs(o.gs) { o.gs = nullptr; }
    ~ShardedParams() { if (gs) kzg_msrs_free(group->handle(), gs); }
    size_t len() const { return kzg_msrs_len(gs); }
};

inline ShardedParams setup_sharded(const DeviceGroup &g, const Scalar &s, size_t num_coeffs) {  // src/lib.rs:38-47
    ShardedParams p;
    p.group = &g;
    g.check(kzg_srs_setup_g1_sharded(g.handle(), s.le.data(), KZG_FR_CANONICAL_LE_32, num_coeffs, &p.gs));
    return p;
}

class ShardedKZGProver {  // KZGProver (src/coeff_form.rs:37-81) with the SRS spread over the group
  public:
    explicit ShardedKZGProver(const ShardedParams &params) : params_(params), g_(*params.group) {}
    KZGCommitment commit(const Polynomial &p) const {  // :59-64
        G1Affine out;
        g_.check(kzg_commit_coeff_sharded(g_.handle(), params_.gs, p.coeffs.data(), p.num_coeffs(), KZG_FR_CANONICAL_LE_32, 0,
                                          out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }
    KZGWitness create_witness(const Polynomial &p, const Scalar &x, const Scalar &y) const {  // :66-81
        G1Affine out;
        g_.check(kzg_witness_coeff_sharded(g_.handle(), params_.gs, p.coeffs.data(), p.num_coeffs(), x.le.data(), y.le.data(),
                                           KZG_FR_CANONICAL_LE_32, 0, out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }
    // :83-111; returns the witness, `r` receives the interpolant (as the reference's (KZGWitness, Polynomial) pair)
    KZGWitness create_witness_batched(const Polynomial &p, const std::vector<Scalar> &xs, const std::vector<Scalar> &ys,
                                      Polynomial *r) const {
        G1Affine out;
        const size_t k = xs.size();
        std::vector<uint8_t> xb(32 * k), yb(32 * k), rb(32 * (k < 2 ? 2 : k));
        for (size_t i = 0; i < k; i++) {
            std::memcpy(&xb[32 * i], xs[i].le.data(), 32);
            std::memcpy(&yb[32 * i], ys[i].le.data(), 32);
        }
        size_t rl = 0;
        g_.check(kzg_witness_coeff_batched_sharded(g_.handle(), params_.gs, p.coeffs.data(), p.num_coeffs(), xb.data(), yb.data(), k,
                                                   KZG_FR_CANONICAL_LE_32, 0, out.bytes.data(), KZG_G1_AFFINE_MONT_96, rb.data(), &rl));
        if (r) {
            std::vector<Scalar> c(rl);
            std::memcpy(c.data(), rb.data(), 32 * rl);
            *r = Polynomial::make(std::move(c));
        }
        return out;
    }

    // KZGProverEvalForm::create_witness over the group (src/eval_form.rs:124-140); `lagrange` = the Lagrange-basis SRS sharded
    // over the same group (kzg_srs_upload_g1_sharded), evals = the d evaluations
    KZGWitness create_witness_eval(const kzg_msrs *lagrange, const std::vector<Scalar> &evals, size_t index) const {
        G1Affine out;
        g_.check(kzg_witness_eval_sharded(g_.handle(), lagrange, evals.data(), evals.size(), index, KZG_FR_CANONICAL_LE_32, 0,
                                          out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }

  private:
    const ShardedParams &params_;
    const DeviceGroup &g_;
};

class KZGProverEvalForm {  // src/eval_form.rs:39-147
  public:
    KZGProverEvalForm(const KZGParams &params, const kzg_srs *lagrange_basis_g)  // :88-100
        : params_(params), lag_(lagrange_basis_g), e_(*params.engine) {
        int rc = kzg_compute_omega(params.len(), &d_, &exp_, omega_.le.data(), KZG_FR_CANONICAL_LE_32);
        if (rc) throw ReferencePanic("compute_omega(...).unwrap()");
    }
    size_t degree() const { return d_; }
    Scalar omega() const { return omega_; }
    KZGCommitment commit(const EvaluationDomain &ev) const {  // :114-122
        if (d_ != ev.d) throw ReferencePanic("assert!(self.d == evals.d)");
        G1Affine out;
        e_.check(kzg_commit_eval(e_.ctx(), lag_, ev.coeffs.data(), ev.len(), KZG_FR_CANONICAL_LE_32, 0, out.bytes.data(),
                                 KZG_G1_AFFINE_MONT_96));
        return out;
    }
    KZGWitness create_witness(const EvaluationDomain &ev, size_t i) const {  // :124-140
        G1Affine out;
        e_.check(kzg_witness_eval(e_.ctx(), lag_, ev.coeffs.data(), ev.len(), i, KZG_FR_CANONICAL_LE_32, 0,
                                  out.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return out;
    }
    KZGWitness create_witness_all() const { return G1Affine{}; }  // :142-146: the identity
    // kzg_open_eval: (y, witness) at ANY point z of Fr against the Lagrange SRS alone; at z = omega^i the witness is
    // create_witness(ev, i).  Not a reference method.
    std::pair<Scalar, KZGWitness> open_at(const EvaluationDomain &ev, const Scalar &z) const {
        std::pair<Scalar, KZGWitness> r;
        e_.check(kzg_open_eval(e_.ctx(), lag_, ev.coeffs.data(), ev.len(), 1, z.le.data(), KZG_FR_CANONICAL_LE_32, 0, r.first.le.data(),
                               r.second.bytes.data(), KZG_G1_AFFINE_MONT_96));
        return r;
    }
    // one call for zs.size() polynomials: evals holds their evaluations back to back (zs.size() x degree() scalars)
    std::pair<std::vector<Scalar>, std::vector<KZGWitness>> open_at_batch(const std::vector<Scalar> &evals, const std::vector<Scalar> &zs) const {
        static_assert(sizeof(Scalar) == 32 && sizeof(G1Affine) == 96, "packed encodings");
        if (evals.size() != zs.size() * d_) throw ReferencePanic("open_at_batch: one evaluation vector of degree() scalars per point");
        std::pair<std::vector<Scalar>, std::vector<KZGWitness>> r{std::vector<Scalar>(zs.size()), std::vector<KZGWitness>(zs.size())};
        e_.check(kzg_open_eval(e_.ctx(), lag_, evals.data(), d_, zs.size(), zs.data(), KZG_FR_CANONICAL_LE_32, 0, r.first.data(),
                               r.second.data(), KZG_G1_AFFINE_MONT_96));
        return r;
    }
    // kzg_open_fold_eval: zs.size() groups of t evaluation vectors each (evals: groups x t x degree() scalars back to back), group g
    // opened at zs[g], any point of Fr: the groups x t values and ONE witness per group, open_at of sum_i gammas[g]^i evals_{g,i}.
    // KZGVerifier::verify_fold checks it.  Not a reference method.
    std::pair<std::vector<Scalar>, std::vector<KZGWitness>> open_fold_batch(const std::vector<Scalar> &evals, size_t t, const std::vector<Scalar> &zs,
                                                                              const std::vector<Scalar> &gammas) const {
        static_assert(sizeof(Scalar) == 32 && sizeof(G1Affine) == 96, "packed encodings");
        if (t == 0 || gammas.size() != zs.size() || evals.size() / d_ / t != zs.size() || evals.size() != zs.size() * t * d_)
            throw ReferencePanic("open_fold_batch: groups x t evaluation vectors of degree() scalars, one point and one challenge per group");
        std::pair<std::vector<Scalar>, std::vector<KZGWitness>> r{std::vector<Scalar>(zs.size() * t), std::vector<KZGWitness>(zs.size())};
        e_.check(kzg_open_fold_eval(e_.ctx(), lag_, evals.data(), d_, t, zs.size(), zs.data(), gammas.data(), KZG_FR_CANONICAL_LE_32, 0,
                                    r.first.data(), r.second.data(), KZG_G1_AFFINE_MONT_96));
        return r;
    }

    // kzg_multiopen_eval_commit / _finish: claim k is the polynomial with the evaluations number poly_idx[k] (empty poly_idx: k) of the
    // evals.size() / degree() vectors (back to back) at zs[k], any point of Fr.  t MUST be drawn after D exists: see the header.
    KZGMultiopenCommit multiopen_commit(const std::vector<Scalar> &evals, const std::vector<uint32_t> &poly_idx, const std::vector<Scalar> &zs,
                                        const Scalar &r) const {
        static_assert(sizeof(Scalar) == 32 && sizeof(G1Affine) == 96, "packed encodings");
        if (evals.size() % d_ != 0 || (!poly_idx.empty() && poly_idx.size() != zs.size())) throw ReferencePanic("multiopen_commit: shape");
        KZGMultiopenCommit c{std::vector<Scalar>(zs.size()), std::vector<Scalar>(d_), KZGCommitment{}};
        e_.check(kzg_multiopen_eval_commit(e_.ctx(), lag_, evals.data(), d_, evals.size() / d_, poly_idx.empty() ? nullptr : poly_idx.data(), zs.data(),
                                           zs.size(), r.le.data(), KZG_FR_CANONICAL_LE_32, 0, c.ys.data(), c.g.data(), &c.d, KZG_G1_AFFINE_MONT_96));
        return c;
    }
    std::pair<KZGWitness, Scalar> multiopen_finish(const std::vector<Scalar> &evals, const std::vector<uint32_t> &poly_idx, const std::vector<Scalar> &zs,
                                                   const Scalar &r, const Scalar &t, const std::vector<Scalar> &g) const {
        if (evals.size() % d_ != 0 || g.size() != d_ || (!poly_idx.empty() && poly_idx.size() != zs.size())) throw ReferencePanic("multiopen_finish: shape");
        std::pair<KZGWitness, Scalar> out;
        e_.check(kzg_multiopen_eval_finish(e_.ctx(), lag_, evals.data(), d_, evals.size() / d_, poly_idx.empty() ? nullptr : poly_idx.data(), zs.data(),
                                           zs.size(), r.le.data(), t.le.data(), g.data(), KZG_FR_CANONICAL_LE_32, 0, &out.second, &out.first,
                                           KZG_G1_AFFINE_MONT_96));
        return out;
    }

  private:
    const KZGParams &params_;
    const kzg_srs *lag_;
    const Engine &e_;
    size_t d_ = 0;
    uint32_t exp_ = 0;
    Scalar omega_;
};

}  // namespace kzg
