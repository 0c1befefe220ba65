// multiopen_plan.h -- the host-side plan of the two-element multiproof (kzg_multiopen_* in capi.hip, kzg_verify_multiopen in
// verify_eval_batch.hip).  field.h only, no HIP: tests/host_multiopen_plan.cpp compiles it with the sanitizers.
//   claims k < N: polynomial m(k), point z_k; challenges r and t
//   prover, first phase    the claims sorted by point (equal points adjacent), the distinct points z_u with their claim ranges, the
//                          weights r^k, the distinct points cut into chunks of at most `cap`
//   second phase, verifier w_k = r^k / (t - z_k) with ONE inversion per run of claims (Montgomery's trick), W_m = sum_{m(k) = m} w_k
// Every scalar is in Montgomery form.
#pragma once
#include <algorithm>
#include <vector>

#include "field.h"

namespace kzg {

struct MoPlan {
    std::vector<uint32_t> order;   // position s of the sorted claims -> claim k
    std::vector<uint32_t> pstart;  // distinct point u -> its sorted claims [pstart[u], pstart[u + 1]); U + 1 entries
    std::vector<Fr> z;             // the distinct points, in the sorted order
    std::vector<Fr> rk;            // r^k, by claim
    size_t points() const { return z.size(); }
};

inline bool mo_less(const Fr &a, const Fr &b) {  // the order of the representations as 256-bit integers: any total order does
    for (int i = 7; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    return false;
}

// the claims sorted by point (claims of one point keep their order), the distinct points and r^k
inline void mo_plan(const Fr *z, size_t count, const Fr &r, MoPlan *p) {
    p->order.resize(count);
    p->rk.resize(count);
    p->pstart.clear();
    p->z.clear();
    Fr w = Fr::one();
    for (size_t k = 0; k < count; k++) {
        p->order[k] = (uint32_t)k;
        p->rk[k] = w;
        w = mul(w, r);
    }
    std::stable_sort(p->order.begin(), p->order.end(), [&](uint32_t a, uint32_t b) { return mo_less(z[a], z[b]); });
    for (size_t s = 0; s < count; s++)
        if (s == 0 || z[p->order[s]] != z[p->order[s - 1]]) {
            p->pstart.push_back((uint32_t)s);
            p->z.push_back(z[p->order[s]]);
        }
    p->pstart.push_back((uint32_t)count);
}

// The distinct points with on[u] == 0 first (both parts keep their order) and their claims with them; src[u] = the place the point had
// before.  Returns how many points have on[u] == 0: the evaluation-form driver works those off in chunks, the others one by one.
inline size_t mo_off_domain_first(MoPlan *p, const uint8_t *on, std::vector<uint32_t> *src) {
    const size_t U = p->points();
    std::vector<uint32_t> order, pstart;
    std::vector<Fr> z;
    size_t n_off = 0;
    src->clear();
    for (int pass = 0; pass < 2; pass++)
        for (size_t u = 0; u < U; u++) {
            if ((on[u] != 0) != (pass == 1)) continue;
            pstart.push_back((uint32_t)order.size());
            z.push_back(p->z[u]);
            src->push_back((uint32_t)u);
            for (uint32_t s = p->pstart[u]; s < p->pstart[u + 1]; s++) order.push_back(p->order[s]);
            if (!pass) n_off++;
        }
    pstart.push_back((uint32_t)order.size());
    p->order.swap(order);
    p->pstart.swap(pstart);
    p->z.swap(z);
    return n_off;
}

// distinct points per chunk: min(16, 2^22 / d), at least one, lowered by the option (0 = default)
inline size_t mo_chunk_points(size_t d, int option) {
    size_t cap = std::max<size_t>(1, std::min<size_t>(16, ((size_t)1 << 22) / std::max<size_t>(d, 1)));
    if (option > 0) cap = std::min(cap, (size_t)option);
    return cap;
}

// w[k] = rk / (t - z[k]) for a run of n claims, rk = r^(first claim of the run) on entry and r^(first claim behind it) on return: a
// caller that works in chunks carries it.  One field inversion per run.  False (nothing written) when t equals a z[k].
inline bool mo_weights(const Fr *z, size_t n, const Fr &r, const Fr &t, Fr *rk, Fr *w) {
    if (!n) return true;
    Fr acc = Fr::one();
    for (size_t k = 0; k < n; k++) {  // w[k] = the product of the denominators before k
        const Fr den = sub(t, z[k]);
        if (den.is_zero()) return false;
        w[k] = acc;
        acc = mul(acc, den);
    }
    Fr ia = inv(acc);
    for (size_t k = n; k-- > 0;) {
        const Fr one_over = mul(w[k], ia);  // 1 / (t - z[k])
        ia = mul(ia, sub(t, z[k]));
        w[k] = one_over;
    }
    Fr p = *rk;
    for (size_t k = 0; k < n; k++) {
        w[k] = mul(w[k], p);
        p = mul(p, r);
    }
    *rk = p;
    return true;
}

// W[m] += sum of w[k] over the run's claims with m(k) = m (idx null: m(k) = first + k)
inline void mo_poly_weights(const Fr *w, const uint32_t *idx, size_t first, size_t n, Fr *W) {
    for (size_t k = 0; k < n; k++) {
        Fr &dst = W[idx ? idx[first + k] : first + k];
        dst = add(dst, w[k]);
    }
}

}  // namespace kzg
