// vcb_host.h -- the host-side logic of the one-pairing verify calls (verify_cosets_batch.hip, verify_eval_batch.hip): the counting sort
// of a chunk's openings by commitment, and the weights of kzg_verify_fold.  field.h only, no HIP: tests/host_vcb_host.cpp compiles it
// with the sanitizers.
#pragma once
#include <new>
#include <vector>

#include "field.h"

namespace kzg {

// A chunk's openings listed per commitment, as k_vcb_cweights reads them.  One object serves every chunk of a call.
struct VcbLists {
    std::vector<uint32_t> cnt;    // per commitment; zero between two builds
    std::vector<uint32_t> which;  // list g -> its commitment, in the order of the commitments' first opening in the chunk
    std::vector<uint32_t> start;  // list g -> its openings order[start[g] .. start[g + 1]); lists + 1 entries
    std::vector<uint32_t> order;  // chunk-local opening indices, list after list, ascending inside a list

    // room for chunks of at most B0 openings naming commitments below n_commitments; false: out of host memory (no exception may
    // leave through the C ABI)
    bool reserve(size_t n_commitments, size_t B0) noexcept {
        try {
            cnt.assign(n_commitments, 0);
            which.resize(B0);
            start.resize(B0 + 1);
            order.resize(B0);
        } catch (const std::bad_alloc &) {
            return false;
        }
        return true;
    }

    // the lists of the B <= B0 openings with the commitments cm[k] < n_commitments; returns how many lists
    size_t build(const uint32_t *cm, size_t B) {
        size_t lists = 0;
        for (size_t k = 0; k < B; k++)
            if (!cnt[cm[k]]++) which[lists++] = cm[k];
        uint32_t at = 0;
        for (size_t g = 0; g < lists; g++) {
            start[g] = at;
            at += cnt[which[g]];
            cnt[which[g]] = start[g];
        }
        start[lists] = at;
        for (size_t k = 0; k < B; k++) order[cnt[cm[k]]++] = (uint32_t)k;
        for (size_t g = 0; g < lists; g++) cnt[which[g]] = 0;
        return lists;
    }
};

// The weights of kzg_verify_fold, rho_{g,i} = r^g gamma_g^i for i < t, in the order (g, i): the walk keeps its place between two
// chunks.  Every scalar is in Montgomery form.
struct FoldWalk {
    size_t wg = 0, wi = 0;
    Fr rg = Fr::one(), w = Fr::one();  // r^wg, r^wg gamma_wg^wi
};
// rho[k] for the next B pairs; gm[g] = gamma_g (read for g below the number of groups only)
inline void fold_weights(FoldWalk *s, size_t t, const Fr &r, const Fr *gm, size_t B, Fr *rho) {
    for (size_t k = 0; k < B; k++) {
        rho[k] = s->w;
        if (++s->wi == t) {
            s->wi = 0;
            s->wg++;
            s->rg = mul(s->rg, r);
            s->w = s->rg;
        } else {
            s->w = mul(s->w, gm[s->wg]);
        }
    }
}

}  // namespace kzg
