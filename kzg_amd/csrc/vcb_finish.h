// vcb_finish.h -- the end of kzg_verify_cosets_batch: about 300 dependent group operations and one pairing product.  Host and device
// code (tower.h only, no HIP): the calling thread runs it on one download of the window sums (option host_pairing = 1), a one-thread
// kernel runs the same functions otherwise, and tests/host_vcb_finish.cpp compiles it with the sanitizers.
#pragma once
#include "tower.h"

namespace kzg {

constexpr int VCB_W = 32;  // windows of 8 bits (VC_W)
// what the bucket reductions leave: win[s][w] = sum_b b B_{s,w,b} for the three bucket sets s = 0: (pi, rho), 1: (pi, rho h), 2: (C, c),
// and Ragg = sum_j a_j gs[j] from the fixed-base table
struct VcbSums {
    G1Xyzz win[3][VCB_W];
    G1Xyzz ragg;
};

// sum_w 2^(8 w) win[w]: Horner from the top window, 8 doublings per step
KZG_NI void vcb_horner(G1Xyzz &r, const G1Xyzz *win) {
    G1Xyzz acc = G1Xyzz::inf();
    for (int w = VCB_W - 1; w >= 0; w--) {
        for (int i = 0; i < 8; i++) acc = g1_dbl(acc);
        acc = g1_add(acc, win[w]);
    }
    r = acc;
}

// ok = [ e(P1, hs[l]) e(-(P2 + Cagg - Ragg), hs[0]) == 1 ] for tot = { P1, P2, Cagg };  hq = { hs[0], hs[l] }, lines = their stored
// Miller lines in that order.  parts (may be null): P1, P2, Cagg, Ragg in affine form
KZG_NI bool vcb_check(const G1Xyzz *tot, const G1Xyzz &ragg, const G2Affine *hq, const Fq2 *lines, G1Affine *parts) {
    const G1Xyzz P1 = tot[0], P2 = tot[1], Cagg = tot[2];
    if (parts) {
        parts[0] = g1_to_affine(P1);
        parts[1] = g1_to_affine(P2);
        parts[2] = g1_to_affine(Cagg);
        parts[3] = g1_to_affine(ragg);
    }
    G1Xyzz nr = ragg;
    if (!nr.y.is_zero()) nr.y = neg(nr.y);
    const G1Xyzz acc = g1_add(g1_add(P2, Cagg), nr);
    G1Affine P[2];
    G2Affine Q[2], T[2];
    const Fq2 *tabs[2] = {lines + 2 * MILLER_LINES, lines};  // pair 0 against hs[l], pair 1 against hs[0]
    P[0] = g1_to_affine(P1);
    P[1] = g1_neg(g1_to_affine(acc));
    Q[0] = hq[1];
    Q[1] = hq[0];
    return pairing_product_is_one(P, Q, T, 2, tabs);
}

// the whole finish on one thread (the calling thread).  The kernel k_vcb_finish runs the three Horner chains on three lanes of one
// wave, which costs it the time of one chain, then vcb_check on one lane.
KZG_NI bool vcb_finish(const VcbSums &s, const G2Affine *hq, const Fq2 *lines, G1Affine *parts) {
    G1Xyzz tot[3];
    for (int i = 0; i < 3; i++) vcb_horner(tot[i], s.win[i]);
    return vcb_check(tot, s.ragg, hq, lines, parts);
}

}  // namespace kzg
