// tower_hooks.h -- the record-level bodies of kzg_test_tower (include/kzg_mi355x_test.h), shared by its two builds: the device twin
// kzg_amd/csrc/tower_hooks.hip (hipcc, gfx950: mul(Fq, Fq) is mul_gfx950.inc and every tower function runs out of line on operands in
// scratch memory) and the host shim ht_tower_op of tests/host_tower.cpp (g++: the portable C).  One definition of every op, so the two
// builds cannot drift apart: what differs between them is only what tower.h itself resolves to.  Test infrastructure; the product
// library does not include this file.
//
// A record is an array of u32 words: field elements canonical little-endian (Fq 12 words, Fq2 24, Fq12 144 as the six f12_coeff
// coefficients, G1 affine 24, G2 affine 48, all zero = the identity), converted to and from Montgomery form here.
//
// ALIASING.  tower.h is called aliased almost everywhere in the product (f12_mul(f, f, l), f12_sqr(f, f), f12_cyclotomic_sqr(acc, acc),
// g2_add(acc, acc, pj)), so every field op carries an `alias` word and tt_alias2 / tt_alias1 make the call ON THE OBJECTS NAMED:
//   0  r distinct from the inputs     1  r is a     2  r is b     3  a is b, r distinct     4  r, a and b one object
// (unary ops: 0 or 1).  No operand is copied first: a copy would test another call than the one the product makes.
#pragma once
#include "tower.h"
#include "../../include/kzg_mi355x_test.h"

namespace kzg {

struct TowerShape {
    uint32_t in_rec, out_rec;  // bytes
};
constexpr uint32_t TT_LINES_WORDS = 2 * MILLER_LINES * 24;  // one stored-lines table as canonical words
// indexed by the KZG_TOWER_* op
constexpr TowerShape kTowerShapes[KZG_TOWER_NUM_OPS] = {
    {196, 96},   {100, 96},  {100, 96},  {148, 96},  {100, 96},                                        // Fq2
    {1156, 576}, {580, 576}, {580, 576}, {580, 576}, {584, 576}, {580, 576}, {576, 4}, {580, 576}, {864, 576},  // Fq12
    {388, 192},  {196, 192}, {224, 192}, {192, 4},                                                     // G2
    {192, 4 * TT_LINES_WORDS}, {1160, 576}, {576, 576}, {1160, 4}};                                    // pairing
// per-record workspace of the ops that store Miller lines (MAX 4 pairs): Fq2 elements
constexpr size_t TT_TABS_PER_RECORD = 4 * 2 * MILLER_LINES;

KZG_HD bool tower_op_needs_tabs(int op) {
    return op == KZG_TOWER_G2_PRECOMPUTE_LINES || op == KZG_TOWER_MILLER_LOOP || op == KZG_TOWER_PAIRING_PRODUCT_IS_ONE;
}

// what a kernel takes from a record and branches or loops on: outside these ranges the record is refused before any launch
inline bool tower_record_ok(int op, const uint32_t *w) {
    switch (op) {
    case KZG_TOWER_F2_MUL: return w[48] <= 4;
    case KZG_TOWER_F2_SQR:
    case KZG_TOWER_F2_INV:
    case KZG_TOWER_F2_MUL_XI: return w[24] <= 1;
    case KZG_TOWER_F2_MUL_FQ: return w[36] <= 1;
    case KZG_TOWER_F12_MUL: return w[288] <= 4;
    case KZG_TOWER_F12_SQR:
    case KZG_TOWER_F12_CYCLOTOMIC_SQR:
    case KZG_TOWER_F12_INV:
    case KZG_TOWER_F12_CONJ:
    case KZG_TOWER_F12_EXP_Z: return w[144] <= 1;
    case KZG_TOWER_F12_FROB: return (w[144] == 1 || w[144] == 2) && w[145] <= 1;
    case KZG_TOWER_G2_ADD: return w[96] <= 4;
    case KZG_TOWER_G2_DOUBLE: return w[48] <= 1;
    case KZG_TOWER_MILLER_LOOP:
    case KZG_TOWER_PAIRING_PRODUCT_IS_ONE: return w[0] >= 1 && w[0] <= 4 && w[1] < (1u << w[0]);
    default: return true;
    }
}

KZG_HD Fq tt_ld_fq(const uint32_t *p) {
    Fq a;
    for (int i = 0; i < 12; i++) a.v[i] = p[i];
    return to_mont(a);
}
KZG_HD void tt_st_fq(uint32_t *p, const Fq &a) {
    Fq c = from_mont(a);
    for (int i = 0; i < 12; i++) p[i] = c.v[i];
}
KZG_HD Fq2 tt_ld_f2(const uint32_t *p) { return Fq2{tt_ld_fq(p), tt_ld_fq(p + 12)}; }
KZG_HD void tt_st_f2(uint32_t *p, const Fq2 &a) {
    tt_st_fq(p, a.c0);
    tt_st_fq(p + 12, a.c1);
}
KZG_HD void tt_ld_f12(Fq12 &a, const uint32_t *p) {
    for (int k = 0; k < 6; k++) *f12_coeff(a, k) = tt_ld_f2(p + 24 * k);
}
KZG_HD void tt_st_f12(uint32_t *p, Fq12 &a) {
    for (int k = 0; k < 6; k++) tt_st_f2(p + 24 * k, *f12_coeff(a, k));
}
KZG_HD G1Affine tt_ld_g1(const uint32_t *p) { return G1Affine{tt_ld_fq(p), tt_ld_fq(p + 12)}; }
KZG_HD G2Affine tt_ld_g2(const uint32_t *p) { return G2Affine{tt_ld_f2(p), tt_ld_f2(p + 24)}; }
KZG_HD void tt_st_g2(uint32_t *p, const G2Affine &a) {
    tt_st_f2(p, a.x);
    tt_st_f2(p + 24, a.y);
}

// op(r, a, b) in the aliasing form `alias` over the objects x (operand a), y (operand b) and t (a third object); returns the object
// that holds the result.  Forms 3 and 4 compute op(a, a): the record's b is not used.
template <class T, class F>
KZG_HD T &tt_alias2(uint32_t alias, T &x, T &y, T &t, F op) {
    switch (alias) {
    case 1: op(x, x, y); return x;
    case 2: op(y, x, y); return y;
    case 3: op(t, x, x); return t;
    case 4: op(x, x, x); return x;
    default: op(t, x, y); return t;
    }
}
template <class T, class F>
KZG_HD T &tt_alias1(uint32_t alias, T &x, T &t, F op) {
    if (alias == 1) {
        op(x, x);
        return x;
    }
    op(t, x);
    return t;
}

// the pairs of a MILLER_LOOP / PAIRING_PRODUCT_IS_ONE record: u32 np, u32 mask, 4 x G1, 4 x G2.  Pair i with bit i of `mask` set uses
// stored lines, precomputed here from Q_i into `tabs` (an identity Q_i leaves an all-zero table, as an identity SRS point does in
// kzg_verify_eval); with no bit set the table argument is absent altogether, as in k_pairing_check.
struct TowerPairs {
    G1Affine P[4];
    G2Affine Q[4], T[4];
    const Fq2 *tp[4];
    int np;
    bool stored;
};
KZG_HD void tt_ld_pairs(TowerPairs &s, const uint32_t *in, Fq2 *tabs) {
    s.np = (int)in[0];
    const uint32_t mask = in[1];
    s.stored = mask != 0;
    for (int i = 0; i < s.np; i++) {
        s.P[i] = tt_ld_g1(in + 2 + 24 * i);
        s.Q[i] = tt_ld_g2(in + 98 + 48 * i);
        s.tp[i] = nullptr;
        if ((mask >> i) & 1) {
            Fq2 *tab = tabs + (size_t)i * 2 * MILLER_LINES;
            g2_precompute_lines(s.Q[i], tab);
            s.tp[i] = tab;
        }
    }
}

// one record of op OP: `in` -> `out`; `tabs`: TT_TABS_PER_RECORD Fq2 of workspace for the ops of tower_op_needs_tabs
template <int OP>
KZG_HD void tower_record(const uint32_t *in, uint32_t *out, Fq2 *tabs) {
    if constexpr (OP == KZG_TOWER_F2_MUL) {
        Fq2 x = tt_ld_f2(in), y = tt_ld_f2(in + 24), t;
        tt_st_f2(out, tt_alias2(in[48], x, y, t, [](Fq2 &r, const Fq2 &a, const Fq2 &b) { f2_mul(r, a, b); }));
    } else if constexpr (OP == KZG_TOWER_F2_SQR) {
        Fq2 x = tt_ld_f2(in), t;
        tt_st_f2(out, tt_alias1(in[24], x, t, [](Fq2 &r, const Fq2 &a) { f2_sqr(r, a); }));
    } else if constexpr (OP == KZG_TOWER_F2_INV) {
        Fq2 x = tt_ld_f2(in), t;
        tt_st_f2(out, tt_alias1(in[24], x, t, [](Fq2 &r, const Fq2 &a) { f2_inv(r, a); }));
    } else if constexpr (OP == KZG_TOWER_F2_MUL_FQ) {
        Fq2 x = tt_ld_f2(in), t;
        Fq k = tt_ld_fq(in + 24);
        tt_st_f2(out, tt_alias1(in[36], x, t, [&k](Fq2 &r, const Fq2 &a) { f2_mul_fq(r, a, k); }));
    } else if constexpr (OP == KZG_TOWER_F2_MUL_XI) {
        Fq2 x = tt_ld_f2(in), t;
        tt_st_f2(out, tt_alias1(in[24], x, t, [](Fq2 &r, const Fq2 &a) { f2_mul_xi(r, a); }));
    } else if constexpr (OP == KZG_TOWER_F12_MUL) {
        Fq12 x, y, t;
        tt_ld_f12(x, in);
        tt_ld_f12(y, in + 144);
        tt_st_f12(out, tt_alias2(in[288], x, y, t, [](Fq12 &r, const Fq12 &a, const Fq12 &b) { f12_mul(r, a, b); }));
    } else if constexpr (OP == KZG_TOWER_F12_SQR || OP == KZG_TOWER_F12_CYCLOTOMIC_SQR || OP == KZG_TOWER_F12_INV ||
                         OP == KZG_TOWER_F12_CONJ || OP == KZG_TOWER_F12_EXP_Z) {
        Fq12 x, t;
        tt_ld_f12(x, in);
        tt_st_f12(out, tt_alias1(in[144], x, t, [](Fq12 &r, const Fq12 &a) {
                      if constexpr (OP == KZG_TOWER_F12_SQR) f12_sqr(r, a);
                      else if constexpr (OP == KZG_TOWER_F12_CYCLOTOMIC_SQR) f12_cyclotomic_sqr(r, a);
                      else if constexpr (OP == KZG_TOWER_F12_INV) f12_inv(r, a);
                      else if constexpr (OP == KZG_TOWER_F12_CONJ) f12_conj(r, a);
                      else f12_exp_z(r, a);
                  }));
    } else if constexpr (OP == KZG_TOWER_F12_FROB) {
        Fq12 x, t;
        tt_ld_f12(x, in);
        const uint32_t power = in[144];
        tt_st_f12(out, tt_alias1(in[145], x, t, [power](Fq12 &r, const Fq12 &a) {
                      if (power == 1) f12_frob(r, a);
                      else f12_frob2(r, a);
                  }));
    } else if constexpr (OP == KZG_TOWER_F12_IS_ONE) {
        Fq12 x;
        tt_ld_f12(x, in);
        out[0] = f12_is_one(x) ? 1u : 0u;
    } else if constexpr (OP == KZG_TOWER_F12_MUL_LINE) {  // in place on f by its signature
        Fq12 f;
        tt_ld_f12(f, in);
        Fq2 lam = tt_ld_f2(in + 144), cst = tt_ld_f2(in + 168);
        G1Affine P = tt_ld_g1(in + 192);
        f12_mul_line(f, lam, cst, P);
        tt_st_f12(out, f);
    } else if constexpr (OP == KZG_TOWER_G2_ADD) {
        G2Jacobian x, y, t;
        g2_from_affine(x, tt_ld_g2(in));
        g2_from_affine(y, tt_ld_g2(in + 48));
        G2Affine r;
        g2_to_affine(r, tt_alias2(in[96], x, y, t, [](G2Jacobian &o, const G2Jacobian &a, const G2Jacobian &b) { g2_add(o, a, b); }));
        tt_st_g2(out, r);
    } else if constexpr (OP == KZG_TOWER_G2_DOUBLE) {
        G2Jacobian x, t;
        g2_from_affine(x, tt_ld_g2(in));
        G2Affine r;
        g2_to_affine(r, tt_alias1(in[48], x, t, [](G2Jacobian &o, const G2Jacobian &a) { g2_dbl(o, a); }));
        tt_st_g2(out, r);
    } else if constexpr (OP == KZG_TOWER_G2_MUL) {
        uint32_t k[8];
        for (int i = 0; i < 8; i++) k[i] = in[48 + i];
        G2Jacobian j;
        g2_scalar_mul(j, tt_ld_g2(in), k);
        G2Affine r;
        g2_to_affine(r, j);
        tt_st_g2(out, r);
    } else if constexpr (OP == KZG_TOWER_G2_ON_CURVE) {
        out[0] = g2_on_curve(tt_ld_g2(in)) ? 1u : 0u;
    } else if constexpr (OP == KZG_TOWER_G2_PRECOMPUTE_LINES) {
        g2_precompute_lines(tt_ld_g2(in), tabs);
        for (int k = 0; k < 2 * MILLER_LINES; k++) tt_st_f2(out + 24 * k, tabs[k]);
    } else if constexpr (OP == KZG_TOWER_MILLER_LOOP) {
        TowerPairs s;
        tt_ld_pairs(s, in, tabs);
        Fq12 f;
        miller_loop(f, s.P, s.Q, s.T, s.np, s.stored ? s.tp : nullptr);
        tt_st_f12(out, f);
    } else if constexpr (OP == KZG_TOWER_FINAL_EXPONENTIATION) {
        Fq12 x, y;
        tt_ld_f12(x, in);
        final_exponentiation(y, x);
        tt_st_f12(out, y);
    } else if constexpr (OP == KZG_TOWER_PAIRING_PRODUCT_IS_ONE) {
        TowerPairs s;
        tt_ld_pairs(s, in, tabs);
        out[0] = pairing_product_is_one(s.P, s.Q, s.T, s.np, s.stored ? s.tp : nullptr) ? 1u : 0u;
    }
}

}  // namespace kzg
