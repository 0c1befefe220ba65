// Stand-alone host program (tests/test_host_madd_signed.py builds and runs it): the sign-tracked mixed addition of curve30.h -- the loop body
// of k_accum_affine -- against the plain g1_madd30 on chains of 64 table entries, and mul30_sgn against mul30_sub / mul30 + add30.
// The same headers are compiled by hipcc for gfx950; on the host the portable branches of field30.h run.
// Prints one line per failed check and a summary; exit status 0 iff every check passed.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../kzg_amd/csrc/curve30.h"
using namespace kzg;

static int failures = 0;
static long checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            failures++;                                   \
            if (failures <= 40) {                         \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;  // fixed seed (splitmix64)
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static G1Affine random_point() {
    uint32_t k[8];
    for (int i = 0; i < 8; i++) k[i] = (uint32_t)rnd();
    k[7] &= 0x3fffffffu;
    return g1_to_affine(g1_scalar_mul(g1_generator(), k));
}

static G1Affine30 neg_table(const G1Affine30 &a) {  // the table entry of -P (normalised again: a table coordinate is)
    G1Affine30 r = a;
    r.y = normalize30(neg30(a.y));
    return r;
}

static bool same_affine(const G1Xyzz30 &a, const G1Xyzz30 &b) {
    const G1Affine x = g1_to_affine(g1_xyzz_from30(a)), y = g1_to_affine(g1_xyzz_from30(b));
    return memcmp(&x, &y, sizeof x) == 0;
}

// ---- limb bounds --------------------------------------------------------------------------------------------------------------
// |value| < c q  =>  |limb 12| <= c q / 2^360 + 1 (the lower limbs are below 2^360 in magnitude); q / 2^360 < mod(12) + 1.  tenths = 10 c.
static int32_t top_bound(int tenths) { return (int32_t)(((int64_t)tenths * (Fq30Consts::mod(12) + 1)) / 10 + 2); }
static int32_t iabs(int32_t v) { return v < 0 ? -v : v; }

// an operand of the accumulation loop's next product that may carry UNSIGNED digits (X, ZZ, ZZZ: field30.h mul30_inline, "one operand
// of a later product whose other operand is balanced"; also the merged subtrahend of mul30_sub, any limbs below 2^31): limbs 0..11 in
// [-2^29, 2^30), the value below `tenths` / 10 q (curve30.h: |X3| < 2.2, ZZ, ZZZ < 0.6; after a restart x2 < 0.51 and one30 < 0.6;
// after a doubling X < 1.6)
static void check_lazy(const Fq30 &a, int tenths, const char *what, int step) {
    for (int i = 0; i < F30_N - 1; i++)
        CHECK(a.v[i] >= -F30_HALF && a.v[i] < (1 << F30_B), "%s limb %d = %d out of [-2^29, 2^30) at step %d", what, i, a.v[i], step);
    CHECK(iabs(a.v[F30_N - 1]) <= top_bound(tenths), "%s top limb %d above %d at step %d", what, a.v[F30_N - 1], top_bound(tenths), step);
}
// Yt: an operand of muladd30 after sgn30 (operand limbs |.| <= 2^29) and the merged term of mul30_sgn (below 2^31); value < 1.2 q
// (a product: < 0.6; the output of a doubling: < 1.2)
static void check_balanced(const Fq30 &a, int tenths, const char *what, int step) {
    for (int i = 0; i < F30_N - 1; i++)
        CHECK(iabs(a.v[i]) <= F30_HALF, "%s limb %d = %d above 2^29 at step %d", what, i, a.v[i], step);
    CHECK(iabs(a.v[F30_N - 1]) <= top_bound(tenths), "%s top limb %d above %d at step %d", what, a.v[F30_N - 1], top_bound(tenths), step);
}
static void check_acc(const G1Xyzz30 &p, int32_t sigma, int step) {
    CHECK(sigma == 1 || sigma == -1, "sigma = %d at step %d", sigma, step);
    if (p.inf) return;
    check_lazy(p.x, 22, "X", step);
    check_balanced(p.y, 12, "Yt", step);
    check_lazy(p.zz, 6, "ZZ", step);
    check_lazy(p.zzz, 6, "ZZZ", step);
}
// what a reader of the partial list hands to g1_add30 / the row and column sums: balanced digits, |X| < 8, |Y| < 8
static void check_partial(const G1Xyzz30 &p, int step) {
    CHECK(p.pad[0] == 0 && p.pad[1] == 0 && p.pad[2] == 0, "pad words not cleared at step %d", step);
    if (p.inf) return;
    const Fq30 *c[4] = {&p.x, &p.y, &p.zz, &p.zzz};
    for (int j = 0; j < 4; j++) check_balanced(*c[j], 80, "partial coordinate", step);
}

// ---- mul30_sgn ----------------------------------------------------------------------------------------------------------------
static Fq30 random_operand() {  // a normalised value below q / 2 in magnitude, or its limb-wise negation
    Fq a;
    for (int i = 0; i < 12; i++) a.v[i] = (uint32_t)rnd();
    a.v[11] &= 0x0fffffffu;  // below q
    Fq30 r = to30(a);
    return (rnd() & 1) ? neg30(r) : r;
}
static Fq30 random_limbs(int bits, int top_bits) {
    Fq30 r;
    for (int i = 0; i < F30_N; i++) {
        const int b = i == F30_N - 1 ? top_bits : bits;
        const int64_t m = (int64_t)1 << b;
        r.v[i] = (int32_t)((int64_t)(rnd() % (uint64_t)(2 * m - 1)) - (m - 1));  // in (-2^b, 2^b)
    }
    return r;
}
static bool same_limbs(const Fq30 &a, const Fq30 &b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

static void test_mul30_sgn() {
    for (int it = 0; it < 2000; it++) {
        const Fq30 a = random_operand(), b = random_operand();
        // t = -1: limb for limb mul30_sub, with c anywhere in its documented range (any limbs below 2^31; extremes included)
        Fq30 c = random_limbs(31, 24);
        if (it % 7 == 0)
            for (int i = 0; i < F30_N - 1; i++) c.v[i] = (it & 8) ? INT32_MAX : -INT32_MAX;
        CHECK(same_limbs(mul30_sgn(a, b, c, -1), mul30_sub(a, b, c)), "mul30_sgn(t = -1) != mul30_sub, iteration %d", it);
        // t = +1: limb for limb mul30 followed by add30 (both are the normalised form of the same integer); add30 takes limbs up to 2^29
        const Fq30 d = random_limbs(29, 24);
        CHECK(same_limbs(mul30_sgn(a, b, d, 1), add30(mul30(a, b), d)), "mul30_sgn(t = +1) != mul30 + add30, iteration %d", it);
        CHECK(same_limbs(sgn30(a, -1), neg30(a)) && same_limbs(sgn30(a, 1), a), "sgn30, iteration %d", it);
    }
}

// ---- chains -------------------------------------------------------------------------------------------------------------------
constexpr int CHAIN = 64;
enum { PLAIN = 0, SAME = 1, INVERSE = 2, IDENTITY = 3 };  // what entry i is relative to entry i - 1
struct Slot {
    int kind;
    bool boundary;  // a bucket boundary in front of entry i: flush the partial, restart from entry i
};

// The special entries sit where the accumulator IS the previous entry (right after a restart), so that SAME is a doubling and INVERSE
// gives infinity; each is followed by ordinary entries and then by a restart, and the restarts themselves fall on every kind of entry.
static std::vector<Slot> layout() {
    std::vector<Slot> L(CHAIN, Slot{PLAIN, false});
    L[1].kind = SAME;                                 // entry 0 starts the chain: 0, 1 = doubling
    L[5].boundary = true;  L[6].kind = INVERSE;       // restart at 5; 5, 6 = infinity; 7.. continue from infinity
    L[10].boundary = true; L[11].kind = IDENTITY;     // restart at 10; a table point at infinity; 12.. continue
    L[15].boundary = true; L[15].kind = IDENTITY;     // a restart ON an identity entry (the accumulator restarts as infinity)
    L[16].kind = PLAIN;
    L[20].boundary = true; L[21].kind = SAME; L[22].kind = SAME;   // doubling, then the same point again (an ordinary addition: 2P + P)
    L[23].boundary = true;                            // restart right after a doubling
    L[24].kind = INVERSE;                             // infinity ...
    L[25].boundary = true;                            // ... flushed as a partial at infinity
    L[30].kind = INVERSE;                             // mid-chain: -(previous entry), not the accumulator: an ordinary addition
    L[31].kind = SAME;
    L[40].boundary = true; L[41].boundary = true; L[42].boundary = true;  // one-entry buckets: a partial that is a bare table point
    L[43].kind = INVERSE; L[44].kind = INVERSE;       // P, -P (infinity), P again (restart from infinity inside a bucket)
    L[50].boundary = true; L[51].kind = IDENTITY; L[52].kind = SAME;  // identity, then "same as the identity" = identity again
    L[53].kind = PLAIN;
    L[60].boundary = true; L[61].kind = SAME; L[62].kind = INVERSE; L[63].kind = PLAIN;
    return L;
}

static void run_chain(const std::vector<G1Affine30> &pts, uint64_t signs, int pattern_id) {
    const std::vector<Slot> L = layout();
    // entry i as a table point: SAME / INVERSE are +-(entry i - 1)'s table point, chosen so that with the pattern's own signs the entry
    // ADDED is the previous added point (SAME) or its inverse (INVERSE)
    std::vector<G1Affine30> ent(CHAIN);
    G1Affine30 ident;
    ident.x = zero30();
    ident.y = zero30();
    for (unsigned i = 0; i < sizeof ident.pad / sizeof ident.pad[0]; i++) ident.pad[i] = 0;
    for (int i = 0; i < CHAIN; i++) {
        const bool flip = i > 0 && (((signs >> i) ^ (signs >> (i - 1))) & 1);
        switch (L[i].kind) {
            case PLAIN: ent[i] = pts[i]; break;
            case SAME: ent[i] = flip ? neg_table(ent[i - 1]) : ent[i - 1]; break;
            case INVERSE: ent[i] = flip ? ent[i - 1] : neg_table(ent[i - 1]); break;
            default: ent[i] = ident; break;
        }
    }
    // reference: today's g1_madd30 (normalising, signs applied to the table point)
    G1Xyzz30 ref = g1_from_affine30(ent[0], signs & 1);
    // sign-tracked: the loop of k_accum_affine (modes 0 / 1 / 2)
    int32_t sigma;
    G1Xyzz30 acc = g1_from_table30s(ent[0], signs & 1, sigma);
    check_acc(acc, sigma, 0);
    G1Xyzz30 total_ref = G1Xyzz30::infinity(), total = G1Xyzz30::infinity();
    for (int i = 1; i < CHAIN; i++) {
        const bool neg = (signs >> i) & 1;
        int mode = 0;
        if (L[i].boundary) {
            const G1Xyzz30 part = g1_partial_load30(g1_partial_store30(acc, sigma));
            check_partial(part, i);
            CHECK(same_affine(part, ref), "pattern %d: partial flushed in front of entry %d differs from g1_madd30's", pattern_id, i);
            total = g1_add30(total, part);
            total_ref = g1_add30(total_ref, ref);
            ref = g1_from_affine30(ent[i], neg);
            mode = 1;
        } else {
            ref = g1_madd30(ref, ent[i], neg);
            if (ent[i].is_inf_table()) mode = 2;
            else if (acc.inf) mode = 1;
        }
        if (mode == 0) {
            const int32_t tau = g1_tau30(sigma, neg);
            const Madd30Mid mid = g1_madd30s_phase1(acc, ent[i], tau);
            acc = g1_madd30s_phase2(acc, mid, tau, neg, sigma, [&]() { return ent[i]; });
        } else if (mode == 1) {
            acc = g1_from_table30s(ent[i], neg, sigma);
        }
        check_acc(acc, sigma, i);
        // the special entries right behind a restart took the paths they are there for
        const bool after_restart = i == 1 || L[i - 1].boundary;
        if (after_restart && !L[i].boundary && L[i].kind == INVERSE) CHECK(acc.inf == 1, "pattern %d: entry %d did not give infinity", pattern_id, i);
        if (after_restart && !L[i].boundary && L[i].kind == SAME && L[i - 1].kind != IDENTITY)
            CHECK(acc.inf == 0 && sigma == 1, "pattern %d: entry %d did not take the doubling path", pattern_id, i);
        const G1Xyzz30 now = g1_partial_load30(g1_partial_store30(acc, sigma));
        CHECK(same_affine(now, ref), "pattern %d: accumulator after entry %d (kind %d) differs from g1_madd30's", pattern_id, i, L[i].kind);
        // the one-call form must agree with the three-mode loop
        if (i == CHAIN - 1) {
            int32_t s2;
            G1Xyzz30 a2 = g1_from_table30s(ent[0], signs & 1, s2);
            G1Xyzz30 r2 = g1_from_affine30(ent[0], signs & 1);
            for (int j = 1; j < CHAIN; j++) {
                a2 = g1_madd30s(a2, s2, ent[j], (signs >> j) & 1);
                r2 = g1_madd30(r2, ent[j], (signs >> j) & 1);
            }
            CHECK(same_affine(g1_partial_load30(g1_partial_store30(a2, s2)), r2), "pattern %d: g1_madd30s chain without restarts differs", pattern_id);
        }
    }
    const G1Xyzz30 part = g1_partial_load30(g1_partial_store30(acc, sigma));
    check_partial(part, CHAIN);
    total = g1_add30(total, part);
    total_ref = g1_add30(total_ref, ref);
    CHECK(same_affine(total, total_ref), "pattern %d: sum of the partials differs", pattern_id);
}

int main() {
    test_mul30_sgn();
    std::vector<G1Affine30> pts(CHAIN);
    for (int i = 0; i < CHAIN; i++) pts[i] = g1_affine_to30(random_point());
    std::vector<uint64_t> patterns = {0ull, ~0ull, 0xaaaaaaaaaaaaaaaaull};  // all +, all -, alternating
    for (int i = 0; i < 32; i++) patterns.push_back(rnd());
    for (size_t p = 0; p < patterns.size(); p++) run_chain(pts, patterns[p], (int)p);
    printf("%ld checks, %d failed, %zu sign patterns\n", checks, failures, patterns.size());
    return failures ? 1 : 0;
}
