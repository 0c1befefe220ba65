// Host build of kzg_amd/csrc/glv.h (the GLV scalar multiplication of the FK20 kernels) for tests/test_host_glv.py: the same source
// hipcc compiles for gfx950.
#include <string.h>

#include "../kzg_amd/csrc/glv.h"
using namespace kzg;

static Fq30 beta30() {
    Fq b;
    for (int i = 0; i < 12; i++) b.v[i] = GLV_BETA[i];
    return to30(to_mont(b));
}

extern "C" {
// out = [k]P (affine Montgomery 96 B; k canonical 32 B) through glv_recode + glv_mul (glv = 1) or mul256 (glv = 0)
void hg_g1_mul(const uint32_t *p, const uint32_t *k, int glv, uint32_t *out) {
    G1Affine a;
    memcpy(&a, p, 96);
    G1Xyzz30 P = g1_from_affine30(g1_affine_to30(a), false), tab[G1NTT_TAB];
    uint32_t kk[8];
    memcpy(kk, k, 32);
    G1Xyzz30 r;
    if (glv) {
        GlvTw w = glv_recode(kk);
        r = glv_mul(P, w, tab, 1, beta30());
    } else {
        Fr f;
        memcpy(f.v, k, 32);
        r = mul256(P, f, tab, 1, beta30());
    }
    G1Affine o = g1_to_affine(g1_xyzz_from30(r));
    memcpy(out, &o, 96);
}
// (k1, k2) of the GLV split and the recoded form
void hg_glv_split(const uint32_t *k, uint32_t *k1, uint32_t *k2, uint32_t *rec) {
    uint32_t kk[8];
    memcpy(kk, k, 32);
    glv_split(kk, k1, k2);
    GlvTw w = glv_recode(kk);
    memcpy(rec, &w, sizeof w);
}
}
