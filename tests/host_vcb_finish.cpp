// Stand-alone host build (g++) of kzg_amd/csrc/vcb_finish.h -- the finish of kzg_verify_cosets_batch that runs on the calling thread:
// the Horner over the window sums, P2 + Cagg - Ragg and the pairing product -- so tests/test_host_vcb_finish.py can run it under
// -fsanitize=address,undefined on the CPU and compare it with the python oracle.  Test infrastructure only.
//   host_vcb_finish IN OUT
// IN : 3 x 32 window sums, then Ragg (affine, canonical little-endian 96 B each, the identity all-zero), then hs[0] and hs[l]
//      (affine canonical 192 B each).  OUT: one verdict byte, then P1, P2, Cagg, Ragg (affine canonical 96 B each).
#include <cstdio>
#include <vector>

#include "../kzg_amd/csrc/vcb_finish.h"
using namespace kzg;

static Fq load_fq(const uint8_t *p) {  // canonical little-endian 48 B -> Montgomery
    Fq a;
    memcpy(a.v, p, 48);
    return to_mont(a);
}
static void store_fq(uint8_t *p, const Fq &a) {
    Fq c = from_mont(a);
    memcpy(p, c.v, 48);
}
static Fq2 load_f2(const uint8_t *p) { return Fq2{load_fq(p), load_fq(p + 48)}; }
static G1Xyzz load_g1(const uint8_t *p) { return G1Xyzz::from_affine(G1Affine{load_fq(p), load_fq(p + 48)}); }
static G2Affine load_g2(const uint8_t *p) { return G2Affine{load_f2(p), load_f2(p + 96)}; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const size_t in_bytes = (3 * VCB_W + 1) * 96 + 2 * 192;
    std::vector<uint8_t> in(in_bytes), out(1 + 4 * 96);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), 1, in_bytes, f) != in_bytes) return 3;
    fclose(f);
    std::vector<VcbSums> sums(1);  // on the heap: the sanitizer sees both ends
    for (int s = 0; s < 3; s++)
        for (int w = 0; w < VCB_W; w++) sums[0].win[s][w] = load_g1(in.data() + (size_t)(s * VCB_W + w) * 96);
    sums[0].ragg = load_g1(in.data() + (size_t)3 * VCB_W * 96);
    std::vector<G2Affine> hq(2);
    std::vector<Fq2> lines(2 * 2 * MILLER_LINES);
    for (int j = 0; j < 2; j++) {
        hq[j] = load_g2(in.data() + (size_t)(3 * VCB_W + 1) * 96 + (size_t)j * 192);
        g2_precompute_lines(hq[j], lines.data() + (size_t)j * 2 * MILLER_LINES);
    }
    std::vector<G1Affine> parts(4);
    out[0] = vcb_finish(sums[0], hq.data(), lines.data(), parts.data()) ? 1 : 0;
    for (int i = 0; i < 4; i++) {
        store_fq(out.data() + 1 + 96 * i, parts[i].x);
        store_fq(out.data() + 1 + 96 * i + 48, parts[i].y);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
