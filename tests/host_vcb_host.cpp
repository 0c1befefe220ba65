// Stand-alone host build (g++) of kzg_amd/csrc/vcb_host.h -- the counting sort of a chunk's openings by commitment and the weight walk
// of kzg_verify_fold -- so tests/test_host_vcb_host.py can run it under -fsanitize=address,undefined on the CPU and compare it with a
// brute-force grouping and with r^g gamma_g^i computed directly.  Test infrastructure only.
//   host_vcb_host IN OUT
// IN : u32 mode, then
//      mode 0 (the sort): u32 n_commitments, B0, chunks; per chunk u32 B and B x u32 commitment index.  One VcbLists serves all chunks.
//      mode 1 (the walk): u32 t, groups, chunk; r, then groups x gamma (canonical little-endian 32 B each).  One FoldWalk serves all chunks.
// OUT: mode 0: per chunk u32 lists, u32 non-zero entries of cnt after the build; lists x which; (lists + 1) x start; B x order
//      mode 1: t x groups weights (canonical little-endian 32 B), chunk after chunk
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../kzg_amd/csrc/vcb_host.h"
using namespace kzg;

static bool get_u32(FILE *f, uint32_t *x, size_t n) { return fread(x, 4, n, f) == n; }
static void put_u32(std::vector<uint8_t> &out, uint32_t x) { out.insert(out.end(), (const uint8_t *)&x, (const uint8_t *)&x + 4); }
static bool get_fr(FILE *f, Fr *a) {
    Fr c;
    if (fread(c.v, 32, 1, f) != 1) return false;
    *a = to_mont(c);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hdr[4];
    if (!get_u32(f, hdr, 4)) return 3;
    std::vector<uint8_t> out;
    if (hdr[0] == 0) {
        const size_t n_commitments = hdr[1], B0 = hdr[2];
        VcbLists lists;
        if (!lists.reserve(n_commitments, B0)) return 5;
        for (uint32_t c = 0; c < hdr[3]; c++) {
            uint32_t B;
            if (!get_u32(f, &B, 1) || B > B0) return 3;
            std::vector<uint32_t> cm(B);  // on the heap, of the chunk's size: the sanitizer sees both ends
            if (B && !get_u32(f, cm.data(), B)) return 3;
            const size_t n = lists.build(cm.data(), B);
            put_u32(out, (uint32_t)n);
            put_u32(out, (uint32_t)std::count_if(lists.cnt.begin(), lists.cnt.end(), [](uint32_t x) { return x != 0; }));
            for (size_t g = 0; g < n; g++) put_u32(out, lists.which[g]);
            for (size_t g = 0; g <= n; g++) put_u32(out, lists.start[g]);
            for (size_t k = 0; k < B; k++) put_u32(out, lists.order[k]);
        }
    } else {
        const size_t t = hdr[1], groups = hdr[2], chunk = hdr[3], count = t * groups;
        Fr r;
        if (!get_fr(f, &r)) return 3;
        std::vector<Fr> gm(groups);
        for (size_t g = 0; g < groups; g++)
            if (!get_fr(f, &gm[g])) return 3;
        FoldWalk walk;
        for (size_t k0 = 0; k0 < count; k0 += chunk) {
            const size_t B = std::min(chunk, count - k0);
            std::vector<Fr> rho(B);
            fold_weights(&walk, t, r, gm.data(), B, rho.data());
            for (const Fr &x : rho) {
                const Fr c = from_mont(x);
                out.insert(out.end(), (const uint8_t *)c.v, (const uint8_t *)c.v + 32);
            }
        }
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
