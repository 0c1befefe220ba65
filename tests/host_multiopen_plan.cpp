// Stand-alone host build (g++) of kzg_amd/csrc/multiopen_plan.h -- the host-side plan of the two-element multiproof: the claims sorted by
// point, the distinct points and their chunks, r^k, w_k = r^k / (t - z_k) in chunks and W_m -- so tests/test_host_multiopen_plan.py can
// run it under -fsanitize=address,undefined on the CPU and compare it with the python model.  Test infrastructure only.
//   host_multiopen_plan IN OUT
// IN : u32 count, n_polys, d, option, wchunk, has_idx; r, t (canonical little-endian 32 B each); count x z; count x on-domain flag byte;
//      count x u32 index (when has_idx).
// OUT: u32 U, n_off, cap, t_hits_a_point; count x u32 order; (U + 1) x u32 pstart; U x z; count x r^k; count x w_k; n_polys x W_m
//      (scalars canonical little-endian 32 B; w and W are zero when t equals a point).
#include <cstdio>
#include <vector>

#include "../kzg_amd/csrc/multiopen_plan.h"
using namespace kzg;

static Fr load_fr(const uint8_t *p) {
    Fr a;
    memcpy(a.v, p, 32);
    return to_mont(a);
}
static void put_fr(std::vector<uint8_t> &out, const Fr &a) {
    const Fr c = from_mont(a);
    out.insert(out.end(), (const uint8_t *)c.v, (const uint8_t *)c.v + 32);
}
static void put_u32(std::vector<uint8_t> &out, uint32_t x) { out.insert(out.end(), (const uint8_t *)&x, (const uint8_t *)&x + 4); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hdr[6];
    if (fread(hdr, 4, 6, f) != 6) return 3;
    const size_t count = hdr[0], n_polys = hdr[1], d = hdr[2], wchunk = hdr[4] ? hdr[4] : (count ? count : 1);
    std::vector<uint8_t> in(64 + count * 33 + (hdr[5] ? count * 4 : 0));
    if (fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    const Fr r = load_fr(in.data()), t = load_fr(in.data() + 32);
    std::vector<Fr> z(count);  // on the heap: the sanitizer sees both ends
    for (size_t k = 0; k < count; k++) z[k] = load_fr(in.data() + 64 + 32 * k);
    const uint8_t *on_claim = in.data() + 64 + 32 * count;
    std::vector<uint32_t> idx(hdr[5] ? count : 0);
    if (hdr[5] && count) memcpy(idx.data(), in.data() + 64 + 33 * count, count * 4);

    MoPlan plan;
    mo_plan(z.data(), count, r, &plan);
    std::vector<uint8_t> on(plan.points());
    for (size_t u = 0; u < plan.points(); u++) on[u] = on_claim[plan.order[plan.pstart[u]]];
    std::vector<uint32_t> src;
    const size_t n_off = mo_off_domain_first(&plan, on.data(), &src);
    const size_t cap = mo_chunk_points(d, (int)hdr[3]);
    std::vector<Fr> w(count), W(n_polys);
    for (auto &x : W) x = Fr::zero();
    for (auto &x : w) x = Fr::zero();
    Fr rk = Fr::one();
    uint32_t hit = 0;
    for (size_t k0 = 0; k0 < count && !hit; k0 += wchunk) {
        const size_t B = std::min(wchunk, count - k0);
        if (!mo_weights(z.data() + k0, B, r, t, &rk, w.data() + k0)) hit = 1;
        else mo_poly_weights(w.data() + k0, hdr[5] ? idx.data() : nullptr, k0, B, W.data());
    }
    if (hit) {
        for (auto &x : W) x = Fr::zero();
        for (auto &x : w) x = Fr::zero();
    }
    std::vector<uint8_t> out;
    put_u32(out, (uint32_t)plan.points());
    put_u32(out, (uint32_t)n_off);
    put_u32(out, (uint32_t)cap);
    put_u32(out, hit);
    for (uint32_t x : plan.order) put_u32(out, x);
    for (uint32_t x : plan.pstart) put_u32(out, x);
    for (const Fr &x : plan.z) put_fr(out, x);
    for (const Fr &x : plan.rk) put_fr(out, x);
    for (const Fr &x : w) put_fr(out, x);
    for (const Fr &x : W) put_fr(out, x);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 4;
    fclose(f);
    return 0;
}
