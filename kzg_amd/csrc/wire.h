// wire.h -- the first byte and the big-endian coordinates of the zcash formats (include/kzg_mi355x.h, "Wire decoding"): what
// k_decode_points (srs.hip, G1) and k_g2_decode (pairing.hip, G2) share.  One byte string per group element: a flag bit that has
// no meaning in a format, or a payload behind the infinity flag, is a malformed encoding, not something to mask away --
// oracle/decode.py is the reference and tests/test_gpu_decode.py holds both kernels against it.
#pragma once
#include "field.h"

namespace kzg {

// bits 7 / 6 / 5 of byte 0: compressed, infinity, y is the lexicographically larger root
struct WireFlags {
    bool compressed, infinity, sign;
};

KZG_HD WireFlags wire_flags(const uint8_t *p) { return WireFlags{(p[0] & 0x80) != 0, (p[0] & 0x40) != 0, (p[0] & 0x20) != 0}; }

// every bit of the `len`-byte encoding behind the three flags is zero
KZG_HD bool wire_rest_is_zero(const uint8_t *p, int len) {
    uint32_t acc = p[0] & 0x1fu;
    for (int i = 1; i < len; i++) acc |= p[i];
    return acc == 0;
}

// The flags of a `len`-byte encoding in a format that is compressed or not.  False: malformed -- the compression bit does not
// match the format, the infinity flag comes with the sign flag or with any other nonzero bit, or an uncompressed point carries
// the sign flag.  True: *infinity says whether this is the identity (nothing else is left to read then), *sign is the flag of a
// compressed finite point.
KZG_HD bool wire_header(const uint8_t *p, int len, bool compressed_format, bool *infinity, bool *sign) {
    const WireFlags f = wire_flags(p);
    *infinity = f.infinity;
    *sign = f.sign;
    if (f.compressed != compressed_format) return false;
    if (f.infinity) return !f.sign && wire_rest_is_zero(p, len);
    return compressed_format || !f.sign;
}

// 48 big-endian bytes -> limbs as they are (the caller checks < q); mask_flags: without the three flag bits of byte 0
KZG_HD Fq wire_read_be48(const uint8_t *src, bool mask_flags) {
    Fq r = Fq::zero();
    for (int i = 0; i < 48; i++) {
        uint32_t byte = src[47 - i];
        if (mask_flags && i == 47) byte &= 0x1f;
        r.v[i >> 2] |= byte << (8 * (i & 3));
    }
    return r;
}

}  // namespace kzg
