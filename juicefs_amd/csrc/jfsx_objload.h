// jfsx_objload.h -- the arithmetic of jfsx_load_objects that both sides run:
// the fold of an object's 32 KiB segment CRCs into the object-store checksum
// (obj_fold_k, jfsx_objload.hip) and the per-block verdict with its gate rule
// (obj_gate_k / obj_verdict_k).  The host build
// (tests/harness/objload_host.cpp) pins both without a GPU.
//
// The checksum is generateChecksum's CRC32C of hdr || C || tag
// (pkg/object/checksum.go:31-53).  CRC32C values as crc32.Update returns them
// compose linearly: crc(A || B) = x^(8 |B|) * crc(A) + crc(B) in GF(2)[x]/P,
// so with e_j the end of segment j and t the tag length
//   obj = x^(8 (|C| + t)) * crc(hdr) + sum_j x^(8 (|C| - e_j + t)) * crc(seg_j) + crc(tag)
// Lane l of a wave takes the segments j = l, l + 64, ...; the lanes' sums are
// XOR-reduced (wave_xor on the device, a loop over 64 emulated lanes in the
// host harness) and fold_finish adds the header and tag terms.
#pragma once
#include <stdint.h>

#include "jfsx_load.h"

namespace jfsx_obj {

constexpr uint32_t kPoly = 0x82F63B78u;  // reflected Castagnoli; bit 31 is the coefficient of x^0
constexpr uint64_t kSeg = 32768;
constexpr int kLanes = 64;

// what the host found in a block's header before anything ran (ObjBlk.flags)
constexpr uint32_t kHdrBad = 1;    // rule 2: hdr_len < 3 or != 3 + klen + nlen
constexpr uint32_t kKeyBad = 2;    // rule 3: klen == 0 or klen > k, the modulus length (rsa.DecryptOAEP's size check)
constexpr uint32_t kNonceBad = 4;  // rule 4: nlen != 12 (aead.Open's nonce size check)

// crc_mulmod / crc_xpow8 of jfsx_internal.h, for both sides
JFSX_HD uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8n) mod P from x8pow[k] = x^(8 * 2^k), k < 32 (the context's crcx + 64)
JFSX_HD uint32_t xpow8(uint64_t n, const uint32_t *x8pow) {
    uint32_t r = 0x80000000u;
    for (int k = 0; n; k++, n >>= 1)
        if (n & 1) r = mulmod(x8pow[k], r);
    return r;
}

JFSX_HD uint32_t be32(const uint8_t *p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// lane's share of the sum over the segments: segs = the big-endian segment
// CRCs of C (ceil(clen / 32K) words; none for an empty C), tail = bytes that
// follow C in the object (16 with a cipher, 0 without)
JFSX_HD uint32_t fold_lane(uint32_t lane, const uint8_t *segs, uint64_t clen, uint32_t tail, const uint32_t *x8pow) {
    const uint64_t nseg = (clen + kSeg - 1) / kSeg;
    uint32_t v = 0;
    for (uint64_t j = lane; j < nseg; j += kLanes) {
        const uint64_t end = (j + 1) * kSeg < clen ? (j + 1) * kSeg : clen;
        v ^= mulmod(xpow8(clen - end + tail, x8pow), be32(segs + 4 * j));
    }
    return v;
}

// lanes = XOR of fold_lane over the 64 lanes; crc_hdr / crc_tag =
// crc32.Update(0, ...) of the header and the tag (0 for an absent one)
JFSX_HD uint32_t fold_finish(uint32_t lanes, uint32_t crc_hdr, uint32_t crc_tag, uint64_t clen, uint32_t tail,
                             const uint32_t *x8pow) {
    return mulmod(xpow8(clen + tail, x8pow), crc_hdr) ^ lanes ^ crc_tag;
}

// The rule of rules 1-4 that stops a block, JFSX_OK if none does.  crc_ct /
// cipher: what the batch was called with; crc_bad: obj_crc != expect_crc;
// flags: kHdrBad | kKeyBad | kNonceBad; key_len: the unwrap's result;
// open_status: Open's per-block status.
JFSX_HD int32_t early_status(bool crc_ct, bool crc_bad, bool cipher, uint32_t flags, int32_t key_len,
                             int32_t open_status) {
    if (crc_ct && crc_bad) return JFSX_ECRC;
    if (!cipher) return JFSX_OK;
    if (flags & kHdrBad) return JFSX_EHEADER;
    if ((flags & kKeyBad) || key_len != 32) return JFSX_EKEY;
    if ((flags & kNonceBad) || open_status != JFSX_OK) return JFSX_ETAG;
    return JFSX_OK;
}

// key_len as the record reports it: -1 where the size check of the unwrap
// fails, 0 where the header names no key
JFSX_HD int32_t reported_key_len(uint32_t flags, int32_t unwrapped) {
    return (flags & kHdrBad) ? 0 : (flags & kKeyBad) ? -1 : unwrapped;
}

// The verdict of jfsx_load_objects: rules 1-4, then jfsx_load_batch's rows
// (jfsx_load::verdict) unchanged.  Without a codec pass dec_status = JFSX_OK
// and dec_out = len.
JFSX_HD jfsx_load::Verdict object_verdict(bool crc_ct, bool crc_bad, bool cipher, uint32_t flags, int32_t key_len,
                                          int32_t open_status, int32_t dec_status, uint64_t dec_out, uint64_t len) {
    const int32_t early = early_status(crc_ct, crc_bad, cipher, flags, key_len, open_status);
    if (early != JFSX_OK) {
        jfsx_load::Verdict v;
        v.status = early;
        v.out_len = 0;
        return v;
    }
    return jfsx_load::verdict(JFSX_OK, dec_status, dec_out, len);
}

}  // namespace jfsx_obj
