// jfsx_objstore.h -- the arithmetic of jfsx_store_objects' frame stage that
// both sides run: the bytes of the object header, the CRC32C of a short span
// spread over the 64 lanes of a wave, and the fold of header, image segment
// CRCs and tag into the object-store checksum (sobj_frame_k,
// jfsx_objstore.hip).  The host build (tests/harness/objstore_host.cpp) pins
// all three without a GPU.
//
// The stored object is dataEncryptor.Encrypt's (pkg/object/encrypt.go:164-194)
//   BE16(k) | 12 | wrapped key (k) | nonce (12) | C | tag (16)
// with k the modulus length of the volume's RSA key (256, or 512 for a
// 4096-bit key: the kbytes argument below), and its checksum generateChecksum's CRC32C of all of it
// (pkg/object/checksum.go:31-53).  The header and the tag exist in device
// memory only (the wrap's output and the Seal's BlkOut), so their CRCs are
// computed there: lane l takes the bytes [l * per, (l + 1) * per) of the span,
// per = ceil(len / 64), runs crc32.Update(0, .) over them bit by bit and lifts
// the value to the span's end with x^(8 * bytes behind it); the XOR of the
// lanes is crc32.Update(0, span), by the composition rule jfsx_objload.h
// states.  fold_lane / fold_finish of jfsx_objload.h do the rest.
#pragma once
#include <stdint.h>

#include "jfsx_objload.h"

namespace jfsx_sobj {

constexpr uint32_t kKeyBytes = 256;  // RSA-2048: the wrapped key
constexpr uint32_t kNonceBytes = 12;
constexpr uint32_t kHdrBytes = 3 + kKeyBytes + kNonceBytes;  // JFSX_OBJ_HDR_BYTES
constexpr uint32_t kTagBytes = 16;                           // JFSX_OBJ_TAG_BYTES
// the header of a key of kbytes: 271, or 527 for RSA-4096
constexpr uint32_t hdr_bytes(uint32_t kbytes) { return 3 + kbytes + kNonceBytes; }

// byte k < hdr_bytes(kbytes) of the header
JFSX_HD uint8_t hdr_byte(uint32_t k, const uint8_t *wrapped, const uint8_t *nonce, uint32_t kbytes = kKeyBytes) {
    if (k < 3) return k == 0 ? (uint8_t)(kbytes >> 8) : k == 1 ? (uint8_t)(kbytes & 255) : (uint8_t)kNonceBytes;
    return k < 3 + kbytes ? wrapped[k - 3] : nonce[k - 3 - kbytes];
}

// lane's stores of the frame around C.  obj is 1 mod 16, so the wrapped key at
// obj + 3 and the nonce at obj + 3 + kbytes (259 or 515) take dword stores (wk
// is dword aligned); the tag lies wherever the image ends and takes byte stores.
JFSX_HD void frame_store(uint32_t lane, uint8_t *obj, const uint8_t *wk, const uint32_t *nonce, const uint8_t *tag,
                         uint64_t img_len, uint32_t kbytes = kKeyBytes) {
    if (lane < 3) obj[lane] = hdr_byte(lane, wk, nullptr, kbytes);
    for (uint32_t w = lane; w < kbytes / 4; w += jfsx_obj::kLanes)
        reinterpret_cast<uint32_t *>(obj + 3)[w] = reinterpret_cast<const uint32_t *>(wk)[w];
    if (lane < kNonceBytes / 4) reinterpret_cast<uint32_t *>(obj + 3 + kbytes)[lane] = nonce[lane];
    if (lane < kTagBytes) obj[hdr_bytes(kbytes) + img_len + lane] = tag[lane];
}

// crc32.Update(crc, one byte), bit by bit
JFSX_HD uint32_t crc_byte(uint32_t crc, uint8_t b) {
    crc = ~crc ^ b;
    for (int i = 0; i < 8; i++) crc = (crc >> 1) ^ (jfsx_obj::kPoly & (0u - (crc & 1u)));
    return ~crc;
}

// lane's share of crc32.Update(0, span): get(k) = byte k of the span, k < len
template <class Get>
JFSX_HD uint32_t span_lane(uint32_t lane, uint32_t len, Get get, const uint32_t *x8pow) {
    const uint32_t per = (len + jfsx_obj::kLanes - 1) / jfsx_obj::kLanes;
    const uint32_t lo = lane * per < len ? lane * per : len;
    const uint32_t hi = lo + per < len ? lo + per : len;
    if (lo == hi) return 0;
    uint32_t v = 0;
    for (uint32_t k = lo; k < hi; k++) v = crc_byte(v, get(k));
    return jfsx_obj::mulmod(jfsx_obj::xpow8(len - hi, x8pow), v);
}

JFSX_HD uint32_t hdr_lane(uint32_t lane, const uint8_t *wrapped, const uint8_t *nonce, const uint32_t *x8pow,
                          uint32_t kbytes = kKeyBytes) {
    return span_lane(lane, hdr_bytes(kbytes), [&](uint32_t k) { return hdr_byte(k, wrapped, nonce, kbytes); }, x8pow);
}

JFSX_HD uint32_t bytes_lane(uint32_t lane, const uint8_t *p, uint32_t len, const uint32_t *x8pow) {
    return span_lane(lane, len, [&](uint32_t k) { return p[k]; }, x8pow);
}

// CRC32C(hdr | C | tag) from the wave's three XOR-reduced sums: the header's
// and the tag's span CRCs and fold_lane over C's segment CRCs
JFSX_HD uint32_t object_crc(uint32_t crc_hdr, uint32_t seg_lanes, uint32_t crc_tag, uint64_t img_len,
                            const uint32_t *x8pow) {
    return jfsx_obj::fold_finish(seg_lanes, crc_hdr, crc_tag, img_len, kTagBytes, x8pow);
}

}  // namespace jfsx_sobj
