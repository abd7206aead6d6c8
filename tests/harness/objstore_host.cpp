// Host harness over juicefs_amd/csrc/jfsx_objstore.h
// (tests/test_store_objects_contract.py): the frame sobj_frame_k writes around
// C and the checksum it folds, run as 64 emulated lanes, and the layout of
// jfsx_soblk as the C compiler sees include/jfsx.h.  Built as a shared library
// for the test and, with its main, as a stand-alone program that runs the same
// cases against a bit-by-bit CRC32C of its own (the sanitizer build).
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../juicefs_amd/csrc/jfsx_objstore.h"

namespace {

struct X8 {
    uint32_t v[32];
    X8() {
        v[0] = 0x00800000u;  // x^8
        for (int k = 1; k < 32; k++) v[k] = jfsx_obj::mulmod(v[k - 1], v[k - 1]);
    }
};
const X8 x8;

template <class F>
uint32_t wave(F lane_fn) {
    uint32_t v = 0;
    for (uint32_t lane = 0; lane < (uint32_t)jfsx_obj::kLanes; lane++) v ^= lane_fn(lane);
    return v;
}

}  // namespace

extern "C" {

// the header's and the tag's stores of all 64 lanes into obj (1 mod 16, at
// least 271 + img_len + 16 bytes); wrapped is dword aligned
void sobj_frame(uint8_t *obj, const uint8_t *wrapped, const uint8_t *nonce, const uint8_t *tag, uint64_t img_len) {
    uint32_t nw[3];
    memcpy(nw, nonce, 12);
    for (uint32_t lane = 0; lane < (uint32_t)jfsx_obj::kLanes; lane++)
        jfsx_sobj::frame_store(lane, obj, wrapped, nw, tag, img_len);
}

// crc32.Update(0, p[0, len)) as the lanes compute it
uint32_t sobj_span_crc(const uint8_t *p, uint32_t len) {
    return wave([&](uint32_t lane) { return jfsx_sobj::bytes_lane(lane, p, len, x8.v); });
}

uint32_t sobj_hdr_crc(const uint8_t *wrapped, const uint8_t *nonce) {
    return wave([&](uint32_t lane) { return jfsx_sobj::hdr_lane(lane, wrapped, nonce, x8.v); });
}

// obj_crc as sobj_frame_k folds it: segs = the big-endian segment CRCs of C
uint32_t sobj_object_crc(const uint8_t *wrapped, const uint8_t *nonce, const uint8_t *segs, uint64_t img_len,
                         const uint8_t *tag) {
    const uint32_t h = sobj_hdr_crc(wrapped, nonce);
    const uint32_t t = sobj_span_crc(tag, jfsx_sobj::kTagBytes);
    const uint32_t s = wave(
        [&](uint32_t lane) { return jfsx_obj::fold_lane(lane, segs, img_len, jfsx_sobj::kTagBytes, x8.v); });
    return jfsx_sobj::object_crc(h, s, t, img_len, x8.v);
}

// out[0] = sizeof(jfsx_soblk), then the offset of every field in declaration order
int soblk_layout(uint64_t *out, int cap) {
    const uint64_t v[] = {sizeof(jfsx_soblk),
                          offsetof(jfsx_soblk, key),         offsetof(jfsx_soblk, nonce),
                          offsetof(jfsx_soblk, reserved),    offsetof(jfsx_soblk, seed),
                          offsetof(jfsx_soblk, src),         offsetof(jfsx_soblk, len),
                          offsetof(jfsx_soblk, obj),         offsetof(jfsx_soblk, obj_cap),
                          offsetof(jfsx_soblk, crc),         offsetof(jfsx_soblk, out_len),
                          offsetof(jfsx_soblk, img_len),     offsetof(jfsx_soblk, obj_crc),
                          offsetof(jfsx_soblk, status),      offsetof(jfsx_soblk, crc_bad_seg),
                          offsetof(jfsx_soblk, crc_got),     offsetof(jfsx_soblk, crc_expect),
                          offsetof(jfsx_soblk, reserved2)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}

int sobj_constants(int *out) {
    out[0] = JFSX_OBJ_HDR_BYTES;
    out[1] = JFSX_OBJ_TAG_BYTES;
    out[2] = (int)jfsx_sobj::kHdrBytes;
    out[3] = (int)jfsx_sobj::kTagBytes;
    out[4] = JFSX_ABI_VERSION;
    return 5;
}
}

// ---------------------------------------------------------------------------
// stand-alone: the cases of the test against a CRC32C of the harness's own
// ---------------------------------------------------------------------------
namespace {

uint32_t ref_crc(uint32_t crc, const uint8_t *p, size_t n) {
    crc = ~crc;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ (0x82F63B78u & (0u - (crc & 1u)));
    }
    return ~crc;
}

uint64_t rng_state = 0x0B5E55EDull;
uint8_t next_byte() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint8_t)(rng_state >> 56);
}

int fails = 0;
void expect(bool ok, const char *what, uint64_t arg) {
    if (!ok) {
        fprintf(stderr, "FAIL %s (%llu)\n", what, (unsigned long long)arg);
        fails++;
    }
}

}  // namespace

int main() {
    alignas(16) uint8_t wrapped[256];
    uint8_t nonce[12], tag[16];
    for (uint8_t &b : wrapped) b = next_byte();
    for (uint8_t &b : nonce) b = next_byte();
    for (uint8_t &b : tag) b = next_byte();
    // span CRCs
    std::vector<uint8_t> span(287);
    for (uint8_t &b : span) b = next_byte();
    for (uint32_t len : {0u, 1u, 3u, 4u, 5u, 16u, 271u, 287u})
        expect(sobj_span_crc(span.data(), len) == ref_crc(0, span.data(), len), "span crc", len);
    // frame and fold
    for (uint64_t clen : {(uint64_t)0, (uint64_t)1, (uint64_t)32767, (uint64_t)32768, (uint64_t)32769,
                          (uint64_t)65541, (uint64_t)(1 << 20) + 3, (uint64_t)(4 << 20) - 1}) {
        std::vector<uint8_t> buf(16 + 1 + 271 + clen + 16 + 16, 0xA5);
        uint8_t *base = buf.data() + 1;
        while (((uintptr_t)base & 15) != 1) base++;
        for (uint64_t i = 0; i < clen; i++) base[271 + i] = next_byte();
        sobj_frame(base, wrapped, nonce, tag, clen);
        expect(base[0] == 1 && base[1] == 0 && base[2] == 12, "header start", clen);
        expect(!memcmp(base + 3, wrapped, 256) && !memcmp(base + 259, nonce, 12), "header body", clen);
        expect(!memcmp(base + 271 + clen, tag, 16), "tag", clen);
        expect(base[-1] == 0xA5 && base[271 + clen + 16] == 0xA5, "guards", clen);
        std::vector<uint8_t> segs;
        for (uint64_t o = 0; o < clen; o += jfsx_obj::kSeg) {
            const uint32_t c = ref_crc(0, base + 271 + o, (size_t)(clen - o < jfsx_obj::kSeg ? clen - o : jfsx_obj::kSeg));
            for (int k = 3; k >= 0; k--) segs.push_back((uint8_t)(c >> (8 * k)));
        }
        if (segs.empty()) segs.assign(4, 0);
        expect(sobj_object_crc(wrapped, nonce, segs.data(), clen, tag) == ref_crc(0, base, 271 + clen + 16),
               "object crc", clen);
    }
    expect(sobj_hdr_crc(wrapped, nonce) != 0, "header crc", 0);
    if (fails) return 1;
    printf("objstore_host ok\n");
    return 0;
}
