// Host harness over juicefs_amd/csrc/jfsx_objload.h
// (tests/test_load_objects_contract.py): the per-block verdict obj_verdict_k
// applies on the GPU, the checksum fold of obj_fold_k run as 64 emulated lanes,
// and the layout of jfsx_oblk as the C compiler sees include/jfsx.h.
#include <stddef.h>

#include "../../juicefs_amd/csrc/jfsx_objload.h"

extern "C" {
// out: status, out_len
void object_verdict(int crc_ct, int crc_bad, int cipher, uint32_t flags, int32_t key_len, int32_t open_status,
                    int32_t dec_status, uint64_t dec_out, uint64_t len, int64_t *out) {
    const jfsx_load::Verdict v = jfsx_obj::object_verdict(crc_ct != 0, crc_bad != 0, cipher != 0, flags, key_len,
                                                          open_status, dec_status, dec_out, len);
    out[0] = v.status;
    out[1] = (int64_t)v.out_len;
}

int32_t reported_key_len(uint32_t flags, int32_t unwrapped) { return jfsx_obj::reported_key_len(flags, unwrapped); }

void obj_flags(uint32_t *out) {
    out[0] = jfsx_obj::kHdrBad;
    out[1] = jfsx_obj::kKeyBad;
    out[2] = jfsx_obj::kNonceBad;
}

// the fold as obj_fold_k runs it: every lane's share, the XOR over the wave,
// lane 0's finish.  x8pow[k] = x^(8 * 2^k) is built by squaring from x^8.
uint32_t obj_fold(const uint8_t *segs, uint64_t clen, uint32_t tail, uint32_t crc_hdr, uint32_t crc_tag) {
    uint32_t x8pow[32];
    x8pow[0] = 0x00800000u;
    for (int k = 1; k < 32; k++) x8pow[k] = jfsx_obj::mulmod(x8pow[k - 1], x8pow[k - 1]);
    uint32_t lanes = 0;
    for (uint32_t lane = 0; lane < (uint32_t)jfsx_obj::kLanes; lane++)
        lanes ^= jfsx_obj::fold_lane(lane, segs, clen, tail, x8pow);
    return jfsx_obj::fold_finish(lanes, crc_hdr, crc_tag, clen, tail, x8pow);
}

// out[0] = sizeof(jfsx_oblk), then the offset of every field in declaration order
int oblk_layout(uint64_t *out, int cap) {
    const uint64_t v[] = {sizeof(jfsx_oblk),
                          offsetof(jfsx_oblk, hdr),        offsetof(jfsx_oblk, hdr_len), offsetof(jfsx_oblk, reserved),
                          offsetof(jfsx_oblk, tag),        offsetof(jfsx_oblk, src),     offsetof(jfsx_oblk, src_len),
                          offsetof(jfsx_oblk, dst),        offsetof(jfsx_oblk, len),     offsetof(jfsx_oblk, crc),
                          offsetof(jfsx_oblk, expect_crc), offsetof(jfsx_oblk, obj_crc), offsetof(jfsx_oblk, out_len),
                          offsetof(jfsx_oblk, status),     offsetof(jfsx_oblk, codec_info),
                          offsetof(jfsx_oblk, key_len),    offsetof(jfsx_oblk, reserved2)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}

int obj_constants(int *out) {
    out[0] = JFSX_CODEC_NONE;
    out[1] = JFSX_EKEY;
    out[2] = JFSX_EHEADER;
    out[3] = JFSX_ABI_VERSION;
    return 4;
}
}
