// Host harness over juicefs_amd/csrc/jfsx_store.h (tests/test_store_contract.py):
// the per-block verdict store_verdict_k applies on the GPU, and the layout of
// jfsx_sblk as the C compiler sees include/jfsx.h, for ctypes.
#include <stddef.h>

#include "../../juicefs_amd/csrc/jfsx_store.h"

extern "C" {
// out: status, out_len, bad_seg, got, expect
void store_verdict(int32_t verify_status, int32_t bad_seg, uint32_t got, uint32_t expect, int32_t comp_status,
                   uint64_t comp_out, uint64_t cap, int64_t *out) {
    const jfsx_store::Verdict v = jfsx_store::verdict(verify_status, bad_seg, got, expect, comp_status, comp_out, cap);
    out[0] = v.status;
    out[1] = (int64_t)v.out_len;
    out[2] = v.bad_seg;
    out[3] = v.got;
    out[4] = v.expect;
}

int store_broken(void) { return jfsx_store::kBroken; }

// out[0] = sizeof(jfsx_sblk), then the offset of every field in declaration order
int sblk_layout(uint64_t *out, int cap) {
    const uint64_t v[] = {sizeof(jfsx_sblk),
                          offsetof(jfsx_sblk, key),     offsetof(jfsx_sblk, nonce),       offsetof(jfsx_sblk, reserved),
                          offsetof(jfsx_sblk, tag),     offsetof(jfsx_sblk, src),         offsetof(jfsx_sblk, len),
                          offsetof(jfsx_sblk, dst),     offsetof(jfsx_sblk, dst_cap),     offsetof(jfsx_sblk, crc),
                          offsetof(jfsx_sblk, hdr),     offsetof(jfsx_sblk, hdr_len),     offsetof(jfsx_sblk, obj_crc),
                          offsetof(jfsx_sblk, out_len), offsetof(jfsx_sblk, status),      offsetof(jfsx_sblk, crc_bad_seg),
                          offsetof(jfsx_sblk, crc_got), offsetof(jfsx_sblk, crc_expect)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}
}
