// Host harness over juicefs_amd/csrc/jfsx_load.h (tests/test_load_verdict.py):
// the per-block verdict load_verdict_k applies on the GPU, and the layout of
// jfsx_lblk as the C compiler sees include/jfsx.h, for ctypes.
#include <stddef.h>

#include "../../juicefs_amd/csrc/jfsx_load.h"

extern "C" {
void load_verdict(int32_t open_status, int32_t dec_status, uint64_t dec_out, uint64_t len, int32_t *status,
                  uint64_t *out_len) {
    const jfsx_load::Verdict v = jfsx_load::verdict(open_status, dec_status, dec_out, len);
    *status = v.status;
    *out_len = v.out_len;
}

// out[0] = sizeof(jfsx_lblk), then the offset of every field in declaration order
int lblk_layout(uint64_t *out, int cap) {
    const uint64_t v[] = {sizeof(jfsx_lblk),         offsetof(jfsx_lblk, key),      offsetof(jfsx_lblk, nonce),
                          offsetof(jfsx_lblk, reserved), offsetof(jfsx_lblk, tag),  offsetof(jfsx_lblk, src),
                          offsetof(jfsx_lblk, src_len),  offsetof(jfsx_lblk, dst),  offsetof(jfsx_lblk, len),
                          offsetof(jfsx_lblk, crc),      offsetof(jfsx_lblk, out_len), offsetof(jfsx_lblk, status),
                          offsetof(jfsx_lblk, codec_info)};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}

// the constants the binding mirrors
int load_constants(int *out) {
    out[0] = JFSX_CIPHER_NONE;
    out[1] = JFSX_CODEC_LZ4;
    out[2] = JFSX_CODEC_ZSTD;
    out[3] = JFSX_ESHORT;
    return 4;
}
}
