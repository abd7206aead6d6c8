// jfsx_load.h -- the per-block verdict of jfsx_load_batch (Open -> decompress
// -> checksum in one call), shared by the device (load_verdict_k,
// jfsx_load.hip) and the host (tests/harness/load_verdict_host.cpp pins it
// without a GPU).
//
// cachedStore.load (pkg/chunk/cached_store.go:673-748) fails a block at the
// first stage that fails: Decrypt (encrypt.go:196-216), then Decompress
// (:738), then the "read %s fully: %s (%d < %d)" length check (:740-743).
// The merge below keeps that order: the first rule that applies wins.
#pragma once
#include <stdint.h>

#include "../../include/jfsx.h"

#ifndef JFSX_HD
#define JFSX_HD static inline
#endif

namespace jfsx_load {

struct Verdict {
    int32_t status;    // JFSX_OK / JFSX_ETAG / JFSX_EFORMAT / JFSX_EDSTSIZE / JFSX_ESHORT
    uint64_t out_len;  // bytes the decoder produced, 0 unless it ran and accepted the image
};

// open_status: Open's per-block status (JFSX_OK with JFSX_CIPHER_NONE);
// dec_status / dec_out: the decoder's ZOut (meaningless when the tag failed:
// the decoder was then given an empty descriptor); len: the page length.
//   tag does not verify          JFSX_ETAG                      0
//   decoder rejects the image    its status (EFORMAT, EDSTSIZE) 0
//   decoder produced n < len     JFSX_ESHORT                    n
//   otherwise                    JFSX_OK                        len
JFSX_HD Verdict verdict(int32_t open_status, int32_t dec_status, uint64_t dec_out, uint64_t len) {
    Verdict v;
    if (open_status != JFSX_OK) {
        v.status = JFSX_ETAG;
        v.out_len = 0;
    } else if (dec_status != JFSX_OK) {
        v.status = dec_status;
        v.out_len = 0;
    } else if (dec_out < len) {
        v.status = JFSX_ESHORT;
        v.out_len = dec_out;
    } else {
        v.status = JFSX_OK;
        v.out_len = len;
    }
    return v;
}

}  // namespace jfsx_load
