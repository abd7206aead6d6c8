// jfsx_store.h -- the per-block verdict of jfsx_store_batch (verify ->
// compress -> Seal -> checksum in one call), shared by the device
// (store_verdict_k, jfsx_store.hip) and the host
// (tests/harness/store_verdict_host.cpp pins it without a GPU).
//
// uploadStagingFile (pkg/chunk/cached_store.go:944-999) re-reads the staged
// page through cacheFile.ReadAt, which fails the read at the first segment
// whose CRC does not match (disk_cache.go:1315-1327); only a page that was
// read goes on to cachedStore.upload's Compress and store.put's Encrypt.  The
// merge below keeps that order: a failed verify wins, and nothing of what the
// compressor reported for such a block (it was given an empty input and a
// private sink) reaches the caller.
#pragma once
#include <stdint.h>

#include "../../include/jfsx.h"

#ifndef JFSX_HD
#define JFSX_HD static inline
#endif

namespace jfsx_store {

// not a per-block status of the ABI: the compressor of a block that passed the
// gate left no usable length (its record was not written, or is outside
// [1, cap]).  The host turns it into the batch-level JFSX_EIO before any Seal
// is planned from such a length.
constexpr int32_t kBroken = -1;

struct Verdict {
    int32_t status;    // JFSX_OK / JFSX_ECRC / kBroken
    uint64_t out_len;  // bytes of the compressed block, 0 unless JFSX_OK
    int32_t bad_seg;   // JFSX_ECRC: first failing segment, else -1
    uint32_t got, expect;
};

// verify_status, bad_seg, got, expect: the page CRC stage's BlkOut (JFSX_OK,
// -1, 0, 0 unless the mode is JFSX_CRC_VERIFY); comp_status / comp_out: the
// compressor's ZOut; cap: the capacity the compressor was given (the codec's
// bound of the page length).  An LZ4 block and a zstd frame are never empty
// (1 and 9 bytes for an empty page), so comp_out == 0 is never a valid length.
//   page fails its CRCs               JFSX_ECRC  0         bad_seg, got, expect
//   compressor record unusable        kBroken    0         -1, 0, 0
//   otherwise                         JFSX_OK    comp_out  -1, 0, 0
JFSX_HD Verdict verdict(int32_t verify_status, int32_t bad_seg, uint32_t got, uint32_t expect, int32_t comp_status,
                        uint64_t comp_out, uint64_t cap) {
    Verdict v;
    v.out_len = 0;
    v.bad_seg = -1;
    v.got = v.expect = 0;
    if (verify_status != JFSX_OK) {
        v.status = JFSX_ECRC;
        v.bad_seg = bad_seg;
        v.got = got;
        v.expect = expect;
    } else if (comp_status != JFSX_OK || comp_out == 0 || comp_out > cap) {
        v.status = kBroken;
    } else {
        v.status = JFSX_OK;
        v.out_len = comp_out;
    }
    return v;
}

}  // namespace jfsx_store
