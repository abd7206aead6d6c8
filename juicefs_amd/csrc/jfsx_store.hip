// jfsx_store.hip -- the device-side chaining of jfsx_store_batch on gfx950:
// the write side of a compressed volume (uploadStagingFile's re-read through
// cacheFile.ReadAt, pkg/chunk/cached_store.go:944-999; cachedStore.upload's
// Compress, :371-413; store.put's Encrypt and the object store's checksum) as
// two runs of kernels on the context's stream with one small read-back
// between them.
//
// Phase A
//   crc_segments_k + crc_finalize_k    checksum() of every page (GEN), or the
//                                      staged re-read (VERIFY); BlkOut[n] stays
//                                      in device memory
//   store_gate_k                       ZDev[n] from the block records and BlkOut
//   lz4 / zstd compressor              ZOut[n]
//   store_verdict_k                    {status, out_len, bad_seg, got, expect}
//                                      per block, downloaded: wait #1
// Phase B (planned on the host from out_len, over the OK blocks only)
//   gcm / chacha Seal (GEN | CT)       image, tag and the ciphertext segment
//   or crc_segments_k (no cipher)      CRCs the object checksum is folded from
//                                      on the host; downloaded: wait #2
//
// The Seal's tasks and partial slots are planned from the lengths of its
// inputs (plan_batch), and those lengths are what the compressor produced: that
// is the one thing a single pass cannot know, hence the read-back.
//
// The gate is what keeps a page that failed its CRCs away from the compressor
// and the cipher: such a block gets the descriptor {src = null, len = 0,
// dst = 16 bytes of engine scratch of its own, cap = 16}, and it is left out
// of phase B.  With len == 0 neither compressor loads from src:
//   lz4c_block (jfsx_lz4.hip)   `if (n >= kMfLimit + 1) {` skips the parse (the
//                               only loads outside the last literals); the last
//                               literals are `const uint32_t run = n - anchor;`
//                               = 0, `st8(dst + tokpos, run << 4);` and
//                               `wave_copy(dst + op, src + anchor, run, lane);`
//                               -- in wave_copy `if (head > len) head = len;`
//                               makes `if (lane < head)` false, `body = len - i`
//                               is 0, so neither unit loop runs and
//                               `if (lane < body - o)` is false: one token byte
//                               stored, no load
//   compress_object             `if (n == 0) { if (lane == 0) jzc::wr24(dst + op,
//   (jfsx_zstdc.hip)            1); return op + 3; }` right after the frame
//                               header (write_frame_header: 6 bytes for n = 0),
//                               before the table clear and the block loop
//   jzc::compress_frame         `if (n == 0) { wr24(op, 1); return ...; }`, the
//   (jfsx_zstdc.h)              same place
// so the sink receives 1 (LZ4) or 9 (zstd) bytes and src stays null.  What such
// a block's ZOut then says is ignored: the verdict looks at the verify status
// first (jfsx_store.h).
#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#include "jfsx_store.h"

namespace jfsx {

namespace {

constexpr int kStoreThreads = 256;

// One thread per block.  ZOut is initialised: a record the compressor did not
// write must not pass for a length (jfsx_store.h, kBroken).
__global__ __launch_bounds__(kStoreThreads) void store_gate_k(int n, const StoreBlk *__restrict__ sb,
                                                              const BlkOut *__restrict__ verified,
                                                              ZDev *__restrict__ z, ZOut *__restrict__ zo) {
    const int i = blockIdx.x * kStoreThreads + threadIdx.x;
    if (i >= n) return;
    const StoreBlk b = sb[i];
    const bool ok = !verified || verified[i].status == JFSX_OK;
    ZDev d;
    d.src = ok ? b.src : nullptr;
    d.dst = ok ? b.dst : b.sink;
    d.len = ok ? b.len : 0;
    d.cap = ok ? b.cap : kStoreSink;
    z[i] = d;
    ZOut o;
    o.out_len = 0;
    o.status = JFSX_EFORMAT;
    o.fallback = 0;
    zo[i] = o;
}

__global__ __launch_bounds__(kStoreThreads) void store_verdict_k(int n, const StoreBlk *__restrict__ sb,
                                                                 const BlkOut *__restrict__ verified,
                                                                 const ZOut *__restrict__ zo,
                                                                 StoreRes *__restrict__ res) {
    const int i = blockIdx.x * kStoreThreads + threadIdx.x;
    if (i >= n) return;
    BlkOut v;
    v.status = JFSX_OK;
    v.bad_seg = -1;
    v.got = v.expect = 0;
    if (verified) v = verified[i];
    const ZOut o = zo[i];
    const jfsx_store::Verdict r =
        jfsx_store::verdict(v.status, v.bad_seg, v.got, v.expect, o.status, o.out_len, sb[i].cap);
    StoreRes s;
    s.out_len = r.out_len;
    s.status = r.status;
    s.bad_seg = r.bad_seg;
    s.got = r.got;
    s.expect = r.expect;
    res[i] = s;
}

}  // namespace

void launch_store_gate(hipStream_t s, int n, const StoreBlk *sb, const BlkOut *verified, ZDev *z, ZOut *zo) {
    if (n > 0)
        hipLaunchKernelGGL(store_gate_k, dim3((n + kStoreThreads - 1) / kStoreThreads), dim3(kStoreThreads), 0, s, n,
                           sb, verified, z, zo);
}

void launch_store_verdict(hipStream_t s, int n, const StoreBlk *sb, const BlkOut *verified, const ZOut *zo,
                          StoreRes *res) {
    if (n > 0)
        hipLaunchKernelGGL(store_verdict_k, dim3((n + kStoreThreads - 1) / kStoreThreads), dim3(kStoreThreads), 0, s,
                           n, sb, verified, zo, res);
}

}  // namespace jfsx
