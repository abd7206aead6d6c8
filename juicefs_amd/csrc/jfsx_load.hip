// jfsx_load.hip -- the device-side chaining of jfsx_load_batch on gfx950: the
// read miss of a compressed volume (cachedStore.load,
// pkg/chunk/cached_store.go:673-748: Decrypt, Decompress into the page,
// bcache.cache -> checksum()) as one stream of kernels with no host round trip
// between the stages.
//
//   enqueue_aead (Open, CRC_NONE)      BlkOut[n] stays in device memory
//   load_gate_k                        ZDev[n] from the block records and BlkOut
//   lz4 / zstd decoder                 ZOut[n]
//   crc_segments_k + crc_finalize_k    checksum() of every page
//   load_verdict_k                     {status, out_len, codec_info} per block
//   load_wipe_k                        zero page and CRC array of every failed block
//
// The gate is what keeps unauthenticated bytes away from the decoders: a block
// whose tag failed gets the descriptor {src = null, dst = null, len = 0,
// cap = 0}.  With both fields zero every decoder returns before it forms an
// address from src or dst:
//   lz4_decompress_k       cap == 0 takes `bad = !(n == 1 && ld8(src) == 0)`,
//                          which short-circuits on n == 0; the ring flush is
//                          skipped when bad (jfsx_lz4.hip)
//   zstd_decompress_par_k  scan() returns kFallback on insize < 9 before its
//                          first in8() (jfsx_zstd2.h), so the block goes to
//   zstd_fallback_k /      jzd::decompress: `while (n - p >= 5)` does not run
//   zstd_decompress_k      and `p != n` is false: it returns 0 (jfsx_zstd.h)
// What such a block's ZOut then says is ignored: the verdict looks at Open's
// status first (jfsx_load.h).
#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#include "jfsx_load.h"

namespace jfsx {

namespace {

constexpr int kLoadThreads = 256;

// One thread per block.  ZOut is initialised too: the LZ4 and the serial zstd
// kernels leave ZOut.fallback unwritten.
__global__ __launch_bounds__(kLoadThreads) void load_gate_k(int n, const LoadBlk *__restrict__ lb,
                                                            const BlkOut *__restrict__ opened, ZDev *__restrict__ z,
                                                            ZOut *__restrict__ zo) {
    const int i = blockIdx.x * kLoadThreads + threadIdx.x;
    if (i >= n) return;
    const LoadBlk b = lb[i];
    const bool ok = !opened || opened[i].status == JFSX_OK;
    ZDev d;
    d.src = ok ? b.img : nullptr;
    d.dst = ok ? b.dst : nullptr;
    d.len = ok ? b.src_len : 0;
    d.cap = ok ? b.len : 0;
    z[i] = d;
    ZOut o;
    o.out_len = 0;
    o.status = JFSX_EFORMAT;
    o.fallback = 0;
    zo[i] = o;
}

__global__ __launch_bounds__(kLoadThreads) void load_verdict_k(int n, const LoadBlk *__restrict__ lb,
                                                               const BlkOut *__restrict__ opened,
                                                               const ZOut *__restrict__ zo, int use_fallback,
                                                               LoadRes *__restrict__ res) {
    const int i = blockIdx.x * kLoadThreads + threadIdx.x;
    if (i >= n) return;
    const int32_t ost = opened ? opened[i].status : JFSX_OK;
    const ZOut o = zo[i];
    const jfsx_load::Verdict v = jfsx_load::verdict(ost, o.status, o.out_len, lb[i].len);
    LoadRes r;
    r.out_len = v.out_len;
    r.status = v.status;
    r.codec_info = use_fallback && ost == JFSX_OK ? o.fallback : 0;
    res[i] = r;
}

// [p, p + len) to zero by the whole grid: bytes up to the first 16-byte
// boundary, 16-byte stores, then the bytes after the last boundary.  Nothing
// outside the range is written.
__device__ __forceinline__ void wipe_range(uint8_t *p, uint64_t len, uint64_t gtid, uint64_t gsize) {
    const uint64_t to16 = (16 - ((uintptr_t)p & 15)) & 15;
    const uint64_t head = to16 < len ? to16 : len;
    const uint64_t units = (len - head) >> 4;
    const uint64_t tail = (len - head) & 15;
    if (gtid < head) p[gtid] = 0;
    uint4 *q = reinterpret_cast<uint4 *>(p + head);
    for (uint64_t u = gtid; u < units; u += gsize) q[u] = make_uint4(0, 0, 0, 0);
    if (gtid < tail) p[head + (units << 4) + gtid] = 0;
}

// Every workgroup walks the blocks; the page and the CRC array of one that is
// not OK are zeroed by all of them together (a plain streaming store: no LDS).
__global__ __launch_bounds__(kLoadThreads) void load_wipe_k(int n, const LoadBlk *__restrict__ lb,
                                                            const LoadRes *__restrict__ res, int crc_gen) {
    const uint64_t gtid = (uint64_t)blockIdx.x * kLoadThreads + threadIdx.x;
    const uint64_t gsize = (uint64_t)gridDim.x * kLoadThreads;
    for (int i = 0; i < n; i++) {
        if (res[i].status == JFSX_OK) continue;
        const LoadBlk b = lb[i];
        wipe_range(b.dst, b.len, gtid, gsize);
        if (crc_gen) wipe_range(b.crc, 4 * (b.len ? (b.len + kSeg - 1) / kSeg : 1), gtid, gsize);
    }
}

}  // namespace

void launch_load_gate(hipStream_t s, int n, const LoadBlk *lb, const BlkOut *opened, ZDev *z, ZOut *zo) {
    if (n > 0)
        hipLaunchKernelGGL(load_gate_k, dim3((n + kLoadThreads - 1) / kLoadThreads), dim3(kLoadThreads), 0, s, n, lb,
                           opened, z, zo);
}

void launch_load_finish(hipStream_t s, int n, int wipe_groups, const LoadBlk *lb, const BlkOut *opened,
                        const ZOut *zo, bool use_fallback, bool crc_gen, LoadRes *res) {
    if (n <= 0) return;
    hipLaunchKernelGGL(load_verdict_k, dim3((n + kLoadThreads - 1) / kLoadThreads), dim3(kLoadThreads), 0, s, n, lb,
                       opened, zo, use_fallback ? 1 : 0, res);
    hipLaunchKernelGGL(load_wipe_k, dim3(wipe_groups < 1 ? 1 : wipe_groups), dim3(kLoadThreads), 0, s, n, lb, res,
                       crc_gen ? 1 : 0);
}

void launch_load_wipe(hipStream_t s, int n, int wipe_groups, const LoadBlk *lb, const LoadRes *res, bool crc_gen) {
    if (n > 0)
        hipLaunchKernelGGL(load_wipe_k, dim3(wipe_groups < 1 ? 1 : wipe_groups), dim3(kLoadThreads), 0, s, n, lb, res,
                           crc_gen ? 1 : 0);
}

}  // namespace jfsx
