// jfsx_objload.hip -- the device-side glue of jfsx_load_objects on gfx950: the
// object store's checksum verify and the data-key unwrap in front of
// jfsx_load_batch's chain (jfsx_load.hip), so that the read miss is one stream
// of kernels from the stored object to the page.
//
//   crc_segments_k (enqueue_crc)       segment CRCs of every image, before Open
//                                      overwrites a host batch's image in place
//   rsa_pair_k + rsa_finish_k          the wrapped keys' messages, device memory
//   obj_fold_k                         obj_crc and obj_crc != expect_crc per object
//   enqueue_aead (Open), with          KeyIn[i].key from the unwrap's message
//     obj_keys_k before its keysetup   slot, which is zeroed; key_len recorded
//   obj_gate_k                         ZDev[n]: as load_gate_k, closed also on
//                                      ECRC / EHEADER / EKEY (rules 1-4)
//   lz4 / zstd decoder, page CRCs      as jfsx_load_batch
//   obj_verdict_k, load_wipe_k         jfsx_obj::object_verdict; failed pages zeroed
//
// The unwrapped key exists in two places only, both device memory of the
// engine: the RSA workspace's message slot between rsa_finish_k and
// obj_keys_k, and the AEAD workspace's KeyIn / schedule as for every Open.
#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#include "jfsx_objload.h"

namespace jfsx {

namespace {

constexpr int kObjThreads = 256;

// One wave per object.
__global__ __launch_bounds__(64) void obj_fold_k(int n, const ObjBlk *__restrict__ ob, uint32_t tail,
                                                 const uint32_t *__restrict__ x8pow, ObjState *__restrict__ st) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const ObjBlk b = ob[i];
    const uint32_t lanes = wave_xor(jfsx_obj::fold_lane(threadIdx.x, b.segs, b.clen, tail, x8pow));
    if (threadIdx.x == 0) {
        const uint32_t crc = jfsx_obj::fold_finish(lanes, b.crc_hdr, b.crc_tag, b.clen, tail, x8pow);
        st[i].obj_crc = crc;
        st[i].crc_bad = crc != b.expect;
    }
}

// One thread per object.  The branch is on the block's outcome (which the
// record reports), not on key bytes.
__global__ __launch_bounds__(kObjThreads) void obj_keys_k(int n, const ObjBlk *__restrict__ ob,
                                                          ObjState *__restrict__ st, uint8_t *__restrict__ em,
                                                          int em_slot, const int32_t *__restrict__ len,
                                                          KeyIn *__restrict__ keys) {
    const int i = blockIdx.x * kObjThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t flags = ob[i].flags;
    const int32_t kl = jfsx_obj::reported_key_len(flags, len[i]);
    // rules 1-3 with Open's status left out: what is known before Open runs
    const bool ok = jfsx_obj::early_status(true, st[i].crc_bad != 0, true, flags & ~jfsx_obj::kNonceBad, kl,
                                           JFSX_OK) == JFSX_OK;
    // em_slot = the unwrap's message slot per object, the modulus length (256 or 512): 256-byte aligned
    uint32_t *slot = reinterpret_cast<uint32_t *>(em + (size_t)em_slot * i);
#pragma unroll
    for (int w = 0; w < 8; w++) keys[i].key[w] = ok ? slot[w] : 0u;
    uint4 *q = reinterpret_cast<uint4 *>(slot);
    for (int w = 0; w < em_slot / 16; w++) q[w] = make_uint4(0, 0, 0, 0);
    st[i].key_len = kl;
}

__device__ __forceinline__ int32_t early_of(int i, const ObjBlk *ob, const ObjState *st, const BlkOut *opened,
                                            int crc_ct) {
    const ObjState s = st[i];
    return jfsx_obj::early_status(crc_ct != 0, s.crc_bad != 0, opened != nullptr, ob[i].flags, s.key_len,
                                  opened ? opened[i].status : JFSX_OK);
}

// load_gate_k with rules 1-4: one thread per block
__global__ __launch_bounds__(kObjThreads) void obj_gate_k(int n, const LoadBlk *__restrict__ lb,
                                                          const ObjBlk *__restrict__ ob,
                                                          const ObjState *__restrict__ st,
                                                          const BlkOut *__restrict__ opened, int crc_ct,
                                                          ZDev *__restrict__ z, ZOut *__restrict__ zo) {
    const int i = blockIdx.x * kObjThreads + threadIdx.x;
    if (i >= n) return;
    const LoadBlk b = lb[i];
    const bool ok = early_of(i, ob, st, opened, crc_ct) == JFSX_OK;
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

__global__ __launch_bounds__(kObjThreads) void obj_verdict_k(int n, const LoadBlk *__restrict__ lb,
                                                             const ObjBlk *__restrict__ ob,
                                                             const ObjState *__restrict__ st,
                                                             const BlkOut *__restrict__ opened,
                                                             const ZOut *__restrict__ zo, int crc_ct,
                                                             int use_fallback, LoadRes *__restrict__ res) {
    const int i = blockIdx.x * kObjThreads + threadIdx.x;
    if (i >= n) return;
    const ObjState s = st[i];
    const uint64_t len = lb[i].len;
    ZOut o;
    o.out_len = len;
    o.status = JFSX_OK;
    o.fallback = 0;
    if (zo) o = zo[i];
    const jfsx_load::Verdict v =
        jfsx_obj::object_verdict(crc_ct != 0, s.crc_bad != 0, opened != nullptr, ob[i].flags, s.key_len,
                                 opened ? opened[i].status : JFSX_OK, o.status, o.out_len, len);
    const bool decoded = early_of(i, ob, st, opened, crc_ct) == JFSX_OK;
    LoadRes r;
    r.out_len = v.out_len;
    r.status = v.status;
    r.codec_info = use_fallback && decoded ? o.fallback : 0;
    res[i] = r;
}

}  // namespace

void launch_obj_fold(hipStream_t s, int n, const ObjBlk *ob, uint32_t tail, const uint32_t *x8pow, ObjState *st) {
    if (n > 0) hipLaunchKernelGGL(obj_fold_k, dim3(n), dim3(64), 0, s, n, ob, tail, x8pow, st);
}

void launch_obj_keys(hipStream_t s, int n, const ObjBlk *ob, ObjState *st, uint8_t *em, int em_slot,
                     const int32_t *len, KeyIn *keys) {
    if (n > 0)
        hipLaunchKernelGGL(obj_keys_k, dim3((n + kObjThreads - 1) / kObjThreads), dim3(kObjThreads), 0, s, n, ob, st,
                           em, em_slot, len, keys);
}

void launch_obj_gate(hipStream_t s, int n, const LoadBlk *lb, const ObjBlk *ob, const ObjState *st,
                     const BlkOut *opened, bool crc_ct, ZDev *z, ZOut *zo) {
    if (n > 0)
        hipLaunchKernelGGL(obj_gate_k, dim3((n + kObjThreads - 1) / kObjThreads), dim3(kObjThreads), 0, s, n, lb, ob,
                           st, opened, crc_ct ? 1 : 0, z, zo);
}

void launch_obj_verdict(hipStream_t s, int n, const LoadBlk *lb, const ObjBlk *ob, const ObjState *st,
                        const BlkOut *opened, const ZOut *zo, bool crc_ct, bool use_fallback, LoadRes *res) {
    if (n > 0)
        hipLaunchKernelGGL(obj_verdict_k, dim3((n + kObjThreads - 1) / kObjThreads), dim3(kObjThreads), 0, s, n, lb,
                           ob, st, opened, zo, crc_ct ? 1 : 0, use_fallback ? 1 : 0, res);
}

}  // namespace jfsx
