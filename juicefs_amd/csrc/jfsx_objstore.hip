// jfsx_objstore.hip -- the device-side glue of jfsx_store_objects on gfx950: the
// data-key wrap in front of jfsx_store_batch's chain (jfsx_store.hip) and the
// object's frame behind it, so that the write is one stream of kernels from
// the page to the stored object.
//
//   rsa_encode_k + rsa_wrap_k          the wrapped keys, device memory (phase A)
//   page CRCs, gate, compressor,       as jfsx_store_batch; without a codec the
//     verdict                          VERIFY stage alone
//   sobj_keys_k                        before the Seal's keysetup: KeyIn[k].key
//                                      out of the wrap's message slot
//   gcm / chacha Seal                  C at obj + 15 + k, k = 256 or 512 the
//                                      key's modulus length (16-byte aligned:
//                                      obj is 1 mod 16), tag and segment CRCs
//                                      stay in device memory
//   sobj_frame_k                       header, tag, obj_crc; per-block results
//
// The data key is uploaded once, into the wrap's message slot; the Seal's
// KeyIn is filled from there, and the slots are zeroed when the call ends.
#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#include "jfsx_objstore.h"

namespace jfsx {

namespace {

constexpr int kSobjThreads = 256;

// One thread per sealed block.
__global__ __launch_bounds__(kSobjThreads) void sobj_keys_k(int m, const SobjBlk *__restrict__ sb,
                                                            const uint32_t *__restrict__ msg, int slot_words,
                                                            KeyIn *__restrict__ keys) {
    const int k = blockIdx.x * kSobjThreads + threadIdx.x;
    if (k >= m) return;
    const uint32_t *slot = msg + (size_t)slot_words * sb[k].idx;
#pragma unroll
    for (int w = 0; w < 8; w++) keys[k].key[w] = slot[w];
}

// One wave per sealed block.  obj is 1 mod 16, so the wrapped key at obj + 3
// and the nonce behind it take dword stores; the tag lies wherever the image
// ends and takes byte stores.  kbytes: the wrapped key's length, 256 or 512.
__global__ __launch_bounds__(64) void sobj_frame_k(int m, const SobjBlk *__restrict__ sb,
                                                   const uint8_t *__restrict__ wrapped, uint32_t kbytes,
                                                   const BlkOut *__restrict__ sealed,
                                                   const uint8_t *__restrict__ segs, int crc_ct,
                                                   const uint32_t *__restrict__ x8pow, SobjRes *__restrict__ res) {
    const int k = blockIdx.x;
    if (k >= m) return;
    const uint32_t lane = threadIdx.x;
    const SobjBlk b = sb[k];
    const uint8_t *wk = wrapped + (size_t)kbytes * b.idx;
    const uint8_t *tag = reinterpret_cast<const uint8_t *>(sealed[k].tag);
    const uint8_t *nonce = reinterpret_cast<const uint8_t *>(sb[k].nonce);
    jfsx_sobj::frame_store(lane, b.obj, wk, sb[k].nonce, tag, b.img_len, kbytes);
    uint32_t crc = 0;
    if (crc_ct) {
        const uint32_t h = wave_xor(jfsx_sobj::hdr_lane(lane, wk, nonce, x8pow, kbytes));
        const uint32_t t = wave_xor(jfsx_sobj::bytes_lane(lane, tag, jfsx_sobj::kTagBytes, x8pow));
        const uint32_t s = wave_xor(
            jfsx_obj::fold_lane(lane, segs + 4 * (size_t)b.seg_off, b.img_len, jfsx_sobj::kTagBytes, x8pow));
        crc = jfsx_sobj::object_crc(h, s, t, b.img_len, x8pow);
    }
    if (lane == 0) {
        SobjRes r;
        r.out_len = jfsx_sobj::hdr_bytes(kbytes) + b.img_len + jfsx_sobj::kTagBytes;
        r.img_len = b.img_len;
        r.obj_crc = crc;
        r.status = JFSX_OK;
        res[k] = r;
    }
}

}  // namespace

void launch_sobj_keys(hipStream_t s, int m, const SobjBlk *sb, const uint8_t *msg, int kbytes, KeyIn *keys) {
    if (m > 0)
        hipLaunchKernelGGL(sobj_keys_k, dim3((m + kSobjThreads - 1) / kSobjThreads), dim3(kSobjThreads), 0, s, m, sb,
                           reinterpret_cast<const uint32_t *>(msg), rsa_wrap_slot(kbytes) / 4, keys);
}

void launch_sobj_frame(hipStream_t s, int m, const SobjBlk *sb, const uint8_t *wrapped, int kbytes,
                       const BlkOut *sealed, const uint8_t *segs, bool crc_ct, const uint32_t *x8pow, SobjRes *res) {
    if (m > 0)
        hipLaunchKernelGGL(sobj_frame_k, dim3(m), dim3(64), 0, s, m, sb, wrapped, (uint32_t)kbytes, sealed, segs,
                           crc_ct ? 1 : 0, x8pow, res);
}

}  // namespace jfsx
