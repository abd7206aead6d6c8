// jfsx_rsa.hip -- batched RSA-OAEP key unwrap on the GPU, and
// the key wrap, its write side (the last part of this file).
//
// rsaEncryptor.Decrypt (pkg/object/encrypt.go:124-134) runs once per object
// the reference opens (encrypt.go:207-210): an RSA-2048 private operation of
// ~0.35 ms per core, which caps end-to-end Decrypt far below the Open kernel.
// Here one batch unwraps every object key of a read window on the GPU:
//   * rsa_pair_k: two lanes per (object, CRT half): c mod p_h, then
//     c^d_h mod p_h by a fixed-window Montgomery exponentiation in 28-bit
//     limbs with lazy carries, each product split by columns over the lane
//     pair with DPP exchanges (jfsx_rsa.h: mod_exp28_pair), constant time in
//     the exponent.  rsa_half_k (JFSX_RSA_PAIR=0) is the one-lane form
//     (mod_exp28): half the waves, each issuing the whole product.
//   * rsa_finish_k: one thread per object: c < n check, CRT recombination,
//     EME-OAEP decoding (SHA-256, MGF1, label hash), message out.
// Bit-exact to rsa.DecryptOAEP(sha256, ..., "keys") and, like it, constant
// time with respect to the private key and the decrypted data (jfsx_rsa.h):
// no branch and no memory address depends on the exponent, the CRT values or
// the OAEP checks; the one branch on secret-derived data is the final valid /
// invalid outcome, which Go's decryptOAEP also returns as an error.
// A 4096-bit key takes kernels of its own (rsa_words_k, rsa_quad_k,
// rsa_finish_w_k; rsa_wrap_w_k, rsa_pack_k below), the launchers choose by the
// key's modulus length; no other key size exists here.
#include <stdlib.h>
#include <string.h>

#include "jfsx_internal.h"

#define JFSX_HD __device__ __forceinline__
#define JFSX_RSA_OPAQUE(x) asm volatile("" : "+v"(x))
#include "jfsx_rsa.h"

namespace jfsx {

using jfsx_rsa::kLimbs;
using jfsx_rsa::kModBytes;

// threads per workgroup of rsa_half_k
constexpr int kRsaLanes = 64;

__global__ __launch_bounds__(kRsaLanes) void rsa_half_k(const jfsx_rsa::Key *__restrict__ key, int n,
                                                        const uint8_t *__restrict__ ct, uint32_t *__restrict__ mh) {
    const int i = blockIdx.x * kRsaLanes + threadIdx.x;
    const int half = blockIdx.y;  // 0: p, 1: q
    if (i >= n) return;
    const jfsx_rsa::Key &k = *key;
    uint32_t c[2 * kLimbs], x[kLimbs], r[kLimbs];
    jfsx_rsa::from_be(ct + (size_t)kModBytes * i, kModBytes, c, 2 * kLimbs);
    if (half == 0) {
        jfsx_rsa::reduce_2048(c, k.p, k.pinv, k.r2p, x);
        jfsx_rsa::mod_exp28(x, k.dp, k.p, k.pinv, k.r2p28, r);
    } else {
        jfsx_rsa::reduce_2048(c, k.q, k.qinv32, k.r2q, x);
        jfsx_rsa::mod_exp28(x, k.dq, k.q, k.qinv32, k.r2q28, r);
    }
    uint32_t *o = mh + ((size_t)half * n + i) * kLimbs;
#pragma unroll
    for (int j = 0; j < kLimbs; j++) o[j] = r[j];
}

// the lane exchange of mod_exp28_pair: the pair is lanes (2k, 2k+1); DPP
// quad_perm moves (0,0,2,2) / (1,1,3,3) / (1,0,3,2)
struct PairDpp {
    uint32_t hi;
    __device__ __forceinline__ static constexpr bool tracing() { return false; }
    __device__ __forceinline__ uint32_t lo(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, true);
    }
    __device__ __forceinline__ uint32_t up(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xF, 0xF, true);
    }
    __device__ __forceinline__ uint32_t other(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
    }
};

// threads 2i, 2i+1 of the grid: object i; blockIdx.y: the CRT half.  Pairs
// never straddle a bound: both lanes of a pair see the same i.
__global__ __launch_bounds__(64) void rsa_pair_k(const jfsx_rsa::Key *__restrict__ key, int n,
                                                 const uint8_t *__restrict__ ct, uint32_t *__restrict__ mh) {
    const int t = blockIdx.x * 64 + threadIdx.x, i = t >> 1;
    const int half = blockIdx.y;
    if (i >= n) return;
    const PairDpp x{(uint32_t)(t & 1)};
    const jfsx_rsa::Key &k = *key;
    uint32_t c[2 * kLimbs], v[kLimbs], r[kLimbs];
    jfsx_rsa::from_be(ct + (size_t)kModBytes * i, kModBytes, c, 2 * kLimbs);
    if (half == 0) {
        jfsx_rsa::reduce_2048(c, k.p, k.pinv, k.r2p, v);
        jfsx_rsa::mod_exp28_pair(x, v, k.dp, k.p, k.pinv, k.r2p28, r);
    } else {
        jfsx_rsa::reduce_2048(c, k.q, k.qinv32, k.r2q, v);
        jfsx_rsa::mod_exp28_pair(x, v, k.dq, k.q, k.qinv32, k.r2q28, r);
    }
    // each lane stores half of the result
    uint32_t *o = mh + ((size_t)half * n + i) * kLimbs + (t & 1) * (kLimbs / 2);
#pragma unroll
    for (int j = 0; j < kLimbs / 2; j++) o[j] = (t & 1) ? r[kLimbs / 2 + j] : r[j];
}

__global__ __launch_bounds__(64) void rsa_finish_k(const jfsx_rsa::Key *__restrict__ key, int n,
                                                   const uint8_t *__restrict__ ct, const uint32_t *__restrict__ mh,
                                                   uint8_t *__restrict__ em_out, int32_t *__restrict__ len_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const jfsx_rsa::Key &k = *key;
    uint32_t c[2 * kLimbs], m1[kLimbs], m2[kLimbs], m[2 * kLimbs];
    jfsx_rsa::from_be(ct + (size_t)kModBytes * i, kModBytes, c, 2 * kLimbs);
    uint8_t *em = em_out + (size_t)kModBytes * i;
    if (jfsx_rsa::geq(c, k.n, 2 * kLimbs)) {  // rsa.decrypt: c >= n is a decryption error
        len_out[i] = -1;
        return;
    }
    for (int j = 0; j < kLimbs; j++) {
        m1[j] = mh[(size_t)i * kLimbs + j];
        m2[j] = mh[((size_t)n + i) * kLimbs + j];
    }
    jfsx_rsa::crt(k, m1, m2, m);
    uint8_t buf[kModBytes];
    jfsx_rsa::to_be(m, 2 * kLimbs, buf, kModBytes);
    const int len = jfsx_rsa::oaep_decode(buf, kModBytes, k.lhash);
    for (int j = 0; j < (len > 0 ? len : 0); j++) em[j] = buf[j];
    len_out[i] = len;
}

// ---------------------------------------------------------------------------
// RSA-4096 (jfsx_rsa.h: KeyW).  The workspace per object: the ciphertext as
// 128 little-endian words (cw), then both CRT halves' results as 76 28-bit
// limbs each (rsa_mh_words(512) words in all).
//   * rsa_words_k: one thread per word: the 512 big-endian bytes to cw.
//   * rsa_quad_k: the four lanes of a DPP quad per (object, CRT half), 16 per
//     wave: c mod p_h through the quad product (reduce_quad), then c^d_h mod
//     p_h by mod_exp28_priv_quad, the 8 x 19 window table in registers.  The
//     one-lane A/B form (JFSX_RSA_PAIR=0) does not exist at this width.
//   * rsa_finish_w_k: rsa_finish_k at k = 512.
// ---------------------------------------------------------------------------
using jfsx_rsa::kLimbsW;
using jfsx_rsa::kModBytesW;
using jfsx_rsa::kNLimbsW;
constexpr int kHalfWords = 4 * jfsx_rsa::kQC;  // a CRT half's result: 76 limbs of 28 bits

__global__ __launch_bounds__(64) void rsa_words_k(int n, const uint8_t *__restrict__ ct, uint32_t *__restrict__ cw) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)n * kNLimbsW) return;
    const size_t i = t / kNLimbsW, w = t % kNLimbsW;  // word w is bytes 508 - 4w .. 511 - 4w
    cw[t] = __builtin_bswap32(*(const uint32_t *)(ct + kModBytesW * i + 4 * (kNLimbsW - 1 - w)));
}

// the lane exchange of the quad forms: the quad is lanes (4k .. 4k+3); DPP
// quad_perm broadcasts (K,K,K,K) and the cyclic shifts (1,2,3,0) / (3,0,1,2)
struct QuadDpp {
    uint32_t lane;
    __device__ __forceinline__ static constexpr bool tracing() { return false; }
    template <int K>
    __device__ __forceinline__ uint32_t from(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, K * 0x55, 0xF, 0xF, true);
    }
    __device__ __forceinline__ uint32_t next(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x39, 0xF, 0xF, true);
    }
    __device__ __forceinline__ uint32_t prev(uint32_t v) const {
        return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x93, 0xF, 0xF, true);
    }
};

// threads 4i .. 4i+3 of the grid: object i; blockIdx.y: the CRT half.  Quads
// never straddle a bound: all four lanes see the same i.  Every address below
// depends on i, the half and the lane only.
__global__ __launch_bounds__(64) void rsa_quad_k(const jfsx_rsa::KeyW *__restrict__ key, int n,
                                                 const uint32_t *__restrict__ cw, uint32_t *__restrict__ mh) {
    constexpr int QC = jfsx_rsa::kQC;
    const int t = blockIdx.x * 64 + threadIdx.x, i = t >> 2;
    const int half = blockIdx.y;
    if (i >= n) return;
    const uint32_t lane = (uint32_t)(t & 3);
    const QuadDpp x{lane};
    const jfsx_rsa::KeyW &k = *key;
    const uint32_t *m32 = half ? k.q : k.p, *d32 = half ? k.dq : k.dp, *r2_32 = half ? k.r2q28 : k.r2p28,
                   *rx32 = half ? k.rxq : k.rxp;
    const uint32_t minv = (half ? k.qinv32 : k.pinv) & jfsx_rsa::kM28;
    const uint32_t *c = cw + (size_t)kNLimbsW * i;
    uint32_t m[QC], r2[QC], v[QC], r[QC];
    {
        uint32_t hi[QC], lo[QC], rx[QC];
#pragma unroll
        for (int j = 0; j < QC; j++) {
            const int col = QC * (int)lane + j;  // limb28 gives zero past bit 2048: columns 74, 75 and the top of 73
            m[j] = jfsx_rsa::limb28(m32, kLimbsW, col);
            r2[j] = jfsx_rsa::limb28(r2_32, kLimbsW, col);
            rx[j] = jfsx_rsa::limb28(rx32, kLimbsW, col);
            lo[j] = jfsx_rsa::limb28(c, kLimbsW, col);
            hi[j] = jfsx_rsa::limb28(c + kLimbsW, kLimbsW, col);
        }
        jfsx_rsa::reduce_quad(x, hi, lo, m, minv, rx, v);
    }
    jfsx_rsa::mod_exp28_priv_quad(x, v, d32, m, minv, r2, r);
    uint32_t *o = mh + ((size_t)half * n + i) * kHalfWords + QC * lane;
#pragma unroll
    for (int j = 0; j < QC; j++) o[j] = r[j];
}

__global__ __launch_bounds__(64) void rsa_finish_w_k(const jfsx_rsa::KeyW *__restrict__ key, int n,
                                                     const uint32_t *__restrict__ cw,
                                                     const uint32_t *__restrict__ mh, uint8_t *__restrict__ em_out,
                                                     int32_t *__restrict__ len_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const jfsx_rsa::KeyW &k = *key;
    uint8_t *em = em_out + (size_t)kModBytesW * i;
    if (jfsx_rsa::geq(cw + (size_t)kNLimbsW * i, k.n, kNLimbsW)) {  // rsa.decrypt: c >= n is a decryption error
        len_out[i] = -1;
        return;
    }
    uint32_t m1[kLimbsW], m2[kLimbsW], m[kNLimbsW];
    jfsx_rsa::from28_wide(mh + (size_t)i * kHalfWords, jfsx_rsa::kN28, m1, kLimbsW);
    jfsx_rsa::from28_wide(mh + ((size_t)n + i) * kHalfWords, jfsx_rsa::kN28, m2, kLimbsW);
    jfsx_rsa::crt<kLimbsW>(k, m1, m2, m);
    uint8_t buf[kModBytesW];
    jfsx_rsa::to_be(m, kNLimbsW, buf, kModBytesW);
    const int len = jfsx_rsa::oaep_decode(buf, kModBytesW, k.lhash);
    for (int j = 0; j < (len > 0 ? len : 0); j++) em[j] = buf[j];
    len_out[i] = len;
}

void launch_rsa_unwrap(hipStream_t s, const void *key, int kbytes, int n, const uint8_t *ct, uint32_t *mh,
                       uint8_t *em, int32_t *len) {
    if (n <= 0) return;
    if (kbytes == kModBytesW) {
        const jfsx_rsa::KeyW *kw = (const jfsx_rsa::KeyW *)key;
        uint32_t *cw = mh, *halves = mh + (size_t)kNLimbsW * n;
        const size_t words = (size_t)n * kNLimbsW;
        hipLaunchKernelGGL(rsa_words_k, dim3((unsigned)((words + 63) / 64)), dim3(64), 0, s, n, ct, cw);
        hipLaunchKernelGGL(rsa_quad_k, dim3((n + 15) / 16, 2), dim3(64), 0, s, kw, n, cw, halves);
        hipLaunchKernelGGL(rsa_finish_w_k, dim3((n + 63) / 64), dim3(64), 0, s, kw, n, cw, halves, em, len);
        return;
    }
    static const bool pair = [] {  // JFSX_RSA_PAIR=0: the one-lane kernel (A/B)
        const char *e = getenv("JFSX_RSA_PAIR");
        return !(e && !strcmp(e, "0"));
    }();
    const int g = (n + 63) / 64, gh = (n + kRsaLanes - 1) / kRsaLanes;
    if (pair)
        hipLaunchKernelGGL(rsa_pair_k, dim3((2 * n + 63) / 64, 2), dim3(64), 0, s, (const jfsx_rsa::Key *)key, n, ct,
                           mh);
    else
        hipLaunchKernelGGL(rsa_half_k, dim3(gh, 2), dim3(kRsaLanes), 0, s, (const jfsx_rsa::Key *)key, n, ct, mh);
    hipLaunchKernelGGL(rsa_finish_k, dim3(g), dim3(64), 0, s, (const jfsx_rsa::Key *)key, n, ct, mh, em, len);
}

// ---------------------------------------------------------------------------
// The key wrap, the write side (rsaEncryptor.Encrypt, encrypt.go:128-130,
// called per object at :169): rsa.EncryptOAEP(sha256, rand, pub, key, label)
// for a whole upload window.
//   * rsa_encode_k: one thread per item: EME-OAEP encoding with the caller's
//     seed into the workspace, as 64 32-bit limbs (rsa_finish_k in reverse).
//     An item longer than the OAEP capacity encodes as zero, which the
//     exponentiation maps to 256 zero bytes.
//   * rsa_wrap_k: the four lanes of a DPP quad per item: EM^e mod n by
//     jfsx_rsa.h's mod_exp28_pub_quad, then 256 big-endian bytes, a quarter
//     from each lane.
// No branch and no address depends on the data key or the seed; e and the
// message lengths are public.
// ---------------------------------------------------------------------------
// (K = jfsx_rsa::Key, MB = 256, or KeyW and 512; slot = rsa_wrap_slot(MB))
template <class K, int MB>
__global__ __launch_bounds__(64) void rsa_encode_k(const K *__restrict__ key, int n, const uint8_t *__restrict__ msg,
                                                   const uint32_t *__restrict__ len, const uint8_t *__restrict__ seed,
                                                   uint32_t *__restrict__ em_out) {
    constexpr int NL = MB / 4, kMax = MB - 2 * jfsx_rsa::kHash - 2, kSlot = rsa_wrap_slot(MB);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t *o = em_out + (size_t)rsa_em_words(MB) * i;
    const uint32_t l = len[i];
    if (l > (uint32_t)kMax) {  // "message too long for RSA key size"
        for (int j = 0; j < NL; j++) o[j] = 0;
        return;
    }
    uint8_t em[MB];
    jfsx_rsa::oaep_encode(key->lhash, msg + (size_t)kSlot * i, (int)l, seed + (size_t)jfsx_rsa::kHash * i, em, MB);
    uint32_t x[NL];
    jfsx_rsa::from_be(em, MB, x, NL);
    for (int j = 0; j < NL; j++) o[j] = x[j];
}

// threads 4i .. 4i+3 of the grid: item i (16 items per workgroup).  Quads
// never straddle a bound: all four lanes see the same i.  (K, N = Key, 74, or
// the form rsa_wrap_w_k below takes at 4096 bits.)
template <class K, int N>
__global__ __launch_bounds__(64) void rsa_wrap_k(const K *__restrict__ key, uint32_t e, int n,
                                                 const uint32_t *__restrict__ em, uint8_t *__restrict__ ct) {
    constexpr int NL = jfsx_rsa::n32_of(N);  // n in 32-bit limbs
    const int t = blockIdx.x * 64 + threadIdx.x, i = t >> 2;
    if (i >= n) return;
    const uint32_t lane = (uint32_t)(t & 3);
    const QuadDpp x{lane};
    const K &k = *key;
    uint32_t r[NL];
    jfsx_rsa::mod_exp28_pub_quad<QuadDpp, N>(x, em + (size_t)NL * i, e, k.n, k.ninv28, k.r2n28, r);
    // lane L stores limbs Q L .. Q L + Q - 1: limb w is bytes 4 (NL - 1 - w) .. + 3
    uint32_t *o = (uint32_t *)(ct + (size_t)(4 * NL) * i);
    constexpr int Q = NL / 4;
    // (picked with masks behind a register barrier: a select on the lane would
    // become an indexed read of r, and r would live in scratch memory)
    uint32_t odd = 0u - (lane & 1u), upper = 0u - (lane >> 1);
    JFSX_RSA_OPAQUE(odd);
    JFSX_RSA_OPAQUE(upper);
#pragma unroll
    for (int j = 0; j < Q; j++) {
        const uint32_t lo = (r[j] & ~odd) | (r[Q + j] & odd), hi = (r[2 * Q + j] & ~odd) | (r[3 * Q + j] & odd);
        o[NL - 1 - ((int)lane * Q + j)] = __builtin_bswap32((lo & ~upper) | (hi & upper));
    }
}

// The same at 4096 bits, 37 columns per lane.  Gathering the whole result into
// every lane (148 + 128 registers after the loop) is what would not fit: each
// lane stores its 37 limbs of 28 bits over the item's EM slot (rsa_em_words(512)
// = 148 words; all four lanes have read EM before the first product), and
// rsa_pack_k, one thread per word, makes the 512 big-endian bytes of them.
__global__ __launch_bounds__(64) void rsa_wrap_w_k(const jfsx_rsa::KeyW *__restrict__ key, uint32_t e, int n,
                                                   uint32_t *em) {
    constexpr int QC = jfsx_rsa::kQCW;
    const int t = blockIdx.x * 64 + threadIdx.x, i = t >> 2;
    if (i >= n) return;
    const uint32_t lane = (uint32_t)(t & 3);
    const QuadDpp x{lane};
    const jfsx_rsa::KeyW &k = *key;
    uint32_t r[QC];
    uint32_t *slot = em + (size_t)rsa_em_words(kModBytesW) * i;
    // x R'' parks in this lane's quarter of the slot: EM has been read by then
    jfsx_rsa::mod_exp28_pub_quad_lane<QuadDpp, jfsx_rsa::kN28W>(x, slot, e, k.n, k.ninv28, k.r2n28, r,
                                                                slot + QC * lane);
#pragma unroll
    for (int j = 0; j < QC; j++) slot[QC * lane + j] = r[j];
}

__global__ __launch_bounds__(64) void rsa_pack_k(int n, const uint32_t *__restrict__ em, uint8_t *__restrict__ ct) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)n * kNLimbsW) return;
    const size_t i = t / kNLimbsW;
    const int w = (int)(t % kNLimbsW), bit = 32 * w, l = bit / 28, o = bit % 28;  // from28_wide's word w
    const uint32_t *y = em + (size_t)rsa_em_words(kModBytesW) * i;
    const uint64_t v = ((uint64_t)y[l] >> o) | ((uint64_t)y[l + 1] << (28 - o));  // l + 1 <= 147 < 148
    *(uint32_t *)(ct + kModBytesW * i + 4 * (kNLimbsW - 1 - w)) = __builtin_bswap32((uint32_t)v);
}

void launch_rsa_wrap(hipStream_t s, const void *key, int kbytes, uint32_t e, int n, const uint8_t *msg,
                     const uint32_t *len, const uint8_t *seed, uint32_t *em, uint8_t *ct) {
    if (n <= 0) return;
    const dim3 ge((n + 63) / 64), gw((n + 15) / 16);
    if (kbytes == kModBytesW) {
        const jfsx_rsa::KeyW *kw = (const jfsx_rsa::KeyW *)key;
        const size_t words = (size_t)n * kNLimbsW;
        hipLaunchKernelGGL((rsa_encode_k<jfsx_rsa::KeyW, kModBytesW>), ge, dim3(64), 0, s, kw, n, msg, len, seed, em);
        hipLaunchKernelGGL(rsa_wrap_w_k, gw, dim3(64), 0, s, kw, e, n, em);
        hipLaunchKernelGGL(rsa_pack_k, dim3((unsigned)((words + 63) / 64)), dim3(64), 0, s, n, (const uint32_t *)em, ct);
        return;
    }
    const jfsx_rsa::Key *k2 = (const jfsx_rsa::Key *)key;
    hipLaunchKernelGGL((rsa_encode_k<jfsx_rsa::Key, kModBytes>), ge, dim3(64), 0, s, k2, n, msg, len, seed, em);
    hipLaunchKernelGGL((rsa_wrap_k<jfsx_rsa::Key, jfsx_rsa::kN28>), gw, dim3(64), 0, s, k2, e, n, em, ct);
}

}  // namespace jfsx
