// jfsx_md5.h -- RFC 1321 MD5, written once for the host and the GPU.
//
// Hadoop's file checksum (MD5-of-MD5-of-CRC32C, getFileChecksum in
// sdk/java/src/main/java/io/juicefs/JuiceFileSystemImpl.java:1286-1343) hashes
// each DFS block's chunk CRCs with MD5 and then the block digests again.
// md5_blocks_k (jfsx_crc.hip) runs compress() one lane per DFS block; the
// host folds the block digests with init / update / final (jfsx_api.cpp).
//
// The round functions are plain C.  On gfx950 the compiler turns F, G and I
// into one v_bitop3_b32 (or v_bfi_b32) each and every rotate into one
// v_alignbit_b32, but leaves H as two v_xor_b32, so H alone is spelled as the
// three-input XOR builtin there: a compression is 64 v_alignbit_b32, 64
// bit operations and about 190 additions (v_add3_u32 / v_add_u32), 5 VALU
// operations per step.  With the 64 steps unrolled the constants, shifts and
// message indices are literals.
//
// Host/device portable: the includer defines JFSX_MD5_HD (the GPU build:
// __host__ __device__ __forceinline__); tests/harness/md5_host.cpp checks it
// against the RFC's test suite on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef JFSX_MD5_HD
#define JFSX_MD5_HD static inline
#endif

namespace jfsx_md5 {

JFSX_MD5_HD uint32_t rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// one step: a = b + rotl(a + f + k + m, s)
#define JFSX_MD5_STEP(f, a, b, c, d, m, k, s) (a) = (b) + rotl((a) + f((b), (c), (d)) + (k) + (m), (s))
#define JFSX_MD5_F(x, y, z) (((x) & (y)) | (~(x) & (z)))
#define JFSX_MD5_G(x, y, z) (((x) & (z)) | ((y) & ~(z)))
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
#define JFSX_MD5_H(x, y, z) __builtin_amdgcn_bitop3_b32((x), (y), (z), 0x96)
#else
#define JFSX_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#endif
#define JFSX_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))

// the initial chaining value (RFC 1321 3.3)
JFSX_MD5_HD void iv(uint32_t st[4]) {
    st[0] = 0x67452301u;
    st[1] = 0xefcdab89u;
    st[2] = 0x98badcfeu;
    st[3] = 0x10325476u;
}

// st += MD5 compression of the 16 little-endian message words m (RFC 1321 3.4)
JFSX_MD5_HD void compress(uint32_t st[4], const uint32_t m[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#define R1(a, b, c, d, i, s, k) JFSX_MD5_STEP(JFSX_MD5_F, a, b, c, d, m[i], k, s)
#define R2(a, b, c, d, i, s, k) JFSX_MD5_STEP(JFSX_MD5_G, a, b, c, d, m[i], k, s)
#define R3(a, b, c, d, i, s, k) JFSX_MD5_STEP(JFSX_MD5_H, a, b, c, d, m[i], k, s)
#define R4(a, b, c, d, i, s, k) JFSX_MD5_STEP(JFSX_MD5_I, a, b, c, d, m[i], k, s)
    R1(a, b, c, d, 0, 7, 0xd76aa478u);
    R1(d, a, b, c, 1, 12, 0xe8c7b756u);
    R1(c, d, a, b, 2, 17, 0x242070dbu);
    R1(b, c, d, a, 3, 22, 0xc1bdceeeu);
    R1(a, b, c, d, 4, 7, 0xf57c0fafu);
    R1(d, a, b, c, 5, 12, 0x4787c62au);
    R1(c, d, a, b, 6, 17, 0xa8304613u);
    R1(b, c, d, a, 7, 22, 0xfd469501u);
    R1(a, b, c, d, 8, 7, 0x698098d8u);
    R1(d, a, b, c, 9, 12, 0x8b44f7afu);
    R1(c, d, a, b, 10, 17, 0xffff5bb1u);
    R1(b, c, d, a, 11, 22, 0x895cd7beu);
    R1(a, b, c, d, 12, 7, 0x6b901122u);
    R1(d, a, b, c, 13, 12, 0xfd987193u);
    R1(c, d, a, b, 14, 17, 0xa679438eu);
    R1(b, c, d, a, 15, 22, 0x49b40821u);

    R2(a, b, c, d, 1, 5, 0xf61e2562u);
    R2(d, a, b, c, 6, 9, 0xc040b340u);
    R2(c, d, a, b, 11, 14, 0x265e5a51u);
    R2(b, c, d, a, 0, 20, 0xe9b6c7aau);
    R2(a, b, c, d, 5, 5, 0xd62f105du);
    R2(d, a, b, c, 10, 9, 0x02441453u);
    R2(c, d, a, b, 15, 14, 0xd8a1e681u);
    R2(b, c, d, a, 4, 20, 0xe7d3fbc8u);
    R2(a, b, c, d, 9, 5, 0x21e1cde6u);
    R2(d, a, b, c, 14, 9, 0xc33707d6u);
    R2(c, d, a, b, 3, 14, 0xf4d50d87u);
    R2(b, c, d, a, 8, 20, 0x455a14edu);
    R2(a, b, c, d, 13, 5, 0xa9e3e905u);
    R2(d, a, b, c, 2, 9, 0xfcefa3f8u);
    R2(c, d, a, b, 7, 14, 0x676f02d9u);
    R2(b, c, d, a, 12, 20, 0x8d2a4c8au);

    R3(a, b, c, d, 5, 4, 0xfffa3942u);
    R3(d, a, b, c, 8, 11, 0x8771f681u);
    R3(c, d, a, b, 11, 16, 0x6d9d6122u);
    R3(b, c, d, a, 14, 23, 0xfde5380cu);
    R3(a, b, c, d, 1, 4, 0xa4beea44u);
    R3(d, a, b, c, 4, 11, 0x4bdecfa9u);
    R3(c, d, a, b, 7, 16, 0xf6bb4b60u);
    R3(b, c, d, a, 10, 23, 0xbebfbc70u);
    R3(a, b, c, d, 13, 4, 0x289b7ec6u);
    R3(d, a, b, c, 0, 11, 0xeaa127fau);
    R3(c, d, a, b, 3, 16, 0xd4ef3085u);
    R3(b, c, d, a, 6, 23, 0x04881d05u);
    R3(a, b, c, d, 9, 4, 0xd9d4d039u);
    R3(d, a, b, c, 12, 11, 0xe6db99e5u);
    R3(c, d, a, b, 15, 16, 0x1fa27cf8u);
    R3(b, c, d, a, 2, 23, 0xc4ac5665u);

    R4(a, b, c, d, 0, 6, 0xf4292244u);
    R4(d, a, b, c, 7, 10, 0x432aff97u);
    R4(c, d, a, b, 14, 15, 0xab9423a7u);
    R4(b, c, d, a, 5, 21, 0xfc93a039u);
    R4(a, b, c, d, 12, 6, 0x655b59c3u);
    R4(d, a, b, c, 3, 10, 0x8f0ccc92u);
    R4(c, d, a, b, 10, 15, 0xffeff47du);
    R4(b, c, d, a, 1, 21, 0x85845dd1u);
    R4(a, b, c, d, 8, 6, 0x6fa87e4fu);
    R4(d, a, b, c, 15, 10, 0xfe2ce6e0u);
    R4(c, d, a, b, 6, 15, 0xa3014314u);
    R4(b, c, d, a, 13, 21, 0x4e0811a1u);
    R4(a, b, c, d, 4, 6, 0xf7537e82u);
    R4(d, a, b, c, 11, 10, 0xbd3af235u);
    R4(c, d, a, b, 2, 15, 0x2ad7d2bbu);
    R4(b, c, d, a, 9, 21, 0xeb86d391u);
#undef R1
#undef R2
#undef R3
#undef R4
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
}

#undef JFSX_MD5_STEP
#undef JFSX_MD5_F
#undef JFSX_MD5_G
#undef JFSX_MD5_H
#undef JFSX_MD5_I

// The end of a message of nw 32-bit words (any nw >= 0, so any length that is
// a multiple of 4 bytes: the padding's 0x80 byte starts a word): the last
// nw % 16 words, read through ld(i), i in [nw - nw % 16, nw), the padding and
// the length, in one or two compressions.  No dynamic indexing of m[] (it
// stays in registers on the GPU).
template <class Load>
JFSX_MD5_HD void finish_words(uint32_t st[4], uint64_t nw, Load ld) {
    uint32_t m[16];
    const uint32_t r = (uint32_t)(nw % 16);
    const uint64_t w0 = nw - r, bits = nw * 32;
    for (uint32_t i = 0; i < 16; i++) m[i] = i < r ? ld(w0 + i) : (i == r ? 0x80u : 0u);
    if (r >= 14) {  // no room for the length: it goes into a block of its own
        compress(st, m);
        for (int i = 0; i < 14; i++) m[i] = 0;
    }
    m[14] = (uint32_t)bits;
    m[15] = (uint32_t)(bits >> 32);
    compress(st, m);
}

// st = MD5 state of a whole message of nw words read through ld(i)
template <class Load>
JFSX_MD5_HD void hash_words(uint32_t st[4], uint64_t nw, Load ld) {
    iv(st);
    uint32_t m[16];
    for (uint64_t k = 0; k < nw / 16; k++) {
        for (int i = 0; i < 16; i++) m[i] = ld(16 * k + i);
        compress(st, m);
    }
    finish_words(st, nw, ld);
}

// ---- host: streaming interface over bytes --------------------------------
struct Ctx {
    uint32_t st[4];
    uint64_t len;     // bytes hashed so far
    uint8_t buf[64];  // the partial block
};

static inline void block_bytes(uint32_t st[4], const uint8_t *p) {
    uint32_t m[16];
    for (int i = 0; i < 16; i++)
        m[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
               (uint32_t)p[4 * i + 3] << 24;
    compress(st, m);
}

static inline void init(Ctx *c) {
    iv(c->st);
    c->len = 0;
}

static inline void update(Ctx *c, const void *data, uint64_t n) {
    const uint8_t *p = (const uint8_t *)data;
    uint32_t have = (uint32_t)(c->len & 63);
    c->len += n;
    if (have) {
        const uint32_t take = 64 - have < n ? 64 - have : (uint32_t)n;
        memcpy(c->buf + have, p, take);
        p += take;
        n -= take;
        have += take;
        if (have < 64) return;
        block_bytes(c->st, c->buf);
    }
    for (; n >= 64; p += 64, n -= 64) block_bytes(c->st, p);
    if (n) memcpy(c->buf, p, n);
}

static inline void final(Ctx *c, uint8_t out[16]) {
    const uint64_t bits = c->len * 8;
    uint32_t have = (uint32_t)(c->len & 63);
    c->buf[have++] = 0x80;
    if (have > 56) {
        memset(c->buf + have, 0, 64 - have);
        block_bytes(c->st, c->buf);
        have = 0;
    }
    memset(c->buf + have, 0, 56 - have);
    for (int i = 0; i < 8; i++) c->buf[56 + i] = (uint8_t)(bits >> (8 * i));
    block_bytes(c->st, c->buf);
    for (int i = 0; i < 16; i++) out[i] = (uint8_t)(c->st[i >> 2] >> (8 * (i & 3)));
}

static inline void digest(const void *data, uint64_t n, uint8_t out[16]) {
    Ctx c;
    init(&c);
    update(&c, data, n);
    final(&c, out);
}

}  // namespace jfsx_md5
