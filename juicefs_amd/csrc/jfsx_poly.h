// jfsx_poly.h -- Poly1305 field arithmetic mod p = 2^130 - 5 in five 26-bit
// limbs, as the ChaCha20-Poly1305 kernels (jfsx_chacha.hip) use it: the lane
// Horner steps, the lifts by powers of r, the canonical reduction and the
// final h + s.
//
// Host/device portable: the includer defines JFSX_P5_HD (the GPU build:
// __device__ __forceinline__); tests/harness/poly_host.cpp builds it for the
// host, where tests/test_poly1305.py checks every function against Python
// integers at the carry edges no random message reaches.  The wave reduction
// (p_wave_sum) shuffles and stays in jfsx_chacha.hip.
#pragma once
#include <stdint.h>

#ifndef JFSX_P5_HD
#define JFSX_P5_HD static inline
#endif

namespace jfsx {

// v_alignbit_b32: the low word of ((hi:lo) >> s), s < 32
#if defined(__HIPCC__)
#define JFSX_P5_ALIGNBIT(hi, lo, s) __builtin_amdgcn_alignbit(hi, lo, s)
#else
#define JFSX_P5_ALIGNBIT(hi, lo, s) ((uint32_t)((((uint64_t)(hi) << 32) | (uint32_t)(lo)) >> ((s) & 31)))
#endif

constexpr uint32_t M26 = 0x3ffffffu;

// ---------------------------------------------------------------------------
// Poly1305 arithmetic mod p = 2^130 - 5, five 26-bit limbs
// ---------------------------------------------------------------------------
struct P5 {
    uint32_t l[5];
};

JFSX_P5_HD P5 p_zero() { return P5{{0, 0, 0, 0, 0}}; }
JFSX_P5_HD P5 p_one() { return P5{{1, 0, 0, 0, 0}}; }

// a * b mod p (partially reduced: limbs < 2^26 + small)
JFSX_P5_HD P5 p_mul(const P5 &a, const P5 &b) {
    const uint32_t s1 = b.l[1] * 5, s2 = b.l[2] * 5, s3 = b.l[3] * 5, s4 = b.l[4] * 5;
    typedef uint64_t u64;
    u64 d0 = (u64)a.l[0] * b.l[0] + (u64)a.l[1] * s4 + (u64)a.l[2] * s3 + (u64)a.l[3] * s2 + (u64)a.l[4] * s1;
    u64 d1 = (u64)a.l[0] * b.l[1] + (u64)a.l[1] * b.l[0] + (u64)a.l[2] * s4 + (u64)a.l[3] * s3 + (u64)a.l[4] * s2;
    u64 d2 = (u64)a.l[0] * b.l[2] + (u64)a.l[1] * b.l[1] + (u64)a.l[2] * b.l[0] + (u64)a.l[3] * s4 + (u64)a.l[4] * s3;
    u64 d3 = (u64)a.l[0] * b.l[3] + (u64)a.l[1] * b.l[2] + (u64)a.l[2] * b.l[1] + (u64)a.l[3] * b.l[0] + (u64)a.l[4] * s4;
    u64 d4 = (u64)a.l[0] * b.l[4] + (u64)a.l[1] * b.l[3] + (u64)a.l[2] * b.l[2] + (u64)a.l[3] * b.l[1] + (u64)a.l[4] * b.l[0];
    P5 r;
    d1 += d0 >> 26; r.l[0] = (uint32_t)d0 & M26;
    d2 += d1 >> 26; r.l[1] = (uint32_t)d1 & M26;
    d3 += d2 >> 26; r.l[2] = (uint32_t)d2 & M26;
    d4 += d3 >> 26; r.l[3] = (uint32_t)d3 & M26;
    const u64 t = (u64)r.l[0] + (d4 >> 26) * 5;
    r.l[4] = (uint32_t)d4 & M26;
    r.l[0] = (uint32_t)t & M26;
    r.l[1] += (uint32_t)(t >> 26);
    return r;
}

// Horner step a * b + m mod p for the main loop: b is r or r^253 (limbs
// < 2^26), sb[i] = 5 * b.l[i] precomputed, m a message block (limbs < 2^26).
// The message limbs and each carry enter the next limb's product sum as its
// first addend, carries are 32-bit (every d_i < 2^57, so d_i >> 26 < 2^31),
// and the top carry folds back into limb 0 times 5 (d4 has no wrapped
// products: d4 < 2^54.4, 5 * (d4 >> 26) < 2^31).  Output limbs < 2^26 except
// l[1] < 2^26 + 2^6.
#define MADC(x, y, z) ((uint64_t)(x) * (y) + (z))

JFSX_P5_HD P5 p_mul_add(const P5 &a, const P5 &b, const uint32_t (&sb)[5], const P5 &m) {
    typedef uint64_t u64;
    P5 r;
    u64 d = MADC(a.l[4], sb[1], MADC(a.l[3], sb[2], MADC(a.l[2], sb[3], MADC(a.l[1], sb[4],
            MADC(a.l[0], b.l[0], (u64)m.l[0])))));
    r.l[0] = (uint32_t)d & M26;
    uint32_t c = (uint32_t)(d >> 26);
    d = MADC(a.l[4], sb[2], MADC(a.l[3], sb[3], MADC(a.l[2], sb[4], MADC(a.l[1], b.l[0],
        MADC(a.l[0], b.l[1], (u64)(c + m.l[1]))))));
    r.l[1] = (uint32_t)d & M26;
    c = (uint32_t)(d >> 26);
    d = MADC(a.l[4], sb[3], MADC(a.l[3], sb[4], MADC(a.l[2], b.l[0], MADC(a.l[1], b.l[1],
        MADC(a.l[0], b.l[2], (u64)(c + m.l[2]))))));
    r.l[2] = (uint32_t)d & M26;
    c = (uint32_t)(d >> 26);
    d = MADC(a.l[4], sb[4], MADC(a.l[3], b.l[0], MADC(a.l[2], b.l[1], MADC(a.l[1], b.l[2],
        MADC(a.l[0], b.l[3], (u64)(c + m.l[3]))))));
    r.l[3] = (uint32_t)d & M26;
    c = (uint32_t)(d >> 26);
    d = MADC(a.l[4], b.l[0], MADC(a.l[3], b.l[1], MADC(a.l[2], b.l[2], MADC(a.l[1], b.l[3],
        MADC(a.l[0], b.l[4], (u64)(c + m.l[4]))))));
    r.l[4] = (uint32_t)d & M26;
    c = (uint32_t)(d >> 26);
    const uint32_t t = r.l[0] + c * 5u;
    r.l[0] = t & M26;
    r.l[1] += t >> 26;
    return r;
}

JFSX_P5_HD P5 p_add(const P5 &a, const P5 &b) {
    P5 r;
#pragma unroll
    for (int i = 0; i < 5; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}

// canonical representative in [0, p)
JFSX_P5_HD P5 p_freeze(P5 a) {
    uint32_t c;
#pragma unroll
    for (int rep = 0; rep < 2; rep++) {
        c = a.l[0] >> 26; a.l[0] &= M26; a.l[1] += c;
        c = a.l[1] >> 26; a.l[1] &= M26; a.l[2] += c;
        c = a.l[2] >> 26; a.l[2] &= M26; a.l[3] += c;
        c = a.l[3] >> 26; a.l[3] &= M26; a.l[4] += c;
        c = a.l[4] >> 26; a.l[4] &= M26; a.l[0] += c * 5;
    }
    // a < 2^130 now; subtract p if a >= p
    P5 g;
    c = a.l[0] + 5; g.l[0] = c & M26; c >>= 26;
    c += a.l[1]; g.l[1] = c & M26; c >>= 26;
    c += a.l[2]; g.l[2] = c & M26; c >>= 26;
    c += a.l[3]; g.l[3] = c & M26; c >>= 26;
    c += a.l[4]; g.l[4] = c & M26; c >>= 26;  // c = 1 iff a + 5 >= 2^130 iff a >= p
    return c ? g : a;
}

// 16 little-endian bytes (+ 2^128 when hibit) to limbs
JFSX_P5_HD P5 p_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit) {
    P5 r;
    r.l[0] = w0 & M26;
    r.l[1] = JFSX_P5_ALIGNBIT(w1, w0, 26) & M26;
    r.l[2] = JFSX_P5_ALIGNBIT(w2, w1, 20) & M26;
    r.l[3] = JFSX_P5_ALIGNBIT(w3, w2, 14) & M26;
    r.l[4] = (w3 >> 8) | (hibit << 24);
    return r;
}

JFSX_P5_HD P5 p_load(const uint32_t *s) { return P5{{s[0], s[1], s[2], s[3], s[4]}}; }

// r^e from the r^(2^k) table
JFSX_P5_HD P5 p_pow(const uint32_t (*r2k)[5], uint64_t e) {
    P5 z = p_one();
    for (int k = 0; e; k++, e >>= 1)
        if (e & 1) z = p_mul(z, p_load(r2k[k]));
    return z;
}

// tag = (h + s) mod 2^128 of a canonical h, as four little-endian words
JFSX_P5_HD void p_tag(const P5 &acc, const uint32_t s[4], uint32_t out[4]) {
    const uint32_t h0 = acc.l[0] | (acc.l[1] << 26), h1 = (acc.l[1] >> 6) | (acc.l[2] << 20),
                   h2 = (acc.l[2] >> 12) | (acc.l[3] << 14), h3 = (acc.l[3] >> 18) | (acc.l[4] << 8);
    uint64_t t = (uint64_t)h0 + s[0];
    out[0] = (uint32_t)t;
    t = (t >> 32) + h1 + s[1];
    out[1] = (uint32_t)t;
    t = (t >> 32) + h2 + s[2];
    out[2] = (uint32_t)t;
    t = (t >> 32) + h3 + s[3];
    out[3] = (uint32_t)t;
}

}  // namespace jfsx
