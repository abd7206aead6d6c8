// jfsx_rsa.h -- RSA-OAEP (SHA-256) private-key decryption arithmetic for the
// batched key unwrap.
//
// Replaces, per object, rsaEncryptor.Decrypt = rsa.DecryptOAEP(sha256.New(),
// rand, privKey, wrapped, []byte("keys")) (pkg/object/encrypt.go:124-134,
// :207-210), which the reference runs on the host for every block it opens.
// The arithmetic is RSA with the CRT (RFC 8017 5.1.2 / Go's precomputed
// Dp, Dq, Qinv): m1 = c^dp mod p, m2 = c^dq mod q, h = qinv (m1 - m2) mod p,
// m = m2 + h q; then EME-OAEP decoding (RFC 8017 7.1.2) with SHA-256 as hash
// and MGF1 hash.  Primes are 1024-bit (RSA-2048, the size the reference docs
// use), in 32 little-endian 32-bit limbs; products use Montgomery CIOS.
// RSA-4096 (2048-bit primes) is the second and last size: the "RSA-4096"
// section at the end of this file, pinned by tests/test_rsa4096.py.
//
// The write side, rsaEncryptor.Encrypt = rsa.EncryptOAEP (encrypt.go:128-130),
// is the last part of this file: EME-OAEP encoding and the public operation
// EM^e mod n, modulo the 2048-bit n itself.
//
// Host/device portable: the includer defines JFSX_HD.  Every function is
// pinned on the CPU by tests/test_rsa.py (the unwrap) and tests/test_rsa_wrap.py
// (the wrap) against libcrypto's RSA-OAEP and a big-integer model.
//
// Constant time with respect to the private key and the decrypted message,
// as Go's rsa.DecryptOAEP is (crypto/internal/bigmod, subtle.ConstantTime*):
// the exponentiation (mod_exp28) runs a fixed 3-bit window over the full
// 1024-bit exponent length, always multiplies (digit 0 multiplies by the
// Montgomery one), and reads its window table by a masked scan of all 8 rows; the
// modular corrections, the CRT recombination and the OAEP checks select with
// masks instead of branching.  Branches remain only on public values: the
// ciphertext length and c >= n (Go rejects both before the private
// operation), and the final valid / invalid outcome.
#pragma once
#include <stdint.h>

// test hook: the host harness records every Montgomery product and every
// window-table read to check that the sequence does not depend on the exponent
#ifndef JFSX_RSA_TRACE
#define JFSX_RSA_TRACE(tag, v) ((void)0)
#endif
// a register barrier: the compiler cannot see through it, so a mask built from
// a secret digit cannot become a branch or an address (the GPU includer passes
// its VGPR form)
#ifndef JFSX_RSA_OPAQUE
#define JFSX_RSA_OPAQUE(x) asm volatile("" : "+r"(x))
#endif

namespace jfsx_rsa {

constexpr int kLimbs = 32;        // 1024-bit prime
constexpr int kL28 = 37;          // the same in 28-bit limbs (1036 bits), the GPU exponentiation's form
constexpr int kModBytes = 256;    // RSA-2048 modulus
constexpr int kHash = 32;         // SHA-256

// ---------------------------------------------------------------------------
// multi-precision helpers (little-endian limbs)
// ---------------------------------------------------------------------------
// -m^-1 mod 2^32 (m odd), Newton iteration
JFSX_HD uint32_t mont_inv32(uint32_t m0) {
    uint32_t x = m0;  // correct to 3 bits
    for (int i = 0; i < 5; i++) x *= 2u - m0 * x;
    return 0u - x;
}

// a >= b ?
JFSX_HD bool geq(const uint32_t *a, const uint32_t *b, int n) {
    for (int i = n - 1; i >= 0; i--)
        if (a[i] != b[i]) return a[i] > b[i];
    return true;
}

// a -= b, returns borrow
JFSX_HD uint32_t sub_in(uint32_t *a, const uint32_t *b, int n) {
    uint64_t br = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - br;
        a[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
    return (uint32_t)br;
}

// a += b, returns carry
JFSX_HD uint32_t add_in(uint32_t *a, const uint32_t *b, int n) {
    uint64_t c = 0;
    for (int i = 0; i < n; i++) {
        c += (uint64_t)a[i] + b[i];
        a[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}

// all-ones if x != 0, else 0 (no branch)
JFSX_HD uint32_t ct_nz(uint32_t x) { return 0u - ((x | (0u - x)) >> 31); }

// a >= b as an all-ones / zero mask, over all n limbs (no early exit)
JFSX_HD uint32_t ct_geq(const uint32_t *a, const uint32_t *b, int n) {
    uint64_t br = 0;
    for (int i = 0; i < n; i++) br = (((uint64_t)a[i] - b[i] - br) >> 32) & 1u;
    return (uint32_t)br - 1u;  // no borrow: a >= b
}

// a = mask ? a - b : a, over n limbs; returns the borrow of a - b
JFSX_HD uint32_t ct_sub_if(uint32_t *a, const uint32_t *b, int n, uint32_t mask) {
    uint64_t br = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - br;
        br = (d >> 32) & 1u;
        a[i] = (a[i] & ~mask) | ((uint32_t)d & mask);
    }
    return (uint32_t)br;
}

// a += mask & b over n limbs
JFSX_HD void ct_add_if(uint32_t *a, const uint32_t *b, int n, uint32_t mask) {
    uint64_t c = 0;
    for (int i = 0; i < n; i++) {
        c += (uint64_t)a[i] + (b[i] & mask);
        a[i] = (uint32_t)c;
        c >>= 32;
    }
}

// out = a b R^-1 mod m (R = 2^(32 NL): 2^1024, or 2^2048 for an RSA-4096
// prime), a, b < m; CIOS with one final subtract
template <int NL = kLimbs>
JFSX_HD void mont_mul(const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t minv, uint32_t *out) {
    constexpr int kLimbs = NL;  // the body below is written on this name
    JFSX_RSA_TRACE('M', 0);
    uint32_t t[kLimbs + 2];
#pragma unroll
    for (int j = 0; j < kLimbs + 2; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < kLimbs; i++) {
        const uint32_t ai = a[i];
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < kLimbs; j++) {
            c = (uint64_t)ai * b[j] + (c + t[j]);
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t[kLimbs];
        t[kLimbs] = (uint32_t)c;
        t[kLimbs + 1] = (uint32_t)(c >> 32);
        const uint32_t mi = t[0] * minv;
        c = ((uint64_t)mi * m[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < kLimbs; j++) {
            c = (uint64_t)mi * m[j] + (c + t[j]);
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[kLimbs];
        t[kLimbs - 1] = (uint32_t)c;
        t[kLimbs] = t[kLimbs + 1] + (uint32_t)(c >> 32);
    }
    // t < 2m: subtract m once if t >= m
    uint32_t d[kLimbs];
    uint64_t br = 0;
#pragma unroll
    for (int j = 0; j < kLimbs; j++) {
        const uint64_t x = (uint64_t)t[j] - m[j] - br;
        d[j] = (uint32_t)x;
        br = (x >> 32) & 1u;
    }
    const bool keep = t[kLimbs] == 0 && br;  // t < m
#pragma unroll
    for (int j = 0; j < kLimbs; j++) out[j] = keep ? t[j] : d[j];
}

// 2^bits mod m by doubling (host side, once per key); R^2 mod m by default
JFSX_HD void mont_r2(const uint32_t *m, uint32_t *r2, int bits = 2 * 32 * kLimbs) {
    uint32_t x[kLimbs + 1];
    for (int j = 0; j <= kLimbs; j++) x[j] = 0;
    x[0] = 1;
    for (int k = 0; k < bits; k++) {  // x = 2^k mod m
        uint32_t c = 0;
        for (int j = 0; j <= kLimbs; j++) {
            const uint32_t nc = x[j] >> 31;
            x[j] = (x[j] << 1) | c;
            c = nc;
        }
        if (x[kLimbs] || geq(x, m, kLimbs)) {
            const uint32_t b = sub_in(x, m, kLimbs);
            x[kLimbs] -= b;
        }
    }
    for (int j = 0; j < kLimbs; j++) r2[j] = x[j];
}

// big-endian bytes <-> limbs
JFSX_HD void from_be(const uint8_t *b, int nbytes, uint32_t *x, int nlimbs) {
    for (int j = 0; j < nlimbs; j++) x[j] = 0;
    for (int i = 0; i < nbytes; i++) {
        const int bit = 8 * (nbytes - 1 - i);
        x[bit >> 5] |= (uint32_t)b[i] << (bit & 31);
    }
}
JFSX_HD void to_be(const uint32_t *x, int nlimbs, uint8_t *b, int nbytes) {
    for (int i = 0; i < nbytes; i++) {
        const int bit = 8 * (nbytes - 1 - i);
        b[i] = (bit >> 5) < nlimbs ? (uint8_t)(x[bit >> 5] >> (bit & 31)) : 0;
    }
}

// ---------------------------------------------------------------------------
// SHA-256 (FIPS 180-4) and MGF1
// ---------------------------------------------------------------------------
JFSX_HD uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

JFSX_HD void sha256_block(uint32_t h[8], const uint8_t *p) {
    const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
        0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
        0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
        0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
        0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
        0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
        0xc67178f2};
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
        w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
        const uint32_t s0 = ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
        const uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
        const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// SHA-256 of a ‖ b (b may be empty), len(a) + len(b) < 2^29
JFSX_HD void sha256_2(const uint8_t *a, int la, const uint8_t *b, int lb, uint8_t out[32]) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t blk[64];
    const int total = la + lb;
    int pos = 0, fill = 0;
    // stream the message bytes, then 0x80, zeros, BE64 bit length
    const int padded = ((total + 9 + 63) / 64) * 64;
    for (int i = 0; i < padded; i++) {
        uint8_t v;
        if (i < la) v = a[i];
        else if (i < total) v = b[i - la];
        else if (i == total) v = 0x80;
        else if (i >= padded - 8) v = (uint8_t)(((uint64_t)total * 8) >> (8 * (padded - 1 - i)));
        else v = 0;
        blk[fill++] = v;
        if (fill == 64) {
            sha256_block(h, blk);
            fill = 0;
        }
        pos++;
    }
    (void)pos;
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)(h[i] >> 24);
        out[4 * i + 1] = (uint8_t)(h[i] >> 16);
        out[4 * i + 2] = (uint8_t)(h[i] >> 8);
        out[4 * i + 3] = (uint8_t)h[i];
    }
}

// dst[0..len) ^= MGF1-SHA256(seed, len)
JFSX_HD void mgf1_xor(const uint8_t *seed, int slen, uint8_t *dst, int len) {
    uint8_t ctr[4], hsh[32];
    for (int c = 0, done = 0; done < len; c++) {
        ctr[0] = (uint8_t)(c >> 24); ctr[1] = (uint8_t)(c >> 16); ctr[2] = (uint8_t)(c >> 8); ctr[3] = (uint8_t)c;
        sha256_2(seed, slen, ctr, 4, hsh);
        for (int i = 0; i < 32 && done < len; i++, done++) dst[done] ^= hsh[i];
    }
}

// EME-OAEP decode (RFC 8017 7.1.2 step 3) of em[0..k), lhash = SHA-256(label).
// Returns the message length and moves the message to em[0..len), or -1
// ("crypto/rsa: decryption error").  As Go's decryptOAEP: the leading zero
// byte, the label hash and the 0x01 separator are checked without branching
// on the data (the separator by a masked scan of the whole of DB), and one
// combined valid / invalid outcome is branched on at the end.
JFSX_HD int oaep_decode(uint8_t *em, int k, const uint8_t lhash[32]) {
    uint8_t *seed = em + 1, *db = em + 1 + kHash;
    const int dblen = k - kHash - 1;
    mgf1_xor(db, dblen, seed, kHash);
    mgf1_xor(seed, kHash, db, dblen);
    uint32_t bad = ct_nz(em[0]);
    for (int i = 0; i < kHash; i++) bad |= ct_nz((uint32_t)(db[i] ^ lhash[i]));
    uint32_t looking = ~0u, index = 0, invalid = 0;
    for (int i = kHash; i < dblen; i++) {
        const uint32_t is0 = ~ct_nz(db[i]), is1 = ~ct_nz((uint32_t)db[i] ^ 1u);
        index = (index & ~(looking & is1)) | ((uint32_t)i & looking & is1);
        invalid |= looking & ~is0 & ~is1;
        looking &= ~is1;
    }
    if (bad | invalid | looking) return -1;
    const int mlen = dblen - (int)index - 1;
    for (int j = 0; j < mlen; j++) em[j] = db[index + 1 + j];
    return mlen;
}

// ---------------------------------------------------------------------------
// key material in device memory (written by the host once per key)
// ---------------------------------------------------------------------------
struct Key {
    uint32_t n[2 * kLimbs];             // modulus p q (ciphertexts must be < n)
    uint32_t p[kLimbs], q[kLimbs];      // primes
    uint32_t dp[kLimbs], dq[kLimbs];    // CRT exponents
    uint32_t qinv[kLimbs];              // q^-1 mod p
    uint32_t r2p[kLimbs], r2q[kLimbs];  // R^2 mod p, R^2 mod q
    uint32_t r2p28[kLimbs], r2q28[kLimbs];  // R'^2 mod p, q for the GPU's 28-bit limbs (R' = 2^(28 kL28))
    uint32_t pinv, qinv32;              // -p^-1, -q^-1 mod 2^32
    int32_t dp_bits, dq_bits;           // exponent bit lengths
    uint8_t lhash[32];                  // SHA-256(label)
    // the key wrap's constants for n in 28-bit limbs (R'' = 2^(28 kN28), below)
    uint32_t r2n28[2 * kLimbs];         // R''^2 mod n
    uint32_t ninv28;                    // -n^-1 mod 2^28
};

// 2^bits mod m for an odd m of nl <= 4 kLimbs limbs (mont_r2 at another width;
// 4 kLimbs is the n of RSA-4096)
JFSX_HD void mont_r2_wide(const uint32_t *m, int nl, uint32_t *r2, int bits) {
    uint32_t x[4 * kLimbs + 1];
    for (int j = 0; j <= nl; j++) x[j] = 0;
    x[0] = 1;
    for (int k = 0; k < bits; k++) {  // x = 2^k mod m
        uint32_t c = 0;
        for (int j = 0; j <= nl; j++) {
            const uint32_t nc = x[j] >> 31;
            x[j] = (x[j] << 1) | c;
            c = nc;
        }
        if (x[nl] || geq(x, m, nl)) {
            const uint32_t b = sub_in(x, m, nl);
            x[nl] -= b;
        }
    }
    for (int j = 0; j < nl; j++) r2[j] = x[j];
}

JFSX_HD int bit_length(const uint32_t *x, int nlimbs) {
    for (int i = nlimbs - 1; i >= 0; i--)
        if (x[i]) return 32 * i + 32 - __builtin_clz(x[i]);
    return 0;
}

// Key from the CRT components (big-endian, 128 bytes each) and the OAEP
// label.  Returns false unless p, q are odd 1024-bit primes' shape.
JFSX_HD bool key_setup(Key &k, const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq,
                       const uint8_t *qinv, const uint8_t *label, int label_len) {
    const int nb = 4 * kLimbs;
    from_be(p, nb, k.p, kLimbs);
    from_be(q, nb, k.q, kLimbs);
    from_be(dp, nb, k.dp, kLimbs);
    from_be(dq, nb, k.dq, kLimbs);
    from_be(qinv, nb, k.qinv, kLimbs);
    if (!(k.p[0] & 1u) || !(k.q[0] & 1u) || bit_length(k.p, kLimbs) != 32 * kLimbs ||
        bit_length(k.q, kLimbs) != 32 * kLimbs)
        return false;
    k.pinv = mont_inv32(k.p[0]);
    k.qinv32 = mont_inv32(k.q[0]);
    mont_r2(k.p, k.r2p);
    mont_r2(k.q, k.r2q);
    mont_r2(k.p, k.r2p28, 2 * 28 * kL28);
    mont_r2(k.q, k.r2q28, 2 * 28 * kL28);
    k.dp_bits = bit_length(k.dp, kLimbs);
    k.dq_bits = bit_length(k.dq, kLimbs);
    if (k.dp_bits < 2 || k.dq_bits < 2) return false;
    for (int j = 0; j < 2 * kLimbs; j++) k.n[j] = 0;
    for (int i = 0; i < kLimbs; i++) {
        uint64_t c = 0;
        for (int j = 0; j < kLimbs; j++) {
            c = (uint64_t)k.p[i] * k.q[j] + (c + k.n[i + j]);
            k.n[i + j] = (uint32_t)c;
            c >>= 32;
        }
        k.n[i + kLimbs] = (uint32_t)c;
    }
    sha256_2(label, label_len, label, 0, k.lhash);
    mont_r2_wide(k.n, 2 * kLimbs, k.r2n28, 2 * 28 * 74);  // 74 = kN28
    k.ninv28 = mont_inv32(k.n[0]) & ((1u << 28) - 1);
    return true;
}

// c mod m for a 2048-bit c = hi R + lo (hi, lo < R): (hi R mod m) + lo, reduced
// (NL = 2 kLimbs: the same for a 4096-bit c and a 2048-bit m, R = 2^2048)
template <int NL = kLimbs>
JFSX_HD void reduce_2048(const uint32_t *c, const uint32_t *m, uint32_t minv, const uint32_t *r2, uint32_t *out) {
    constexpr int kLimbs = NL;
    uint32_t t[kLimbs + 1];
    mont_mul<NL>(c + kLimbs, r2, m, minv, t);  // hi R mod m (hi < R, r2 < m: CIOS bound holds)
    t[kLimbs] = add_in(t, c, kLimbs);      // + lo: < 3m since lo < R < 2m
    for (int rep = 0; rep < 2; rep++) {     // two masked corrections, always both
        const uint32_t ge = ct_nz(t[kLimbs]) | ct_geq(t, m, kLimbs);
        t[kLimbs] -= ct_sub_if(t, m, kLimbs, ge) & ge;
    }
    for (int j = 0; j < kLimbs; j++) out[j] = t[j];
}

// m = m2 + q (qinv (m1 - m2) mod p), the 2048-bit CRT recombination
// (NL = 2 kLimbs, K = KeyW: the 4096-bit one)
template <int NL = kLimbs, class K = Key>
JFSX_HD void crt(const K &k, const uint32_t *m1, const uint32_t *m2, uint32_t *m) {
    constexpr int kLimbs = NL;
    uint32_t t[kLimbs + 1], h[kLimbs], u[kLimbs];
    for (int j = 0; j < kLimbs; j++) t[j] = m2[j];
    t[kLimbs] = 0;
    ct_sub_if(t, k.p, kLimbs, ct_geq(t, k.p, kLimbs));  // m2 < q < 2p
    for (int j = 0; j < kLimbs; j++) u[j] = m1[j];
    const uint32_t neg = 0u - sub_in(u, t, kLimbs);     // (m1 - m2) mod p
    ct_add_if(u, k.p, kLimbs, neg);
    mont_mul<NL>(u, k.qinv, k.p, k.pinv, h);           // u qinv R^-1
    mont_mul<NL>(h, k.r2p, k.p, k.pinv, h);            // u qinv
    for (int j = 0; j < 2 * kLimbs; j++) m[j] = j < kLimbs ? m2[j] : 0;
    for (int i = 0; i < kLimbs; i++) {  // m += h q, carries run to the top every time
        uint64_t c = 0;
        for (int j = 0; j < kLimbs; j++) {
            c = (uint64_t)h[i] * k.q[j] + (c + m[i + j]);
            m[i + j] = (uint32_t)c;
            c >>= 32;
        }
        for (int j = i + kLimbs; j < 2 * kLimbs; j++) {
            c += m[j];
            m[j] = (uint32_t)c;
            c >>= 32;
        }
    }
}

// ---------------------------------------------------------------------------
// The exponentiation the unwrap runs, in 28-bit limbs.  With 32-bit limbs every
// multiply-add of the CIOS carries into the next (a GPU thread spends ~9K
// instructions per product on the multiply-adds and the moves that build
// their 64-bit addends).  With 37 limbs of 28 bits a product is < 2^56, so
// each column's 64-bit accumulator takes every row's two products with no
// carry at all (37 rows x 2 x 2^56 < 2^63): a row is 74 independent
// multiply-adds, and carries are resolved once per product.  R' = 2^(28 kL28);
// R'^2 mod p, q come with the key (Key::r2p28, r2q28).
// ---------------------------------------------------------------------------
constexpr uint32_t kM28 = (1u << 28) - 1;

// 32-bit limbs (kLimbs) <-> 28-bit limbs (kL28)
JFSX_HD void to28(const uint32_t *x, uint32_t *y) {
#pragma unroll
    for (int j = 0; j < kL28; j++) {
        const int bit = 28 * j, l = bit >> 5, o = bit & 31;
        uint64_t v = x[l];
        if (l + 1 < kLimbs) v |= (uint64_t)x[l + 1] << 32;
        y[j] = (uint32_t)(v >> o) & kM28;
    }
}
JFSX_HD void from28(const uint32_t *y, uint32_t *x) {
#pragma unroll
    for (int j = 0; j < kLimbs; j++) {
        const int bit = 32 * j, l = bit / 28, o = bit % 28;  // o <= 24: two limbs cover the word
        uint64_t v = (uint64_t)y[l] >> o;
        if (l + 1 < kL28) v |= (uint64_t)y[l + 1] << (28 - o);
        x[j] = (uint32_t)v;
    }
}

// out = a b R'^-1 mod m: a, b < m in normalized 28-bit limbs, minv = -m^-1
// mod 2^28; out normalized and < m (one masked final subtract)
JFSX_HD void mont_mul28(const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t minv, uint32_t *out) {
    JFSX_RSA_TRACE('M', 1);
    uint64_t acc[kL28];
#pragma unroll
    for (int j = 0; j < kL28; j++) acc[j] = 0;
#pragma unroll
    for (int i = 0; i < kL28; i++) {
        const uint32_t ai = a[i];
#pragma unroll
        for (int j = 0; j < kL28; j++) acc[j] += (uint64_t)ai * b[j];
        const uint32_t mi = ((uint32_t)acc[0] * minv) & kM28;
#pragma unroll
        for (int j = 0; j < kL28; j++) acc[j] += (uint64_t)mi * m[j];
        const uint64_t c = acc[0] >> 28;  // acc[0] is now a multiple of 2^28
#pragma unroll
        for (int j = 0; j < kL28 - 1; j++) acc[j] = acc[j + 1];
        acc[kL28 - 1] = 0;
        acc[0] += c;
    }
    // normalize (the value is < 2m < 2^1036), then subtract m unless t < m
    uint32_t t[kL28], d[kL28];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < kL28; j++) {
        c += acc[j];
        t[j] = (uint32_t)c & kM28;
        c >>= 28;
    }
    uint32_t br = 0;
#pragma unroll
    for (int j = 0; j < kL28; j++) {
        const uint32_t x = t[j] - m[j] - br;
        d[j] = x & kM28;
        br = x >> 31;
    }
    const uint32_t keep = 0u - br;  // t < m
#pragma unroll
    for (int j = 0; j < kL28; j++) out[j] = (t[j] & keep) | (d[j] & ~keep);
}

// The constant-time fixed-window schedule: kWDigits kWBits-bit digits of the
// exponent zero-extended to the prime's length, top first; per digit kWBits
// squarings and one multiply by tab[digit] (tab[0] = the Montgomery one),
// whatever the digit, the entry picked by a masked scan of all kWTab entries.
// One Montgomery multiply site in a loop over a step counter (the unrolled
// product is a few thousand instructions; one copy stays in the GPU's
// instruction cache), table writes at static indices only (so the table can
// live in registers), and the exponent only feeding masks through a register
// barrier.  A 3-bit window: the 8-entry table of 37-limb values fits the GPU
// thread's registers, a 16-entry one spills to scratch memory and the scan
// then reads it for every digit.
constexpr int kWBits = 3, kWTab = 1 << kWBits, kWDigits = (32 * kLimbs + kWBits - 1) / kWBits;

// digit d (0 = least significant) of e in kWBits-bit digits
JFSX_HD uint32_t w_digit(const uint32_t *e, int d) {
    const int b = kWBits * d, l = b >> 5, o = b & 31;
    uint64_t v = e[l];
    if (l + 1 < kLimbs) v |= (uint64_t)e[l + 1] << 32;
    return (uint32_t)(v >> o) & (kWTab - 1);
}

// x^e mod m (x < m; 32-bit limbs in and out), constant time in e
JFSX_HD void mod_exp28(const uint32_t *x32, const uint32_t *e, const uint32_t *m32, uint32_t minv32,
                       const uint32_t *r2_32, uint32_t *out32) {
    uint32_t m[kL28], x[kL28], r2[kL28];
    to28(m32, m);
    to28(x32, x);
    to28(r2_32, r2);
    const uint32_t minv = minv32 & kM28;
    uint32_t tab[kWTab][kL28];
    uint32_t acc[kL28], b[kL28];
    for (int w = 0; w < kWTab; w++)
        for (int j = 0; j < kL28; j++) tab[w][j] = 0;
    constexpr int kPer = kWBits + 1, kMain = kWTab + kPer * kWDigits;  // steps: table, digits, leave the domain
#pragma unroll 1
    for (int st = 0; st <= kMain; st++) {
        if (st == 0) {  // R' mod m = r2 * 1
#pragma unroll
            for (int j = 0; j < kL28; j++) acc[j] = r2[j], b[j] = j == 0;
        } else if (st == 1) {  // x R' mod m
#pragma unroll
            for (int j = 0; j < kL28; j++) acc[j] = x[j], b[j] = r2[j];
        } else if (st < kWTab) {  // tab[st] = tab[st - 1] * x R'
#pragma unroll
            for (int j = 0; j < kL28; j++) b[j] = tab[1][j];
        } else if (st < kMain) {
            const int r = st - kWTab;
            if (r % kPer < kWBits) {
#pragma unroll
                for (int j = 0; j < kL28; j++) b[j] = acc[j];
            } else {
                uint32_t idx = w_digit(e, kWDigits - 1 - r / kPer);
                JFSX_RSA_OPAQUE(idx);
#pragma unroll
                for (int j = 0; j < kL28; j++) b[j] = 0;
#pragma unroll
                for (uint32_t w = 0; w < (uint32_t)kWTab; w++) {
                    uint32_t msk = ~ct_nz(w ^ idx);
                    JFSX_RSA_OPAQUE(msk);
                    JFSX_RSA_TRACE('S', w);
#pragma unroll
                    for (int j = 0; j < kL28; j++) b[j] |= tab[w][j] & msk;
                }
            }
        } else {  // out of the Montgomery domain
#pragma unroll
            for (int j = 0; j < kL28; j++) b[j] = j == 0;
        }
        mont_mul28(acc, b, m, minv, acc);
        if (st < kWTab) {
#pragma unroll
            for (int w = 0; w < kWTab; w++)
#pragma unroll
                for (int j = 0; j < kL28; j++) tab[w][j] = st == w ? acc[j] : tab[w][j];
            if (st == kWTab - 1) {
#pragma unroll
                for (int j = 0; j < kL28; j++) acc[j] = tab[0][j];
            }
        }
    }
    from28(acc, out32);
}

// ---------------------------------------------------------------------------
// The same exponentiation on a PAIR of lanes (the GPU kernel's form).  One
// lane per exponentiation gives a batch of 16384 objects 32768 threads, 512
// waves: one wave on half of the chip's 1024 SIMDs, each issuing the whole
// ~4.4K-instruction product stream alone.  Two lanes per exponentiation split
// every product by columns -- lane 0 holds columns 0..18, lane 1 columns
// 19..37 (column 37 stays zero) -- so the batch is 1024 waves issuing about
// half the instructions each.  Per row of the product the lanes exchange four
// words: a_i from the lane holding it, the reduction multiplier m_i (lane 0
// computes it from column 0), and the 64-bit column 19 that moves into lane 0
// when the accumulator shifts down.  The final carry and borrow chains cross
// the lanes once each.  Same arithmetic, bounds and schedule as mod_exp28
// (one multiply site, masked table scan), so constant time in the exponent
// the same way.
//
// X is the exchange between the two lanes: X::hi (0 or 1), X::lo(v) / X::up(v)
// (v as held by lane 0 / lane 1, in both lanes), X::other(v) (the partner's
// v), X::tracing() (the lane that records the test trace).  The GPU kernel
// passes DPP moves; the CPU pin (tests/harness/rsa_host.cpp) runs the two
// lanes as two threads meeting at a barrier per exchange.
// ---------------------------------------------------------------------------
constexpr int kPC = (kL28 + 1) / 2;  // columns per lane (2 kPC = 38 >= kL28)

template <class X>
JFSX_HD uint64_t lo64(const X &x, uint64_t v) {
    return (uint64_t)x.lo((uint32_t)v) | (uint64_t)x.lo((uint32_t)(v >> 32)) << 32;
}
template <class X>
JFSX_HD uint64_t other64(const X &x, uint64_t v) {
    return (uint64_t)x.other((uint32_t)v) | (uint64_t)x.other((uint32_t)(v >> 32)) << 32;
}

// this lane's kPC limbs of a 28-bit-limb value f[0..kL28)
template <class X>
JFSX_HD void pair_pick(const X &x, const uint32_t *f, uint32_t *y) {
    const uint32_t up = 0u - x.hi;
#pragma unroll
    for (int j = 0; j < kPC; j++) y[j] = (f[j] & ~up) | ((kPC + j < kL28 ? f[kPC + j] : 0u) & up);
}

// out = a b R'^-1 mod m on the pair: a, b, m, out are this lane's kPC limbs
// (normalized); minv = -m^-1 mod 2^28
template <class X>
JFSX_HD void mont_mul28_pair(const X &x, const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t minv,
                             uint32_t *out) {
    if (x.tracing()) JFSX_RSA_TRACE('M', 2);
    const uint64_t low = (uint64_t)0 - (uint64_t)(x.hi ^ 1u);  // all-ones in lane 0
    uint64_t acc[kPC];
#pragma unroll
    for (int j = 0; j < kPC; j++) acc[j] = 0;
    // one row: + a_i b, + m_i m (m_i from lane 0's column 0), then the
    // columns move down one: column 0 leaves (its carry joins column 1) and
    // lane 1's first column becomes lane 0's last
    auto row = [&](uint32_t ai) {
#pragma unroll
        for (int j = 0; j < kPC; j++) acc[j] += (uint64_t)ai * b[j];
        const uint32_t mi = x.lo(((uint32_t)acc[0] * minv) & kM28);
#pragma unroll
        for (int j = 0; j < kPC; j++) acc[j] += (uint64_t)mi * m[j];
        const uint64_t c = acc[0] >> 28, s = other64(x, acc[0]);
#pragma unroll
        for (int j = 0; j < kPC - 1; j++) acc[j] = acc[j + 1];
        acc[kPC - 1] = s & low;
        acc[0] += c & low;
    };
#pragma unroll
    for (int r = 0; r < kPC; r++) row(x.lo(a[r]));
#pragma unroll
    for (int r = 0; r < kL28 - kPC; r++) row(x.up(a[r]));
    // normalize: each lane on its own, then lane 0's carry through lane 1
    uint32_t t[kPC], d[kPC];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < kPC; j++) {
        c += acc[j];
        t[j] = (uint32_t)c & kM28;
        c >>= 28;
    }
    c = lo64(x, c) & ~low;
#pragma unroll
    for (int j = 0; j < kPC; j++) {
        c += t[j];
        t[j] = (uint32_t)c & kM28;
        c >>= 28;
    }
    // t - m: lane 0's borrow first, then lane 1's chain from it
    uint32_t br = 0;
#pragma unroll
    for (int j = 0; j < kPC; j++) br = (t[j] - m[j] - br) >> 31;
    br = x.lo(br) & (0u - x.hi);
#pragma unroll
    for (int j = 0; j < kPC; j++) {
        const uint32_t v = t[j] - m[j] - br;
        d[j] = v & kM28;
        br = v >> 31;
    }
    const uint32_t keep = 0u - x.up(br);  // t < m
#pragma unroll
    for (int j = 0; j < kPC; j++) out[j] = (t[j] & keep) | (d[j] & ~keep);
}

// x^e mod m (x < m; 32-bit limbs in, out32 in both lanes), constant time in e:
// mod_exp28's schedule on the pair
template <class X>
JFSX_HD void mod_exp28_pair(const X &x, const uint32_t *x32, const uint32_t *e, const uint32_t *m32,
                            uint32_t minv32, const uint32_t *r2_32, uint32_t *out32) {
    uint32_t m[kPC], xv[kPC], r2[kPC];
    {
        uint32_t f[kL28];
        to28(m32, f);
        pair_pick(x, f, m);
        to28(x32, f);
        pair_pick(x, f, xv);
        to28(r2_32, f);
        pair_pick(x, f, r2);
    }
    const uint32_t minv = minv32 & kM28, one0 = x.hi ^ 1u;  // the Montgomery 1's low limb sits in lane 0
    uint32_t tab[kWTab][kPC];
    uint32_t acc[kPC], b[kPC];
    for (int w = 0; w < kWTab; w++)
        for (int j = 0; j < kPC; j++) tab[w][j] = 0;
    constexpr int kPer = kWBits + 1, kMain = kWTab + kPer * kWDigits;
#pragma unroll 1
    for (int st = 0; st <= kMain; st++) {
        if (st == 0) {
#pragma unroll
            for (int j = 0; j < kPC; j++) acc[j] = r2[j], b[j] = j == 0 ? one0 : 0u;
        } else if (st == 1) {
#pragma unroll
            for (int j = 0; j < kPC; j++) acc[j] = xv[j], b[j] = r2[j];
        } else if (st < kWTab) {
#pragma unroll
            for (int j = 0; j < kPC; j++) b[j] = tab[1][j];
        } else if (st < kMain) {
            const int r = st - kWTab;
            if (r % kPer < kWBits) {
#pragma unroll
                for (int j = 0; j < kPC; j++) b[j] = acc[j];
            } else {
                uint32_t idx = w_digit(e, kWDigits - 1 - r / kPer);
                JFSX_RSA_OPAQUE(idx);
#pragma unroll
                for (int j = 0; j < kPC; j++) b[j] = 0;
#pragma unroll
                for (uint32_t w = 0; w < (uint32_t)kWTab; w++) {
                    uint32_t msk = ~ct_nz(w ^ idx);
                    JFSX_RSA_OPAQUE(msk);
                    if (x.tracing()) JFSX_RSA_TRACE('S', w);
#pragma unroll
                    for (int j = 0; j < kPC; j++) b[j] |= tab[w][j] & msk;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kPC; j++) b[j] = j == 0 ? one0 : 0u;
        }
        mont_mul28_pair(x, acc, b, m, minv, acc);
        if (st < kWTab) {
#pragma unroll
            for (int w = 0; w < kWTab; w++)
#pragma unroll
                for (int j = 0; j < kPC; j++) tab[w][j] = st == w ? acc[j] : tab[w][j];
            if (st == kWTab - 1) {
#pragma unroll
                for (int j = 0; j < kPC; j++) acc[j] = tab[0][j];
            }
        }
    }
    // both halves of the result in both lanes, back to 32-bit limbs
    uint32_t f[2 * kPC];
    const uint32_t up = 0u - x.hi;
#pragma unroll
    for (int j = 0; j < kPC; j++) {
        const uint32_t o = x.other(acc[j]);
        f[j] = (acc[j] & ~up) | (o & up);
        f[kPC + j] = (o & ~up) | (acc[j] & up);
    }
    from28(f, out32);
}

// One whole unwrap on one thread (the CPU pin; the GPU splits it into the
// two half exponentiations and a finish kernel): ct = k bytes, big-endian.
// Returns the message length (msg in em[0..len)) or -1.
JFSX_HD int decrypt(const Key &k, const uint8_t *ct, uint8_t em[kModBytes]) {
    uint32_t c[2 * kLimbs], m1[kLimbs], m2[kLimbs], m[2 * kLimbs], x[kLimbs];
    from_be(ct, kModBytes, c, 2 * kLimbs);
    if (geq(c, k.n, 2 * kLimbs)) return -1;
    reduce_2048(c, k.p, k.pinv, k.r2p, x);
    mod_exp28(x, k.dp, k.p, k.pinv, k.r2p28, m1);
    reduce_2048(c, k.q, k.qinv32, k.r2q, x);
    mod_exp28(x, k.dq, k.q, k.qinv32, k.r2q28, m2);
    crt(k, m1, m2, m);
    to_be(m, 2 * kLimbs, em, kModBytes);
    return oaep_decode(em, kModBytes, k.lhash);
}

// ---------------------------------------------------------------------------
// The key wrap, the write side: rsaEncryptor.Encrypt = rsa.EncryptOAEP(
// sha256.New(), rand, &privKey.PublicKey, key, []byte("keys"))
// (pkg/object/encrypt.go:128-130, called at :169).  EME-OAEP encoding with a
// seed the caller draws, then EM^e mod n with the public exponent: no CRT, so
// the arithmetic is modulo the 2048-bit n itself, in kN28 = 74 limbs of 28
// bits with R'' = 2^(28 kN28).
//
// The lazy column accumulators of mont_mul28 carry over, with a tighter bound:
// a column takes at most kN28 rows of two products, each at most (2^28 - 1)^2,
// so at most 148 (2^28 - 1)^2 < 2^63.21, plus one carry below 2^37 when it
// reaches column 0: it fits an unsigned 64-bit word with under one bit to
// spare, and only because both operands and the modulus are normalized limbs
// (<= 2^28 - 1) of values < n.  The products' results are therefore always
// normalized and < n (one masked final subtract), never "< 2n".
//
// e is public (Go's checkPub takes 2 <= e <= 2^31 - 1): its bits steer a
// plain left-to-right square-and-multiply.  The operands (the encoded data
// key) steer nothing: no branch and no address depends on them.
// ---------------------------------------------------------------------------
constexpr int kNLimbs = 2 * kLimbs;                    // n in 32-bit limbs
constexpr int kN28 = 74;                               // and in 28-bit limbs (2072 bits)
constexpr int kMaxMsg = kModBytes - 2 * kHash - 2;     // OAEP capacity: 190 bytes
constexpr uint32_t kMinE = 2, kMaxE = 0x7FFFFFFFu;     // Go's checkPub

// EME-OAEP encode (RFC 8017 7.1.1 step 2, Go's EncryptOAEP): em (k bytes) = 00 ‖
// maskedSeed ‖ maskedDB with DB = lhash ‖ PS ‖ 01 ‖ msg; len <= k - 66.  Only
// the length places bytes; the message and seed bytes are moved and hashed.
JFSX_HD void oaep_encode(const uint8_t lhash[32], const uint8_t *msg, int len, const uint8_t *seed, uint8_t *em,
                         int k = kModBytes) {
    uint8_t *ms = em + 1, *db = em + 1 + kHash;
    const int dblen = k - kHash - 1, sep = dblen - 1 - len;
    em[0] = 0;
    for (int i = 0; i < kHash; i++) db[i] = lhash[i], ms[i] = seed[i];
    for (int i = kHash; i < dblen; i++) db[i] = i < sep ? 0 : i == sep ? 1 : msg[i - sep - 1];
    mgf1_xor(ms, kHash, db, dblen);
    mgf1_xor(db, dblen, ms, kHash);
}

// 28-bit limb j of a value in nl32 32-bit limbs (zero past its end)
JFSX_HD uint32_t limb28(const uint32_t *x, int nl32, int j) {
    const int bit = 28 * j, l = bit >> 5, o = bit & 31;
    uint64_t v = l < nl32 ? x[l] : 0u;
    if (l + 1 < nl32) v |= (uint64_t)x[l + 1] << 32;
    return (uint32_t)(v >> o) & kM28;
}
// n28 28-bit limbs -> n32 32-bit limbs (from28 at another width)
JFSX_HD void from28_wide(const uint32_t *y, int n28, uint32_t *x, int n32) {
#pragma unroll
    for (int j = 0; j < n32; j++) {
        const int bit = 32 * j, l = bit / 28, o = bit % 28;
        uint64_t v = l < n28 ? (uint64_t)y[l] >> o : 0u;
        if (l + 1 < n28) v |= (uint64_t)y[l + 1] << (28 - o);
        x[j] = (uint32_t)v;
    }
}

// out = a b R''^-1 mod m for a 2048-bit odd m: a, b < m in kN28 normalized
// limbs, minv = -m^-1 mod 2^28; out normalized and < m.  mont_mul28 at twice
// the width; the accumulator bound is the one stated above.
//
// N = kN28W = 148 is the same modulo a 4096-bit m (RSA-4096's n).  There a
// column would take up to 148 rows of two products, 296 (2^28 - 1)^2 > 2^64:
// the lazy accumulators alone overflow.  So after kSweepAt = 74 rows the
// carries are resolved once, in place (every column back below 2^28, plus a
// carry below 2^37 in the next): no column then holds more than 74 rows' worth
// before the sweep nor more than 74 rows' worth and 2^38 after it, the bound
// above.  The sweep moves bits between columns and leaves the value alone, so
// the reduction multipliers and the result are what they are without it.
constexpr int kSweepAt = 74;
constexpr int n32_of(int n28) { return 28 * n28 / 2048 * 64; }  // 32-bit limbs of the modulus: 74 -> 64, 148 -> 128
constexpr bool needs_sweep(int n28) { return 2 * n28 >= 256; }  // 2 n28 (2^28 - 1)^2 + 2^38 < 2^64 below that

template <int N = 74>
JFSX_HD void mont_mul28_wide(const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t minv, uint32_t *out) {
    constexpr int kN28 = N;  // the body below is written on this name
    JFSX_RSA_TRACE('M', 3);
    uint64_t acc[kN28];
#pragma unroll
    for (int j = 0; j < kN28; j++) acc[j] = 0;
#pragma unroll
    for (int i = 0; i < kN28; i++) {
        if (needs_sweep(N) && i == kSweepAt) {
            uint64_t c = 0;
            for (int j = 0; j < kN28; j++) {
                c += acc[j];
                acc[j] = c & kM28;
                c >>= 28;
            }  // c == 0: the running value is below 2 m < 2^(28 N)
        }
        const uint32_t ai = a[i];
#pragma unroll
        for (int j = 0; j < kN28; j++) acc[j] += (uint64_t)ai * b[j];
        const uint32_t mi = ((uint32_t)acc[0] * minv) & kM28;
#pragma unroll
        for (int j = 0; j < kN28; j++) acc[j] += (uint64_t)mi * m[j];
        const uint64_t c = acc[0] >> 28;
#pragma unroll
        for (int j = 0; j < kN28 - 1; j++) acc[j] = acc[j + 1];
        acc[kN28 - 1] = 0;
        acc[0] += c;
    }
    // the value is < m (1 + m / R'') < 2m: normalize, then subtract m unless t < m
    uint32_t t[kN28], d[kN28];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < kN28; j++) {
        c += acc[j];
        t[j] = (uint32_t)c & kM28;
        c >>= 28;
    }
    uint32_t br = 0;
#pragma unroll
    for (int j = 0; j < kN28; j++) {
        const uint32_t x = t[j] - m[j] - br;
        d[j] = x & kM28;
        br = x >> 31;
    }
    const uint32_t keep = 0u - br;  // t < m
#pragma unroll
    for (int j = 0; j < kN28; j++) out[j] = (t[j] & keep) | (d[j] & ~keep);
}

// The public exponentiation's schedule, shared by both forms below: one
// product to enter the Montgomery domain, then for every bit of e under the
// top one a squaring and, where the bit is set, a multiply by x R''; one
// product to leave: bit_length(e) + popcount(e) products.  One multiply site
// in a loop (one copy of the unrolled product in the instruction cache).
struct PubSchedule {
    enum Phase { kEnter, kSquare, kMultiply, kLeave };
    uint32_t e;
    int bit;    // the bit of e being worked on
    int phase;  // the product about to run
};
JFSX_HD PubSchedule pub_begin(uint32_t e) { return PubSchedule{e, 31 - __builtin_clz(e), PubSchedule::kEnter}; }
// moves to the step after the current one; false once kLeave has run
JFSX_HD bool pub_next(PubSchedule &s) {
    if (s.phase == PubSchedule::kLeave) return false;
    if (s.phase == PubSchedule::kSquare && ((s.e >> s.bit) & 1u)) {
        s.phase = PubSchedule::kMultiply;
    } else {
        s.bit--;
        s.phase = s.bit >= 0 ? PubSchedule::kSquare : PubSchedule::kLeave;
    }
    return true;
}

// x^e mod m (x < m, m odd, 2048 bits, or 4096 bits for N = kN28W; 32-bit limbs
// in and out), kMinE <= e
template <int N = 74>
JFSX_HD void mod_exp28_pub(const uint32_t *x32, uint32_t e, const uint32_t *m32, uint32_t minv, const uint32_t *r2_32,
                           uint32_t *out32) {
    constexpr int kN28 = N, kNLimbs = n32_of(N);
    uint32_t m[kN28], xr[kN28], acc[kN28], b[kN28];
    for (int j = 0; j < kN28; j++) {
        m[j] = limb28(m32, kNLimbs, j);
        acc[j] = limb28(x32, kNLimbs, j);
        b[j] = limb28(r2_32, kNLimbs, j);
        xr[j] = 0;
    }
    PubSchedule s = pub_begin(e);
#pragma unroll 1
    do {
        if (s.phase == PubSchedule::kSquare) {
            for (int j = 0; j < kN28; j++) b[j] = acc[j];
        } else if (s.phase == PubSchedule::kMultiply) {
            for (int j = 0; j < kN28; j++) b[j] = xr[j];
        } else if (s.phase == PubSchedule::kLeave) {
            for (int j = 0; j < kN28; j++) b[j] = j == 0;
        }
        mont_mul28_wide<N>(acc, b, m, minv, acc);
        if (s.phase == PubSchedule::kEnter)
            for (int j = 0; j < kN28; j++) xr[j] = acc[j];
    } while (pub_next(s));
    from28_wide(acc, kN28, out32, kNLimbs);
}

// ---------------------------------------------------------------------------
// The same on a QUAD of lanes (the GPU kernel's form): the four lanes of one
// DPP quad share one exponentiation, lane L holding columns kQC L .. kQC L +
// 18 (4 kQC = 76 >= kN28; columns 74 and 75 stay zero).  Per row of the
// product the lanes exchange a_i (a broadcast from the lane holding it), the
// reduction multiplier m_i (a broadcast of lane 0's), and the 64-bit column
// that moves into the lane below when the accumulator shifts down.  The
// carries of the normalization ripple through lanes 1, 2, 3 in turn; the
// final subtract's borrow crosses the lanes as one (generate, propagate) pair
// per lane.  There is no window table: the live state is acc, x R'', m, the
// operand and the 19 column accumulators.
//
// X is the exchange inside the quad: X::lane (0..3), X::from<K>(v) (lane K's
// v, in all lanes), X::next(v) / X::prev(v) (v of the lane above / below,
// cyclically), X::tracing().  The GPU kernel passes DPP quad_perm moves; the
// CPU pin (tests/harness/rsa_wrap_host.cpp) runs four threads and a barrier.
// ---------------------------------------------------------------------------
constexpr int kQC = (kN28 + 3) / 4;  // columns per lane

template <class X>
JFSX_HD uint64_t next64(const X &x, uint64_t v) {
    return (uint64_t)x.next((uint32_t)v) | (uint64_t)x.next((uint32_t)(v >> 32)) << 32;
}
template <class X>
JFSX_HD uint64_t prev64(const X &x, uint64_t v) {
    return (uint64_t)x.prev((uint32_t)v) | (uint64_t)x.prev((uint32_t)(v >> 32)) << 32;
}

// a compile-time number as an argument (of the generic lambdas below)
template <int V>
struct Const {
    static constexpr int value = V;
};

// f(Const<I>{}) for I = B .. E - 1, in order
template <int B, int E, class F>
JFSX_HD void static_for(F &&f) {
    if constexpr (B < E) {
        f(Const<B>{});
        static_for<B + 1, E>(f);
    }
}

// t = the normalized limbs of the value in the quad's QC column accumulators
// per lane: each lane on its own, then the carry out of lane k - 1 (below
// 2^37) through lane k, for k = 1, 2, 3
template <int QC, class X>
JFSX_HD void quad_normalize(const X &x, const uint64_t *acc, uint32_t *t) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < QC; j++) {
        c += acc[j];
        t[j] = (uint32_t)c & kM28;
        c >>= 28;
    }
#pragma unroll
    for (uint32_t k = 1; k < 4; k++) {
        uint64_t ci = prev64(x, c) & ((uint64_t)0 - (uint64_t)(x.lane == k));
#pragma unroll
        for (int j = 0; j < QC; j++) {
            ci += t[j];
            t[j] = (uint32_t)ci & kM28;
            ci >>= 28;
        }
        c += ci;
    }
}

// out = t >= m ? t - m : t on the quad's normalized limbs, by a mask: every
// lane's borrow out for a borrow in of 0 (g) and of 1 (p), then the chain over
// the four (g, p) pairs, the same in all lanes
template <int QC, class X>
JFSX_HD void quad_sub_if_geq(const X &x, const uint32_t *t, const uint32_t *m, uint32_t *out) {
    uint32_t d[QC];
    uint32_t g = 0, p = 1;
#pragma unroll
    for (int j = 0; j < QC; j++) {
        g = (t[j] - m[j] - g) >> 31;
        p = (t[j] - m[j] - p) >> 31;
    }
    uint32_t br = 0, bin = 0;
    br = x.template from<0>(g) | (x.template from<0>(p) & br);
    bin |= br & (0u - (uint32_t)(x.lane == 1u));
    br = x.template from<1>(g) | (x.template from<1>(p) & br);
    bin |= br & (0u - (uint32_t)(x.lane == 2u));
    br = x.template from<2>(g) | (x.template from<2>(p) & br);
    bin |= br & (0u - (uint32_t)(x.lane == 3u));
    br = x.template from<3>(g) | (x.template from<3>(p) & br);
#pragma unroll
    for (int j = 0; j < QC; j++) {
        const uint32_t v = t[j] - m[j] - bin;
        d[j] = v & kM28;
        bin = v >> 31;
    }
    const uint32_t keep = 0u - br;  // t < m
#pragma unroll
    for (int j = 0; j < QC; j++) out[j] = (t[j] & keep) | (d[j] & ~keep);
}

// out = a b R''^-1 mod m on the quad: a, b, m, out are this lane's QC = (N +
// 3) / 4 limbs (normalized, b < m, a < m or at least a < R'' = 2^(28 N): the
// value before the last subtract is below b + m either way); the accumulator
// bound is mont_mul28_wide's, and so is the carry sweep at N = kN28W = 4 x 37,
// which falls between the rows of lane 1 and lane 2 (kSweepAt = 2 QC there)
// and hands each lane's carry out to the first column of the lane above
template <class X, int N = 74>
JFSX_HD void mont_mul28_quad(const X &x, const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t minv,
                             uint32_t *out) {
    constexpr int kN28 = N, kQC = (N + 3) / 4;  // the body below is written on these names
    static_assert(!needs_sweep(N) || kSweepAt == 2 * kQC, "the sweep sits between two lanes' rows");
    if (x.tracing()) JFSX_RSA_TRACE('M', 4);
    const uint64_t first = (uint64_t)0 - (uint64_t)(x.lane == 0u), inner = (uint64_t)0 - (uint64_t)(x.lane != 3u);
    uint64_t acc[kQC];
#pragma unroll
    for (int j = 0; j < kQC; j++) acc[j] = 0;
    // one row: + a_i b, + m_i m (m_i from lane 0's column 0), then the columns
    // move down one: column 0 leaves (its carry joins column 1) and every
    // lane's first column becomes the last of the lane below
    auto row = [&](uint32_t ai) {
#pragma unroll
        for (int j = 0; j < kQC; j++) acc[j] += (uint64_t)ai * b[j];
        const uint32_t mi = x.template from<0>(((uint32_t)acc[0] * minv) & kM28);
#pragma unroll
        for (int j = 0; j < kQC; j++) acc[j] += (uint64_t)mi * m[j];
        const uint64_t c = acc[0] >> 28, s = next64(x, acc[0]);
#pragma unroll
        for (int j = 0; j < kQC - 1; j++) acc[j] = acc[j + 1];
        acc[kQC - 1] = s & inner;
        acc[0] += c & first;
    };
    if constexpr (!needs_sweep(N)) {
        // 74 rows, all unrolled: the shifts are register renaming
#pragma unroll
        for (int r = 0; r < kQC; r++) row(x.template from<0>(a[r]));
#pragma unroll
        for (int r = 0; r < kQC; r++) row(x.template from<1>(a[r]));
#pragma unroll
        for (int r = 0; r < kQC; r++) row(x.template from<2>(a[r]));
#pragma unroll
        for (int r = 0; r < kN28 - 3 * kQC; r++) row(x.template from<3>(a[r]));
    } else {
        // 148 rows of 74 multiply-adds unrolled would be several times the
        // instruction cache: a loop over the four lanes' rows instead, one
        // lane's 37 rows unrolled in its body.  A row's limb of a comes from
        // lane 0 every time: after a lane's rows every lane takes over the
        // limbs of the lane above it (all indices static: an indexed read
        // would put a into scratch memory), and over 37 rows every column has
        // moved down by one whole lane, into the registers it started from.
        static_assert(N == 4 * kQC, "whole lanes of rows");
        uint32_t ar[kQC];
#pragma unroll
        for (int j = 0; j < kQC; j++) ar[j] = a[j];
#pragma unroll 1
        for (int g = 0; g < 4; g++) {
            if (g == 2) {
                // the carry sweep; lane 3's carry out is zero: the running
                // value is below 2 m, and m ends inside lane 3's columns
                uint64_t c = 0;
#pragma unroll
                for (int j = 0; j < kQC; j++) {
                    c += acc[j];
                    acc[j] = c & kM28;
                    c >>= 28;
                }
                acc[0] += prev64(x, c) & ~first;
            }
            // (unrolled by the template: 37 rows are past what the
            // compiler unrolls on a pragma's word)
            static_for<0, kQC>([&](auto r) { row(x.template from<0>(ar[decltype(r)::value])); });
#pragma unroll
            for (int r = 0; r < kQC; r++) ar[r] = x.next(ar[r]);
        }
    }
    uint32_t t[kQC];
    quad_normalize<kQC>(x, acc, t);
    quad_sub_if_geq<kQC>(x, t, m, out);
}

// x^e mod m on the quad (x < m; 32-bit limbs in, this lane's kQC normalized
// 28-bit limbs of the result out): mod_exp28_pub's schedule.  With park (kQC
// words of memory of this lane's own) x R'' waits there between the product
// that makes it and the multiplies that take it, not in registers: at 37
// columns the registers do not hold it next to acc, the operand, m and the
// column accumulators.  The addresses are the lane's, whatever the data.
template <class X, int N = 74>
JFSX_HD void mod_exp28_pub_quad_lane(const X &x, const uint32_t *x32, uint32_t e, const uint32_t *m32, uint32_t minv,
                                     const uint32_t *r2_32, uint32_t *acc, uint32_t *park = nullptr) {
    constexpr int kQC = (N + 3) / 4, kNLimbs = n32_of(N);  // 74: 19, 64; kN28W: 37, 128
    uint32_t m[kQC], xr[kQC], b[kQC];
    const uint32_t one0 = x.lane == 0u;  // the Montgomery 1's low limb sits in lane 0
#pragma unroll
    for (int j = 0; j < kQC; j++) {
        const int col = kQC * (int)x.lane + j;  // limb28 gives zero for columns 74, 75
        m[j] = limb28(m32, kNLimbs, col);
        acc[j] = limb28(x32, kNLimbs, col);
        b[j] = limb28(r2_32, kNLimbs, col);
        xr[j] = 0;
    }
    PubSchedule s = pub_begin(e);
#pragma unroll 1
    do {
        if (s.phase == PubSchedule::kSquare) {
#pragma unroll
            for (int j = 0; j < kQC; j++) b[j] = acc[j];
        } else if (s.phase == PubSchedule::kMultiply) {
#pragma unroll
            for (int j = 0; j < kQC; j++) b[j] = park ? park[j] : xr[j];
        } else if (s.phase == PubSchedule::kLeave) {
#pragma unroll
            for (int j = 0; j < kQC; j++) b[j] = j == 0 ? one0 : 0u;
        }
        mont_mul28_quad<X, N>(x, acc, b, m, minv, acc);
        if (s.phase == PubSchedule::kEnter) {
#pragma unroll
            for (int j = 0; j < kQC; j++) {
                if (park) park[j] = acc[j];
                else xr[j] = acc[j];
            }
        }
    } while (pub_next(s));
}

// the same with the whole result in every lane, as 32-bit limbs
template <class X, int N = 74>
JFSX_HD void mod_exp28_pub_quad(const X &x, const uint32_t *x32, uint32_t e, const uint32_t *m32, uint32_t minv,
                                const uint32_t *r2_32, uint32_t *out32) {
    constexpr int kN28 = N, kQC = (N + 3) / 4, kNLimbs = n32_of(N);
    uint32_t acc[kQC];
    mod_exp28_pub_quad_lane<X, N>(x, x32, e, m32, minv, r2_32, acc);
    // all four quarters of the result in every lane, back to 32-bit limbs
    uint32_t f[4 * kQC];
#pragma unroll
    for (int j = 0; j < kQC; j++) {
        f[j] = x.template from<0>(acc[j]);
        f[kQC + j] = x.template from<1>(acc[j]);
        f[2 * kQC + j] = x.template from<2>(acc[j]);
        f[3 * kQC + j] = x.template from<3>(acc[j]);
    }
    from28_wide(f, kN28, out32, kNLimbs);
}

// One whole wrap on one thread (the CPU pin; the GPU splits it into an encode
// kernel and the quad exponentiation): ct = EM^e mod n, kModBytes big-endian
// bytes, left-padded with zeros.  Returns 0, or -1 for Go's "message too long
// for RSA key size" (ct all zero).  EM's first byte is zero, so EM < 2^2040 < n.
JFSX_HD int encrypt(const Key &k, uint32_t e, const uint8_t *msg, int len, const uint8_t *seed,
                    uint8_t ct[kModBytes]) {
    if (len < 0 || len > kMaxMsg) {
        for (int i = 0; i < kModBytes; i++) ct[i] = 0;
        return -1;
    }
    uint8_t em[kModBytes];
    oaep_encode(k.lhash, msg, len, seed, em);
    uint32_t x[kNLimbs], r[kNLimbs];
    from_be(em, kModBytes, x, kNLimbs);
    mod_exp28_pub(x, e, k.n, k.ninv28, k.r2n28, r);
    to_be(r, kNLimbs, ct, kModBytes);
    return 0;
}

// ---------------------------------------------------------------------------
// RSA-4096: the second and last key size (`juicefs format --encrypt-rsa-key`
// with a 4096-bit key; 3072-bit and every other size stay refused).  k = 512
// bytes, the primes are 2048 bits: 64 limbs of 32 bits, kN28 = 74 limbs of 28,
// which is the width the wrap's quad product already has, so a CRT half is a
// fixed-window exponentiation over mont_mul28_quad<X, 74> with the 8-entry
// table in registers.  n is 128 limbs of 32 bits, kN28W = 148 of 28, 37
// columns per lane of the quad (mont_mul28_quad<X, 148>, with the carry sweep).
// The CRT recombination and the one-lane pins run the 32-bit CIOS at 64 limbs.
// ---------------------------------------------------------------------------
constexpr int kLimbsW = 2 * kLimbs;                      // 2048-bit prime
constexpr int kNLimbsW = 2 * kLimbsW;                    // 4096-bit n
constexpr int kModBytesW = 4 * kNLimbsW;                 // 512
// n in 28-bit limbs: 147 hold it (4116 bits); 148 = 4 x 37 are taken, the top
// one always zero, so that every lane of the quad has 37 whole columns and the
// product 37 whole rows per lane (R'' = 2^(28 * 148))
constexpr int kN28W = 148;
constexpr int kQCW = (kN28W + 3) / 4;                    // 37 columns per lane
constexpr int kMaxMsgW = kModBytesW - 2 * kHash - 2;     // OAEP capacity: 446 bytes
constexpr int kWDigitsW = (32 * kLimbsW + kWBits - 1) / kWBits;  // 683 window digits
constexpr int kHalfBits = 32 * kLimbsW;                  // the input reduction splits c = hi 2^2048 + lo

struct KeyW {
    uint32_t n[kNLimbsW];
    uint32_t p[kLimbsW], q[kLimbsW];
    uint32_t dp[kLimbsW], dq[kLimbsW];
    uint32_t qinv[kLimbsW];
    uint32_t r2p[kLimbsW], r2q[kLimbsW];      // 2^4096 mod p, q: the 32-bit CIOS (CRT, one-lane reduction)
    uint32_t r2p28[kLimbsW], r2q28[kLimbsW];  // R'^2 mod p, q, R' = 2^(28 kN28): the exponentiation
    uint32_t rxp[kLimbsW], rxq[kLimbsW];      // 2^2048 R' mod p, q: the quad's input reduction
    uint32_t pinv, qinv32;                    // -p^-1, -q^-1 mod 2^32
    int32_t dp_bits, dq_bits;
    uint8_t lhash[32];
    uint32_t r2n28[kNLimbsW];                 // R''^2 mod n, R'' = 2^(28 kN28W)
    uint32_t ninv28;                          // -n^-1 mod 2^28
};

// KeyW from the CRT components (big-endian, 256 bytes each): key_setup's
// checks at this width (odd primes with bit 2047 set, dp, dq >= 2)
JFSX_HD bool key_setup_w(KeyW &k, const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq,
                         const uint8_t *qinv, const uint8_t *label, int label_len) {
    constexpr int L = kLimbsW, nb = 4 * L;
    from_be(p, nb, k.p, L);
    from_be(q, nb, k.q, L);
    from_be(dp, nb, k.dp, L);
    from_be(dq, nb, k.dq, L);
    from_be(qinv, nb, k.qinv, L);
    if (!(k.p[0] & 1u) || !(k.q[0] & 1u) || bit_length(k.p, L) != 32 * L || bit_length(k.q, L) != 32 * L) return false;
    k.dp_bits = bit_length(k.dp, L);
    k.dq_bits = bit_length(k.dq, L);
    if (k.dp_bits < 2 || k.dq_bits < 2) return false;
    k.pinv = mont_inv32(k.p[0]);
    k.qinv32 = mont_inv32(k.q[0]);
    mont_r2_wide(k.p, L, k.r2p, 2 * 32 * L);
    mont_r2_wide(k.q, L, k.r2q, 2 * 32 * L);
    mont_r2_wide(k.p, L, k.r2p28, 2 * 28 * kN28);
    mont_r2_wide(k.q, L, k.r2q28, 2 * 28 * kN28);
    mont_r2_wide(k.p, L, k.rxp, kHalfBits + 28 * kN28);
    mont_r2_wide(k.q, L, k.rxq, kHalfBits + 28 * kN28);
    for (int j = 0; j < 2 * L; j++) k.n[j] = 0;
    for (int i = 0; i < L; i++) {
        uint64_t c = 0;
        for (int j = 0; j < L; j++) {
            c = (uint64_t)k.p[i] * k.q[j] + (c + k.n[i + j]);
            k.n[i + j] = (uint32_t)c;
            c >>= 32;
        }
        k.n[i + L] = (uint32_t)c;
    }
    sha256_2(label, label_len, label, 0, k.lhash);
    mont_r2_wide(k.n, kNLimbsW, k.r2n28, 2 * 28 * kN28W);
    k.ninv28 = mont_inv32(k.n[0]) & kM28;
    return true;
}

// digit d (0 = least significant) of the nl-limb e in kWBits-bit digits
JFSX_HD uint32_t w_digit_n(const uint32_t *e, int nl, int d) {
    const int b = kWBits * d, l = b >> 5, o = b & 31;
    uint64_t v = e[l];
    if (l + 1 < nl) v |= (uint64_t)e[l + 1] << 32;
    return (uint32_t)(v >> o) & (kWTab - 1);
}

// x^e mod m for a 2048-bit m and a 2048-bit e on ONE lane (x < m; 32-bit limbs
// in and out): mod_exp28 over mont_mul28_wide.  The CPU pin of the whole
// unwrap runs it; on the GPU its table would not fit the registers, and the
// kernel runs the quad form below.
JFSX_HD void mod_exp28_priv_wide(const uint32_t *x32, const uint32_t *e, const uint32_t *m32, uint32_t minv32,
                                 const uint32_t *r2_32, uint32_t *out32) {
    constexpr int L = kN28;
    uint32_t m[L], x[L], r2[L];
    for (int j = 0; j < L; j++)
        m[j] = limb28(m32, kLimbsW, j), x[j] = limb28(x32, kLimbsW, j), r2[j] = limb28(r2_32, kLimbsW, j);
    const uint32_t minv = minv32 & kM28;
    uint32_t tab[kWTab][L];
    uint32_t acc[L], b[L];
    for (int w = 0; w < kWTab; w++)
        for (int j = 0; j < L; j++) tab[w][j] = 0;
    constexpr int kPer = kWBits + 1, kMain = kWTab + kPer * kWDigitsW;
#pragma unroll 1
    for (int st = 0; st <= kMain; st++) {
        if (st == 0) {
            for (int j = 0; j < L; j++) acc[j] = r2[j], b[j] = j == 0;
        } else if (st == 1) {
            for (int j = 0; j < L; j++) acc[j] = x[j], b[j] = r2[j];
        } else if (st < kWTab) {
            for (int j = 0; j < L; j++) b[j] = tab[1][j];
        } else if (st < kMain) {
            const int r = st - kWTab;
            if (r % kPer < kWBits) {
                for (int j = 0; j < L; j++) b[j] = acc[j];
            } else {
                uint32_t idx = w_digit_n(e, kLimbsW, kWDigitsW - 1 - r / kPer);
                JFSX_RSA_OPAQUE(idx);
                for (int j = 0; j < L; j++) b[j] = 0;
                for (uint32_t w = 0; w < (uint32_t)kWTab; w++) {
                    uint32_t msk = ~ct_nz(w ^ idx);
                    JFSX_RSA_OPAQUE(msk);
                    JFSX_RSA_TRACE('S', w);
                    for (int j = 0; j < L; j++) b[j] |= tab[w][j] & msk;
                }
            }
        } else {
            for (int j = 0; j < L; j++) b[j] = j == 0;
        }
        mont_mul28_wide(acc, b, m, minv, acc);
        if (st < kWTab) {
            for (int j = 0; j < L; j++) tab[st][j] = acc[j];
            if (st == kWTab - 1)
                for (int j = 0; j < L; j++) acc[j] = tab[0][j];
        }
    }
    from28_wide(acc, L, out32, kLimbsW);
}

// ---------------------------------------------------------------------------
// The private half on a QUAD of lanes (the GPU kernel's form): everything is
// this lane's kQC = 19 limbs of a 74-limb value, as in mont_mul28_quad.
//
// The input reduction c mod m for the 4096-bit c = hi 2^2048 + lo and the
// 2048-bit m runs through the quad product, not through a 64-limb one-lane
// CIOS: t = hi rx R'^-1 = hi 2^2048 mod m with rx = 2^2048 R' mod m from the
// key (hi < 2^2048 < R', rx < m: the product's bound holds), then t + lo < 3 m
// (lo < 2^2048 < 2 m), carried across the lanes, and two masked subtractions
// of m, always both: reduce_2048's steps.
// ---------------------------------------------------------------------------
template <class X>
JFSX_HD void reduce_quad(const X &x, const uint32_t *hi, const uint32_t *lo, const uint32_t *m, uint32_t minv,
                         const uint32_t *rx, uint32_t *out) {
    uint32_t t[kQC];
    mont_mul28_quad(x, hi, rx, m, minv, t);
    uint64_t s[kQC];
#pragma unroll
    for (int j = 0; j < kQC; j++) s[j] = (uint64_t)t[j] + lo[j];
    quad_normalize<kQC>(x, s, t);  // < 3 m < 2^2050: inside the 74 limbs
    quad_sub_if_geq<kQC>(x, t, m, t);
    quad_sub_if_geq<kQC>(x, t, m, out);
}

// out = xv^e mod m on the quad (xv < m; e a 2048-bit exponent in 64 32-bit
// limbs, the same pointer in all lanes; r2 = R'^2 mod m), constant time in e:
// mod_exp28_pair's schedule -- one multiply site in a loop over a step
// counter, table writes at static indices, every digit multiplies, the entry
// picked by a masked scan of all 8 behind a register barrier -- with the
// 8 x 19 table in this lane's registers.
template <class X>
JFSX_HD void mod_exp28_priv_quad(const X &x, const uint32_t *xv, const uint32_t *e, const uint32_t *m, uint32_t minv,
                                 const uint32_t *r2, uint32_t *out) {
    const uint32_t one0 = x.lane == 0u;  // the Montgomery 1's low limb sits in lane 0
    uint32_t tab[kWTab][kQC];
    uint32_t acc[kQC], b[kQC];
    for (int w = 0; w < kWTab; w++)
        for (int j = 0; j < kQC; j++) tab[w][j] = 0;
    constexpr int kPer = kWBits + 1, kMain = kWTab + kPer * kWDigitsW;
#pragma unroll 1
    for (int st = 0; st <= kMain; st++) {
        if (st == 0) {  // R' mod m = r2 * 1
#pragma unroll
            for (int j = 0; j < kQC; j++) acc[j] = r2[j], b[j] = j == 0 ? one0 : 0u;
        } else if (st == 1) {  // x R' mod m
#pragma unroll
            for (int j = 0; j < kQC; j++) acc[j] = xv[j], b[j] = r2[j];
        } else if (st < kWTab) {  // tab[st] = tab[st - 1] * x R'
#pragma unroll
            for (int j = 0; j < kQC; j++) b[j] = tab[1][j];
        } else if (st < kMain) {
            const int r = st - kWTab;
            if (r % kPer < kWBits) {
#pragma unroll
                for (int j = 0; j < kQC; j++) b[j] = acc[j];
            } else {
                uint32_t idx = w_digit_n(e, kLimbsW, kWDigitsW - 1 - r / kPer);
                JFSX_RSA_OPAQUE(idx);
#pragma unroll
                for (int j = 0; j < kQC; j++) b[j] = 0;
#pragma unroll
                for (uint32_t w = 0; w < (uint32_t)kWTab; w++) {
                    uint32_t msk = ~ct_nz(w ^ idx);
                    JFSX_RSA_OPAQUE(msk);
                    if (x.tracing()) JFSX_RSA_TRACE('S', w);
#pragma unroll
                    for (int j = 0; j < kQC; j++) b[j] |= tab[w][j] & msk;
                }
            }
        } else {  // out of the Montgomery domain
#pragma unroll
            for (int j = 0; j < kQC; j++) b[j] = j == 0 ? one0 : 0u;
        }
        mont_mul28_quad(x, acc, b, m, minv, acc);
        if (st < kWTab) {
#pragma unroll
            for (int w = 0; w < kWTab; w++)
#pragma unroll
                for (int j = 0; j < kQC; j++) tab[w][j] = st == w ? acc[j] : tab[w][j];
            if (st == kWTab - 1) {
#pragma unroll
                for (int j = 0; j < kQC; j++) acc[j] = tab[0][j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kQC; j++) out[j] = acc[j];
}

// One whole 4096-bit unwrap on one thread (the CPU pin): ct = 512 bytes,
// big-endian.  Returns the message length (msg in em[0..len)) or -1.
JFSX_HD int decrypt_w(const KeyW &k, const uint8_t *ct, uint8_t em[kModBytesW]) {
    uint32_t c[kNLimbsW], m1[kLimbsW], m2[kLimbsW], m[kNLimbsW], x[kLimbsW];
    from_be(ct, kModBytesW, c, kNLimbsW);
    if (geq(c, k.n, kNLimbsW)) return -1;
    reduce_2048<kLimbsW>(c, k.p, k.pinv, k.r2p, x);
    mod_exp28_priv_wide(x, k.dp, k.p, k.pinv, k.r2p28, m1);
    reduce_2048<kLimbsW>(c, k.q, k.qinv32, k.r2q, x);
    mod_exp28_priv_wide(x, k.dq, k.q, k.qinv32, k.r2q28, m2);
    crt<kLimbsW>(k, m1, m2, m);
    to_be(m, kNLimbsW, em, kModBytesW);
    return oaep_decode(em, kModBytesW, k.lhash);
}

// One whole 4096-bit wrap on one thread (the CPU pin): encrypt() at k = 512
JFSX_HD int encrypt_w(const KeyW &k, uint32_t e, const uint8_t *msg, int len, const uint8_t *seed,
                      uint8_t ct[kModBytesW]) {
    if (len < 0 || len > kMaxMsgW) {
        for (int i = 0; i < kModBytesW; i++) ct[i] = 0;
        return -1;
    }
    uint8_t em[kModBytesW];
    oaep_encode(k.lhash, msg, len, seed, em, kModBytesW);
    uint32_t x[kNLimbsW], r[kNLimbsW];
    from_be(em, kModBytesW, x, kNLimbsW);
    mod_exp28_pub<kN28W>(x, e, k.n, k.ninv28, k.r2n28, r);
    to_be(r, kNLimbsW, ct, kModBytesW);
    return 0;
}

}  // namespace jfsx_rsa
