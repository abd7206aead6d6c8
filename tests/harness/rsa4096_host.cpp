// CPU build of the RSA-4096 arithmetic in juicefs_amd/csrc/jfsx_rsa.h (test
// infrastructure only): the Montgomery product modulo a 4096-bit number in 148
// limbs of 28 bits (one lane and lane quad), the input reduction of a 4096-bit
// ciphertext modulo a 2048-bit prime, the constant-time private exponentiation
// in its one-lane and its lane-quad form, and decrypt_w() / encrypt_w().
// tests/test_rsa4096.py loads it as a shared object and checks it against
// Python integers and tests/rsa_model_wide.py; with RSA4096_MAIN it is a
// stand-alone program for the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
// the sequence of Montgomery products and window-table reads, hashed
static uint64_t g_trace = 1469598103934665603ull, g_ops = 0;
#define JFSX_RSA_TRACE(tag, v) \
    (g_trace = (g_trace ^ ((uint64_t)(tag) << 8 ^ (uint64_t)(v))) * 1099511628211ull, g_ops++)
#define JFSX_HD static inline
#include "../../juicefs_amd/csrc/jfsx_rsa.h"

using namespace jfsx_rsa;

// the quad's lane exchange on the CPU: four threads that meet at a barrier for
// every exchanged word (SIMT lock step)
struct QuadShared {
    std::atomic<uint32_t> gen{0};
    std::atomic<int> cnt{0};
    uint32_t slot[4];
};
struct QuadThreads {
    uint32_t lane;
    QuadShared *sh;
    bool tracing() const { return lane == 0; }
    void barrier() const {
        const uint32_t g = sh->gen.load(std::memory_order_acquire);
        if (sh->cnt.fetch_add(1, std::memory_order_acq_rel) == 3) {
            sh->cnt.store(0, std::memory_order_relaxed);
            sh->gen.store(g + 1, std::memory_order_release);
        } else {
            for (int k = 0; sh->gen.load(std::memory_order_acquire) == g; k++)
                if (k > 64) std::this_thread::yield();
        }
    }
    uint32_t xchg(uint32_t v, uint32_t src) const {
        sh->slot[lane] = v;
        barrier();
        const uint32_t r = sh->slot[src];
        barrier();
        return r;
    }
    template <int K>
    uint32_t from(uint32_t v) const {
        return xchg(v, K);
    }
    uint32_t next(uint32_t v) const { return xchg(v, (lane + 1) & 3u); }
    uint32_t prev(uint32_t v) const { return xchg(v, (lane + 3) & 3u); }
};

template <class F>
static void run_quad(F f) {
    QuadShared sh;
    std::thread t1([&] { f(QuadThreads{1, &sh}); }), t2([&] { f(QuadThreads{2, &sh}); }),
        t3([&] { f(QuadThreads{3, &sh}); });
    f(QuadThreads{0, &sh});
    t1.join();
    t2.join();
    t3.join();
}

static void start_trace() {
    g_trace = 1469598103934665603ull;
    g_ops = 0;
}

// this lane's QC limbs of a value in nl32 32-bit limbs
template <int QC>
static void lane_limbs(const uint32_t *v, int nl32, uint32_t lane, uint32_t *y) {
    for (int j = 0; j < QC; j++) y[j] = limb28(v, nl32, QC * (int)lane + j);
}

extern "C" {
// EM (512 bytes) of msg under the label and the seed (32 bytes); len <= 446
void w_oaep_encode(const uint8_t *label, int label_len, const uint8_t *msg, int len, const uint8_t *seed,
                   uint8_t *em) {
    uint8_t lh[32];
    sha256_2(label, label_len, label, 0, lh);
    oaep_encode(lh, msg, len, seed, em, kModBytesW);
}

// out = a b R''^-1 mod m (512-byte big-endian operands, m odd with bit 4095
// set, a, b < m; R'' = 2^(28 * 148)) by the one-lane product (quad = 0) or the
// lane-quad one; returns 1 when the limbs came out normalized
int w_mont_mul(const uint8_t *m_be, const uint8_t *a_be, const uint8_t *b_be, uint8_t *out_be, int quad) {
    static uint32_t m32[kNLimbsW], a32[kNLimbsW], b32[kNLimbsW], r32[kNLimbsW];
    from_be(m_be, kModBytesW, m32, kNLimbsW);
    from_be(a_be, kModBytesW, a32, kNLimbsW);
    from_be(b_be, kModBytesW, b32, kNLimbsW);
    const uint32_t minv = mont_inv32(m32[0]) & kM28;
    uint32_t f[4 * kQCW];
    for (int j = 0; j < 4 * kQCW; j++) f[j] = 0;
    if (!quad) {
        uint32_t m[kN28W], a[kN28W], b[kN28W];
        for (int j = 0; j < kN28W; j++)
            m[j] = limb28(m32, kNLimbsW, j), a[j] = limb28(a32, kNLimbsW, j), b[j] = limb28(b32, kNLimbsW, j);
        mont_mul28_wide<kN28W>(a, b, m, minv, f);
    } else {
        run_quad([&](QuadThreads x) {
            uint32_t m[kQCW], a[kQCW], b[kQCW];
            lane_limbs<kQCW>(m32, kNLimbsW, x.lane, m);
            lane_limbs<kQCW>(a32, kNLimbsW, x.lane, a);
            lane_limbs<kQCW>(b32, kNLimbsW, x.lane, b);
            mont_mul28_quad<QuadThreads, kN28W>(x, a, b, m, minv, f + kQCW * x.lane);
        });
    }
    int ok = f[kN28W - 1] == 0;  // the 148th limb
    for (int j = 0; j < kN28W; j++) ok &= f[j] <= kM28;
    from28_wide(f, kN28W, r32, kNLimbsW);
    to_be(r32, kNLimbsW, out_be, kModBytesW);
    return ok;
}

// out = c mod m for a 512-byte c and a 256-byte odd m with bit 2047 set, by
// reduce_2048<64> (quad = 0) or reduce_quad; returns 1 when the quad's limbs
// came out normalized
int w_reduce(const uint8_t *m_be, const uint8_t *c_be, uint8_t *out_be, int quad) {
    uint32_t m32[kLimbsW], c32[kNLimbsW], r32[kLimbsW], k32[kLimbsW];
    from_be(m_be, 4 * kLimbsW, m32, kLimbsW);
    from_be(c_be, kModBytesW, c32, kNLimbsW);
    const uint32_t minv = mont_inv32(m32[0]);
    int ok = 1;
    if (!quad) {
        mont_r2_wide(m32, kLimbsW, k32, 2 * 32 * kLimbsW);
        reduce_2048<kLimbsW>(c32, m32, minv, k32, r32);
    } else {
        mont_r2_wide(m32, kLimbsW, k32, kHalfBits + 28 * kN28);
        uint32_t f[4 * kQC];
        run_quad([&](QuadThreads x) {
            uint32_t m[kQC], hi[kQC], lo[kQC], rx[kQC];
            lane_limbs<kQC>(m32, kLimbsW, x.lane, m);
            lane_limbs<kQC>(c32 + kLimbsW, kLimbsW, x.lane, hi);
            lane_limbs<kQC>(c32, kLimbsW, x.lane, lo);
            lane_limbs<kQC>(k32, kLimbsW, x.lane, rx);
            reduce_quad(x, hi, lo, m, minv & kM28, rx, f + kQC * x.lane);
        });
        ok = f[kN28] == 0 && f[kN28 + 1] == 0;
        for (int j = 0; j < kN28; j++) ok &= f[j] <= kM28;
        from28_wide(f, kN28, r32, kLimbsW);
    }
    to_be(r32, kLimbsW, out_be, 4 * kLimbsW);
    return ok;
}

// x^e mod m (256-byte big-endian, m odd with bit 2047 set, x < m, e any 2048-bit
// value) by mod_exp28_priv_wide (quad = 0) or mod_exp28_priv_quad; returns the
// operation-trace hash, *ops the count, *same = 1 when the quad's limbs came
// out normalized
uint64_t w_priv_exp_trace(const uint8_t *m_be, const uint8_t *e_be, const uint8_t *x_be, uint8_t *out_be,
                          uint64_t *ops, int *same, int quad) {
    uint32_t m32[kLimbsW], e32[kLimbsW], x32[kLimbsW], r2[kLimbsW], r32[kLimbsW];
    from_be(m_be, 4 * kLimbsW, m32, kLimbsW);
    from_be(e_be, 4 * kLimbsW, e32, kLimbsW);
    from_be(x_be, 4 * kLimbsW, x32, kLimbsW);
    mont_r2_wide(m32, kLimbsW, r2, 2 * 28 * kN28);
    const uint32_t minv = mont_inv32(m32[0]);
    start_trace();
    *same = 1;
    if (!quad) {
        mod_exp28_priv_wide(x32, e32, m32, minv, r2, r32);
    } else {
        uint32_t f[4 * kQC];
        run_quad([&](QuadThreads x) {
            uint32_t m[kQC], xv[kQC], r[kQC];
            lane_limbs<kQC>(m32, kLimbsW, x.lane, m);
            lane_limbs<kQC>(x32, kLimbsW, x.lane, xv);
            lane_limbs<kQC>(r2, kLimbsW, x.lane, r);
            mod_exp28_priv_quad(x, xv, e32, m, minv & kM28, r, f + kQC * x.lane);
        });
        *same = f[kN28] == 0 && f[kN28 + 1] == 0;
        for (int j = 0; j < kN28; j++) *same &= f[j] <= kM28;
        from28_wide(f, kN28, r32, kLimbsW);
    }
    to_be(r32, kLimbsW, out_be, 4 * kLimbsW);
    *ops = g_ops;
    return g_trace;
}

static KeyW g_key;

// decrypt_w() of a ciphertext of ct_len bytes as rsa.DecryptOAEP takes it:
// longer than 512 bytes is the decryption error, shorter is a big-endian
// integer.  Returns the message length (msg: up to 446 bytes) or -1; -2 on a
// bad key.
int w_decrypt(const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq, const uint8_t *qinv,
              const uint8_t *label, int label_len, const uint8_t *ct, int ct_len, uint8_t *msg) {
    if (!key_setup_w(g_key, p, q, dp, dq, qinv, label, label_len)) return -2;
    if (ct_len > kModBytesW || ct_len <= 0) return -1;
    uint8_t c[kModBytesW], em[kModBytesW];
    memset(c, 0, sizeof(c));
    memcpy(c + kModBytesW - ct_len, ct, ct_len);
    const int len = decrypt_w(g_key, c, em);
    if (len > 0) memcpy(msg, em, len);
    return len;
}

// encrypt_w(): 0 or -1 (message too long), -2 on a bad key; ct 512 bytes
int w_encrypt(const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq, const uint8_t *qinv,
              const uint8_t *label, int label_len, uint32_t e, const uint8_t *msg, int len, const uint8_t *seed,
              uint8_t *ct) {
    if (!key_setup_w(g_key, p, q, dp, dq, qinv, label, label_len)) return -2;
    return encrypt_w(g_key, e, msg, len, seed, ct);
}
}

#ifdef RSA4096_MAIN
// the stand-alone sanitizer run: every entry point above on edge operands, the
// one-lane and the quad forms against each other, and a wrap and an unwrap on
// the odd numbers 2^2048 - 1557 and 2^2048 - 1827 in the primes' place, with 3
// for dp, dq and qinv (the arithmetic is exercised, not the key's meaning)
int main() {
    static uint8_t m[kModBytesW], x[kModBytesW], y[kModBytesW], r0[kModBytesW], r1[kModBytesW];
    int bad = 0;
    for (int mod = 0; mod < 3; mod++) {
        for (int i = 0; i < kModBytesW; i++) m[i] = mod == 0 ? 0xFF : mod == 1 ? 0 : (uint8_t)(0x9E + 37 * i);
        m[0] |= 0x80;
        m[kModBytesW - 1] |= 1;
        for (int op = 0; op < 3; op++) {
            for (int i = 0; i < kModBytesW; i++) x[i] = op == 0 ? 0 : op == 1 ? m[i] : (uint8_t)(0x3B + 101 * i);
            if (op == 1) x[kModBytesW - 1] &= 0xFE;
            if (op == 2) x[0] &= 0x3F;
            memcpy(y, x, sizeof(y));
            bad |= !w_mont_mul(m, x, y, r0, 0) || !w_mont_mul(m, x, y, r1, 1) || memcmp(r0, r1, kModBytesW);
            // the 2048-bit modulus m[256..512) with its top bit set
            uint8_t pm[256];
            memcpy(pm, m + 256, 256);
            pm[0] |= 0x80;
            bad |= !w_reduce(pm, x, r0, 0) || !w_reduce(pm, x, r1, 1) || memcmp(r0, r1, 256);
        }
    }
    static uint8_t p[256], q[256], three[256], msg[448], seed[32], ct[kModBytesW], em[kModBytesW], out[kModBytesW];
    memset(p, 0xFF, 256);
    memset(q, 0xFF, 256);
    p[254] = 0xF9, p[255] = 0xEB;  // 2^2048 - 1557
    q[254] = 0xF8, q[255] = 0xDD;  // 2^2048 - 1827
    memset(three, 0, 256);
    three[255] = 3;
    {
        // one private exponentiation, both forms, exponent all ones
        uint8_t e[256], xx[256];
        uint64_t o0, o1;
        int s0, s1;
        memset(e, 0xFF, 256);
        for (int i = 0; i < 256; i++) xx[i] = (uint8_t)(i * 13 + 5);
        xx[0] &= 0x7F;
        w_priv_exp_trace(p, e, xx, r0, &o0, &s0, 0);
        w_priv_exp_trace(p, e, xx, r1, &o1, &s1, 1);
        bad |= !s1 || o0 != o1 || memcmp(r0, r1, 256);
    }
    for (int i = 0; i < 448; i++) msg[i] = (uint8_t)(i * 7 + 1);
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(255 - i);
    const int lens[] = {0, 1, 32, 446, 447};
    for (int len : lens) {
        const int rc = w_encrypt(p, q, three, three, three, (const uint8_t *)"keys", 4, 65537, msg, len, seed, ct);
        bad |= rc != (len > kMaxMsgW ? -1 : 0);
        if (len <= kMaxMsgW) w_oaep_encode((const uint8_t *)"", 0, msg, len, seed, em);
    }
    // the unwrap's whole path on a ciphertext of 511 bytes (the result is a
    // decryption error or not; no byte outside the buffers is touched)
    (void)w_decrypt(p, q, three, three, three, (const uint8_t *)"keys", 4, ct + 1, 511, out);
    bad |= w_decrypt(p, q, three, three, three, (const uint8_t *)"keys", 4, ct, 513, out) != -1;
    printf(bad ? "rsa4096_host: MISMATCH\n" : "rsa4096_host: ok\n");
    return bad;
}
#endif
