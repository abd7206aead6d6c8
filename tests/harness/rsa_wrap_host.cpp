// CPU build of the key wrap in juicefs_amd/csrc/jfsx_rsa.h (test
// infrastructure only): EME-OAEP encoding, the Montgomery product modulo a
// 2048-bit number in 28-bit limbs, the public exponentiation in its one-lane
// and its lane-quad form, and encrypt().  tests/test_rsa_wrap.py loads it as a
// shared object and checks it against Python integers and tests/rsa_model.py;
// with RSA_WRAP_MAIN it is a stand-alone program for the sanitizers (make -f
// rsa_wrap_sanitize.mk run).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <thread>
// the sequence of Montgomery products, hashed
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

// f(QuadThreads, lane) on four threads in lock step
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

extern "C" {
// EM (256 bytes) of msg under the label and the seed (32 bytes); len <= 190
void wrap_oaep_encode(const uint8_t *label, int label_len, const uint8_t *msg, int len, const uint8_t *seed,
                      uint8_t *em) {
    uint8_t lh[32];
    sha256_2(label, label_len, label, 0, lh);
    oaep_encode(lh, msg, len, seed, em);
}

// out = a b R''^-1 mod m (256-byte big-endian operands, m odd, a, b < m) by
// the one-lane product (quad = 0) or the lane-quad one; returns 1 unless the
// quad's lanes disagree on which limbs are whose
int wrap_mont_mul(const uint8_t *m_be, const uint8_t *a_be, const uint8_t *b_be, uint8_t *out_be, int quad) {
    uint32_t m32[kNLimbs], a32[kNLimbs], b32[kNLimbs], r32[kNLimbs];
    from_be(m_be, kModBytes, m32, kNLimbs);
    from_be(a_be, kModBytes, a32, kNLimbs);
    from_be(b_be, kModBytes, b32, kNLimbs);
    const uint32_t minv = mont_inv32(m32[0]) & kM28;
    uint32_t f[4 * kQC];
    for (int j = 0; j < 4 * kQC; j++) f[j] = 0;
    if (!quad) {
        uint32_t m[kN28], a[kN28], b[kN28];
        for (int j = 0; j < kN28; j++)
            m[j] = limb28(m32, kNLimbs, j), a[j] = limb28(a32, kNLimbs, j), b[j] = limb28(b32, kNLimbs, j);
        mont_mul28_wide(a, b, m, minv, f);
    } else {
        run_quad([&](QuadThreads x) {
            uint32_t m[kQC], a[kQC], b[kQC];
            for (int j = 0; j < kQC; j++) {
                const int col = kQC * (int)x.lane + j;
                m[j] = limb28(m32, kNLimbs, col), a[j] = limb28(a32, kNLimbs, col), b[j] = limb28(b32, kNLimbs, col);
            }
            mont_mul28_quad(x, a, b, m, minv, f + kQC * x.lane);
        });
    }
    int ok = f[kN28] == 0 && f[kN28 + 1] == 0;
    for (int j = 0; j < kN28; j++) ok &= f[j] <= kM28;  // normalized limbs
    from28_wide(f, kN28, r32, kNLimbs);
    to_be(r32, kNLimbs, out_be, kModBytes);
    return ok;
}

// x^e mod m (256-byte big-endian, m odd, x < m) by mod_exp28_pub (quad = 0)
// or mod_exp28_pub_quad; returns the operation-trace hash, *ops the count,
// *same = 1 when all four lanes returned the same result
uint64_t wrap_exp_trace(const uint8_t *m_be, uint32_t e, const uint8_t *x_be, uint8_t *out_be, uint64_t *ops,
                        int *same, int quad) {
    uint32_t m[kNLimbs], x[kNLimbs], r2[kNLimbs], r[4][kNLimbs];
    from_be(m_be, kModBytes, m, kNLimbs);
    from_be(x_be, kModBytes, x, kNLimbs);
    mont_r2_wide(m, kNLimbs, r2, 2 * 28 * kN28);
    const uint32_t minv = mont_inv32(m[0]) & kM28;
    start_trace();
    *same = 1;
    if (!quad) {
        mod_exp28_pub(x, e, m, minv, r2, r[0]);
    } else {
        run_quad([&](QuadThreads q) { mod_exp28_pub_quad(q, x, e, m, minv, r2, r[q.lane]); });
        for (int l = 1; l < 4; l++) *same &= memcmp(r[0], r[l], sizeof(r[0])) == 0;
    }
    to_be(r[0], kNLimbs, out_be, kModBytes);
    *ops = g_ops;
    return g_trace;
}

// encrypt(): 0 or -1 (message too long), -2 on a bad key; ct 256 bytes
int wrap_encrypt(const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq, const uint8_t *qinv,
                 const uint8_t *label, int label_len, uint32_t e, const uint8_t *msg, int len, const uint8_t *seed,
                 uint8_t *ct) {
    static Key k;
    if (!key_setup(k, p, q, dp, dq, qinv, label, label_len)) return -2;
    return encrypt(k, e, msg, len, seed, ct);
}
}

#ifdef RSA_WRAP_MAIN
// the stand-alone sanitizer run: every entry point above on edge operands,
// the one-lane and the quad form against each other
int main() {
    uint8_t m[kModBytes], x[kModBytes], y[kModBytes], r0[kModBytes], r1[kModBytes];
    int bad = 0;
    for (int mod = 0; mod < 3; mod++) {
        // 2^2048 - 1, 2^2047 + 1, and a byte pattern
        for (int i = 0; i < kModBytes; i++) m[i] = mod == 0 ? 0xFF : mod == 1 ? 0 : (uint8_t)(0x9E + 37 * i);
        if (mod == 1) m[0] = 0x80;
        m[kModBytes - 1] |= 1;
        if (mod == 2) m[0] |= 0x80;
        for (int op = 0; op < 3; op++) {
            // 0, m - 1, a pattern below m
            for (int i = 0; i < kModBytes; i++) x[i] = op == 0 ? 0 : op == 1 ? m[i] : (uint8_t)(0x3B + 101 * i);
            if (op == 1) x[kModBytes - 1] &= 0xFE;
            if (op == 2) x[0] &= 0x3F;
            memcpy(y, x, sizeof(y));
            bad |= !wrap_mont_mul(m, x, y, r0, 0) || !wrap_mont_mul(m, x, y, r1, 1) || memcmp(r0, r1, kModBytes);
            const uint32_t es[] = {2, 3, 65537, 0x5A5A5A5Bu, 0x7FFFFFFFu};
            for (uint32_t e : es) {
                uint64_t o0, o1;
                int s0, s1;
                const uint64_t h0 = wrap_exp_trace(m, e, x, r0, &o0, &s0, 0);
                (void)h0;
                wrap_exp_trace(m, e, x, r1, &o1, &s1, 1);
                bad |= !s1 || o0 != o1 || memcmp(r0, r1, kModBytes);
            }
        }
    }
    // a whole wrap on the primes 2^1024 - 105 and 2^1024 - 179, every length edge
    uint8_t p[128], q[128], one[128], msg[192], seed[32], ct[kModBytes], em[kModBytes];
    memset(p, 0xFF, 128);
    memset(q, 0xFF, 128);
    p[127] = (uint8_t)(0x100 - 105);
    q[127] = (uint8_t)(0x100 - 179);
    memset(one, 0, 128);
    one[127] = 3;
    for (int i = 0; i < 192; i++) msg[i] = (uint8_t)(i * 7 + 1);
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(255 - i);
    const int lens[] = {0, 1, 31, 32, 33, 190, 191};
    for (int len : lens) {
        const int rc = wrap_encrypt(p, q, one, one, one, (const uint8_t *)"keys", 4, 65537, msg, len, seed, ct);
        bad |= rc != (len > kMaxMsg ? -1 : 0);
        if (len <= kMaxMsg) wrap_oaep_encode((const uint8_t *)"", 0, msg, len, seed, em);
    }
    printf(bad ? "rsa_wrap_host: MISMATCH\n" : "rsa_wrap_host: ok\n");
    return bad;
}
#endif
