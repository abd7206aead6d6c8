// CPU build of juicefs_amd/csrc/jfsx_poly.h (test infrastructure only): the
// Poly1305 limb arithmetic of the ChaCha20-Poly1305 kernels, exported one
// function at a time, and two emulations built from those same functions that
// follow jfsx_chacha.hip step by step -- one task's stream (cp_task) and the
// block's finalize (cp_finalize_k).  tests/test_poly1305.py compares all of it
// with Python integers mod 2^130 - 5.
#include <stdint.h>
#include <string.h>

#include "../../juicefs_amd/csrc/jfsx_poly.h"

using namespace jfsx;

namespace {
constexpr uint64_t kSeg = 32768;  // jfsx_internal.h
constexpr int kCpWaves = 4;

void put(uint32_t *o, const P5 &a) {
    for (int i = 0; i < 5; i++) o[i] = a.l[i];
}

// load_piece (jfsx_dev.h): 16 bytes at o, zero past end
void piece(const uint8_t *src, uint64_t o, uint64_t end, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint64_t i = o; i < end && i < o + 16; i++) w[(i - o) >> 2] |= (uint32_t)src[i] << (8 * ((i - o) & 3));
}

// p_wave_sum (jfsx_chacha.hip): the xor butterfly over 64 lanes, every lane
// computing as the wave does; lane 0 holds what the kernel stores
P5 wave_sum(P5 a[64]) {
    for (int off = 32; off > 0; off >>= 1) {
        P5 b[64];
        for (int l = 0; l < 64; l++) b[l] = a[l ^ off];
        for (int l = 0; l < 64; l++) a[l] = p_freeze(p_add(a[l], b[l]));
    }
    return a[0];
}
}  // namespace

extern "C" {
void ph_mul(const uint32_t *a, const uint32_t *b, uint32_t *out) { put(out, p_mul(p_load(a), p_load(b))); }

// the main loop's step, sb = 5 * b as cp_task precomputes it
void ph_mul_add(const uint32_t *a, const uint32_t *b, const uint32_t *m, uint32_t *out) {
    const P5 B = p_load(b);
    uint32_t sb[5];
    for (int i = 0; i < 5; i++) sb[i] = 5u * B.l[i];
    put(out, p_mul_add(p_load(a), B, sb, p_load(m)));
}

void ph_add(const uint32_t *a, const uint32_t *b, uint32_t *out) { put(out, p_add(p_load(a), p_load(b))); }
void ph_freeze(const uint32_t *a, uint32_t *out) { put(out, p_freeze(p_load(a))); }
void ph_from_words(const uint32_t *w, uint32_t hibit, uint32_t *out) {
    put(out, p_from_words(w[0], w[1], w[2], w[3], hibit));
}
void ph_pow(const uint32_t *r2k, uint64_t e, uint32_t *out) {
    put(out, p_pow(reinterpret_cast<const uint32_t(*)[5]>(r2k), e));
}
void ph_tag(const uint32_t *acc, const uint32_t *s, uint32_t *out) { p_tag(p_load(acc), s, out); }

// The bounds p_mul_add's comment states, recomputed here in 128-bit sums that
// cannot wrap: bit 0 a product sum d_i does not fit 64 bits, bit 1 a carry
// d_i >> 26 is not below 2^32, bit 2 carry + message limb wraps 32 bits,
// bit 3 5 * (d4 >> 26) or t = l[0] + 5 * (d4 >> 26) is not below 2^32, bit 4
// an output limb is not below 2^26 (l[1]: 2^26 + 2^6).  0: all hold.
int ph_mul_add_bounds(const uint32_t *a, const uint32_t *b, const uint32_t *m) {
    typedef unsigned __int128 u128;
    int bad = 0;
    u128 sb[5];
    for (int i = 0; i < 5; i++) {
        sb[i] = (u128)5 * b[i];
        if (i && sb[i] >> 32) bad |= 8;  // cp_task's 5u * r.l[i]
    }
    u128 c = 0;
    uint32_t lim[5];
    for (int i = 0; i < 5; i++) {
        const u128 add = c + m[i];
        if (add >> 32) bad |= 4;
        u128 d = add;
        for (int j = 0; j < 5; j++) d += (u128)a[j] * (j <= i ? (u128)b[i - j] : sb[5 + i - j]);
        if (d >> 64) bad |= 1;
        lim[i] = (uint32_t)d & M26;
        c = d >> 26;
        if (c >> 32) bad |= 2;
    }
    const u128 t = (u128)lim[0] + c * 5;
    if ((c * 5) >> 32 || t >> 32) bad |= 8;
    const uint32_t out1 = lim[1] + (uint32_t)(t >> 26);
    if (out1 >= (1u << 26) + (1u << 6)) bad |= 16;
    // and the function itself keeps them
    uint32_t sb32[5];
    for (int i = 0; i < 5; i++) sb32[i] = 5u * b[i];
    const P5 r = p_mul_add(p_load(a), p_load(b), sb32, p_load(m));
    for (int i = 0; i < 5; i++)
        if (r.l[i] >= (1u << 26) + (i == 1 ? 1u << 6 : 0u)) bad |= 16;
    return bad;
}

// cp_keysetup_k's Poly1305 part from keystream block 0's first four words
// (unclamped) and the block's length: r, r^253, init = (length block) * r and
// the table r^(2^k), k < 32.
void ph_keysetup(const uint32_t *blk0, uint64_t len, uint32_t *r_out, uint32_t *r253_out, uint32_t *init_out,
                 uint32_t *r2k_out) {
    const P5 r = p_from_words(blk0[0] & 0x0fffffffu, blk0[1] & 0x0ffffffcu, blk0[2] & 0x0ffffffcu,
                              blk0[3] & 0x0ffffffcu, 0);
    P5 g = r;
    P5 r253 = p_one();
    for (int i = 0; i < 32; i++) {
        put(r2k_out + 5 * i, g);
        if ((253 >> i) & 1) r253 = p_mul(r253, g);
        g = p_mul(g, g);
    }
    const P5 L = p_from_words(0, 0, (uint32_t)len, (uint32_t)(len >> 32), 1);
    put(r_out, r);
    put(r253_out, r253);
    put(init_out, p_freeze(p_mul(L, r)));
}

// cp_task's Poly1305 over the ciphertext c of a block of len bytes, task
// [c0, c1): per wave its whole segments, per lane 64 bytes of every 4 KiB row;
// full rows through p_mul_add (r253 into a row, r within it), the guarded tail
// rows through p_mul + p_add, the lift by r^(wend + 1 - jlast), the wave sum.
// raw: [4][64][5] the lanes' accumulators before the lift; lanes: [4][64][5]
// the lifted canonical values; waves: [4][5] what lane 0 stores as the slot's
// partial; pexp: [4] the slot's exponent.
void ph_stream(const uint8_t *c, uint64_t len, uint64_t c0, uint64_t c1, const uint32_t *r_in,
               const uint32_t *r253_in, const uint32_t *r2k_in, uint32_t *raw, uint32_t *lanes, uint32_t *waves,
               uint32_t *pexp) {
    const uint32_t(*r2k)[5] = reinterpret_cast<const uint32_t(*)[5]>(r2k_in);
    const P5 r1 = p_load(r_in), r253 = p_load(r253_in);
    uint32_t s1[5], s253[5];
    for (int i = 0; i < 5; i++) {
        s1[i] = 5u * r1.l[i];
        s253[i] = 5u * r253.l[i];
    }
    const uint32_t nseg = (uint32_t)((c1 - c0 + kSeg - 1) / kSeg);
    for (uint32_t wave = 0; wave < (uint32_t)kCpWaves; wave++) {
        const uint32_t sa = wave * nseg / kCpWaves, sb = (wave + 1) * nseg / kCpWaves;
        const uint64_t sub0 = c0 + (uint64_t)sa * kSeg;
        const uint64_t sub1 = sb > sa ? (c0 + (uint64_t)sb * kSeg < c1 ? c0 + (uint64_t)sb * kSeg : c1) : sub0;
        const uint64_t rf = (sub1 - sub0) / 4096;  // full rows
        const uint64_t wend = (sub1 + 15) >> 4;
        P5 z[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            P5 A = p_zero();
            uint64_t jlast = 0;
            bool has = false;
            const uint64_t lo = 64 * lane;
            for (uint64_t row = 0; row < rf; row++) {
                const uint64_t o = sub0 + 4096 * row + lo;
                for (int q = 0; q < 4; q++) {
                    uint32_t w[4];
                    piece(c, o + 16 * q, len, w);
                    A = q == 0 ? p_mul_add(A, r253, s253, p_from_words(w[0], w[1], w[2], w[3], 1))
                               : p_mul_add(A, r1, s1, p_from_words(w[0], w[1], w[2], w[3], 1));
                }
            }
            if (rf) {
                has = true;
                jlast = (sub0 + 4096 * (rf - 1) + lo + 48) >> 4;
            }
            // cp_row_generic
            for (uint64_t row = sub0 + 4096 * rf; row < sub1; row += 4096) {
                const uint64_t base = row + 64 * lane;
                for (int q = 0; q < 4; q++) {
                    const uint64_t o = base + 16 * q;
                    if (o >= sub1) break;
                    uint32_t w[4];
                    piece(c, o, sub1, w);
                    A = p_add(p_mul(A, q == 0 ? r253 : r1), p_from_words(w[0], w[1], w[2], w[3], 1));
                    jlast = o >> 4;
                    has = true;
                }
            }
            put(raw + 5 * (64 * wave + lane), A);
            z[lane] = p_zero();
            if (has && sub1 > sub0) z[lane] = p_freeze(p_mul(A, p_pow(r2k, wend + 1 - jlast)));
            put(lanes + 5 * (64 * wave + lane), z[lane]);
        }
        put(waves + 5 * wave, wave_sum(z));
        const uint64_t nblk = (len + 15) >> 4;
        pexp[wave] = (uint32_t)(nblk - wend);
    }
}

// cp_finalize_k's Poly1305: every slot's partial lifted by r^pexp (an all-zero
// partial is not), summed 64 slots at a time with the wave sum, plus init, plus
// s.  lifted: [nslots][5]; acc: the canonical h; tag: 4 words.  Returns the
// number of slots that took the zero-partial skip.
int ph_finalize(const uint32_t *partial, const uint32_t *pexp, uint32_t nslots, const uint32_t *r2k_in,
                const uint32_t *init, const uint32_t *s, uint32_t *lifted, uint32_t *acc_out, uint32_t *tag) {
    const uint32_t(*r2k)[5] = reinterpret_cast<const uint32_t(*)[5]>(r2k_in);
    int skipped = 0;
    P5 acc = p_zero();
    for (uint32_t base = 0; base < nslots; base += 64) {
        P5 zs[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t sl = base + lane;
            P5 z = p_zero();
            if (sl < nslots) {
                z = p_load(partial + 5 * sl);
                if (z.l[0] | z.l[1] | z.l[2] | z.l[3] | z.l[4])
                    z = p_freeze(p_mul(z, p_pow(r2k, pexp[sl])));
                else
                    skipped++;
                put(lifted + 5 * sl, z);
            }
            zs[lane] = z;
        }
        acc = p_freeze(p_add(acc, wave_sum(zs)));
    }
    acc = p_freeze(p_add(acc, p_load(init)));
    put(acc_out, acc);
    p_tag(acc, s, tag);
    return skipped;
}
}
