"""Poly1305 and the ChaCha20-Poly1305 tag over Python integers (RFC 8439), the
reference of tests/test_poly1305.py and tests/test_gpu_poly_edges.py, and the
routine that crafts ciphertexts which drive the kernels' limb arithmetic to a
chosen value.  Nothing here shares code with the kernels' 26-bit limbs
(juicefs_amd/csrc/jfsx_poly.h) or the oracle's 44/44/42-bit ones.

Crafting.  Poly1305 runs over the ciphertext, which the caller of Open chooses
(and the caller of Seal reaches with plaintext = target ^ keystream), and r, s
come from ChaCha20 block 0 of (key, nonce).  A sum of blocks
    sum_{j in J} m_j * r^(E - j)  mod p,    m_j = 2^128 + (16 bytes of C)
is linear in each m_j, so the last 16-byte block of J can be solved for any
target; the solved m_j is a ciphertext block only if it lies in [2^128, 2^129)
(one chance in four), so J's other bytes are reseeded until it does.

Which J: the kernels' layout (jfsx_chacha.hip, cp_task), restated by layout():
  * the planner (engine.debug_plan) cuts a block into tasks [c0, c1);
  * wave w of a task takes its segments [w * nseg / 4, (w + 1) * nseg / 4) of
    32 KiB, nseg = ceil((c1 - c0) / 32 KiB), integer division: a one-segment
    task is wave 3's, waves 0..2 stay empty;
  * a wave walks its bytes in rows of 4 KiB; lane l of a row holds bytes
    64 l .. 64 l + 63, four 16-byte blocks;
  * a lane's sum and the wave's sum are lifted to r^(wend + 1 - j) for block j,
    wend = ceil(wave end / 16); finalize lifts a wave's partial by
    r^(nblk - wend) more and adds (length block) * r.
The layout only chooses inputs: every expected value comes from tag() below."""
import random

P = (1 << 130) - 5
SEG = 32 << 10
M128 = (1 << 128) - 1
R_MAX = 0x0ffffffc0ffffffc0ffffffc0fffffff  # the largest clamped r


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xffffffff


def chacha20_block(key, counter, nonce):
    """RFC 8439 2.3: 64 bytes of keystream."""
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574]
    init += [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)]
    init += [counter & 0xffffffff]
    init += [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
    x = list(init)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return b"".join(((a + b) & 0xffffffff).to_bytes(4, "little") for a, b in zip(x, init))


def poly_key(key, nonce):
    """The one-time Poly1305 key of an AEAD call (RFC 8439 2.6): 32 bytes."""
    return chacha20_block(key, 0, nonce)[:32]


def rs(otk):
    """(clamped r, s) of a 32-byte one-time key."""
    return int.from_bytes(otk[:16], "little") & R_MAX, int.from_bytes(otk[16:32], "little")


def poly1305_h(otk, msg):
    """The accumulator before s is added, in [0, p) (RFC 8439 2.5.1)."""
    r, _ = rs(otk)
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P
    return h


def poly1305(otk, msg):
    return ((poly1305_h(otk, msg) + rs(otk)[1]) & M128).to_bytes(16, "little")


def mac_data(c, aad=b""):
    """RFC 8439 2.8: aad | pad16 | C | pad16 | le64(len aad) | le64(len C)."""
    pad = lambda b: bytes(-len(b) % 16)
    return aad + pad(aad) + c + pad(c) + len(aad).to_bytes(8, "little") + len(c).to_bytes(8, "little")


def tag_h(key, nonce, c):
    """The AEAD's Poly1305 accumulator over ciphertext c (empty AAD)."""
    return poly1305_h(poly_key(key, nonce), mac_data(bytes(c)))


def tag(key, nonce, c, aad=b""):
    """The ChaCha20-Poly1305 tag of ciphertext c."""
    return poly1305(poly_key(key, nonce), mac_data(bytes(c), aad))


# ---------------------------------------------------------------------------
# the kernels' layout


def wave_range(c0, c1, w):
    """Bytes [sub0, sub1) of task [c0, c1) that wave w of the workgroup takes."""
    nseg = -(-(c1 - c0) // SEG)
    sa, sb = w * nseg // 4, (w + 1) * nseg // 4
    sub0 = c0 + sa * SEG
    return (sub0, min(c0 + sb * SEG, c1)) if sb > sa else (sub0, sub0)


def lane_blocks(sub0, sub1, lane):
    """16-byte block indices of lane `lane` of a wave over [sub0, sub1)."""
    return [(row + 64 * lane) // 16 + q for row in range(sub0, sub1, 4096) for q in range(4)
            if row + 64 * lane + 16 * q < sub1]


def wave_blocks(sub0, sub1):
    return list(range(sub0 // 16, -(-sub1 // 16)))


def block_value(c, j):
    """m_j of the AEAD's Poly1305 over c: 16 bytes, zero padded, plus 2^128."""
    return int.from_bytes(bytes(c[16 * j:16 * j + 16]), "little") | (1 << 128)


def lifted_sum(r, c, J, E):
    """sum of m_j * r^(E - j) over the ascending block list J, mod p (Horner over the gaps)."""
    acc, prev, pw = 0, None, {}
    for j in J:
        if prev is not None:
            g = j - prev
            if g not in pw:
                pw[g] = pow(r, g, P)
            acc = acc * pw[g] % P
        acc = (acc + block_value(c, j)) % P
        prev = j
    return acc * pow(r, E - prev, P) % P if J else 0


MAX_RESEEDS = 64


def solve(c, r, J, E, target, seed):
    """Rewrite the bytes of blocks J of bytearray c (seeded) so that
    lifted_sum(r, c, J, E) == target mod p: the last block of J that lies
    wholly inside c is solved for, the others are reseeded, at most
    MAX_RESEEDS times, until the solved block is a 16-byte string plus 2^128.
    Returns the number of reseeds; raises if the cap is reached."""
    full = [j for j in J if 16 * j + 16 <= len(c)]
    if not full:
        raise ValueError("no whole block to solve for")
    js = full[-1]
    inv = pow(pow(r, E - js, P), -1, P)
    for attempt in range(MAX_RESEEDS + 1):
        if attempt:
            rnd = random.Random("%s/%d" % (seed, attempt))
            for j in J:
                n = min(16, len(c) - 16 * j)
                c[16 * j:16 * j + n] = rnd.randbytes(n)
        c[16 * js:16 * js + 16] = bytes(16)
        rest = (lifted_sum(r, c, J, E) - pow(r, E - js, P) * (1 << 128)) % P
        m = (target - rest) * inv % P
        if (1 << 128) <= m < (1 << 129):
            c[16 * js:16 * js + 16] = (m - (1 << 128)).to_bytes(16, "little")
            assert lifted_sum(r, c, J, E) == target % P
            return attempt
    raise RuntimeError("could not craft %r within %d reseeds" % (seed, MAX_RESEEDS))


def seeded(n, seed):
    return bytearray(random.Random("%s/fill" % (seed,)).randbytes(n))


def craft_final(key, nonce, n, target, seed):
    """n bytes of ciphertext whose Poly1305 accumulator (before + s) is target.
    target may be a function of s."""
    r, s = rs(poly_key(key, nonce))
    t = target(s) if callable(target) else target
    c = seeded(n, seed)
    nblk = -(-n // 16)
    length_block = ((n << 64) | (1 << 128)) * r % P
    solve(c, r, list(range(nblk)), nblk + 1, (t - length_block) % P, seed)
    assert tag_h(key, nonce, c) == t % P
    return bytes(c)


def craft_lanes(key, nonce, n, task, wave, lanes, seed):
    """n bytes of ciphertext in which the lifted partials of the given lanes of
    wave `wave` of task (c0, c1) take given values: lanes is a list of
    (lane, target); a target None leaves the lane seeded, a target ("p-", l)
    is p minus lane l's value (so the two add up to exactly p)."""
    r, _ = rs(poly_key(key, nonce))
    c = seeded(n, seed)
    sub0, sub1 = wave_range(task[0], task[1], wave)
    E = -(-sub1 // 16) + 1
    val = {}
    for lane, target in lanes:
        J = lane_blocks(sub0, sub1, lane)
        if isinstance(target, tuple):
            target = P - val[target[1]]
        if target is not None:
            solve(c, r, J, E, target, "%s/lane%d" % (seed, lane))
        val[lane] = lifted_sum(r, c, J, E)
    return bytes(c)


def craft_wave(key, nonce, n, task, wave, target, seed):
    """n bytes of ciphertext in which wave `wave` of task (c0, c1) sums to target."""
    r, _ = rs(poly_key(key, nonce))
    c = seeded(n, seed)
    sub0, sub1 = wave_range(task[0], task[1], wave)
    solve(c, r, wave_blocks(sub0, sub1), -(-sub1 // 16) + 1, target, seed)
    return bytes(c)
