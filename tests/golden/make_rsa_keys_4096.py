"""Write tests/golden/rsa_keys_4096.json: the fixed RSA-4096 keys of the wide
RSA tests (tests/rsa_model_wide.py, test_rsa4096.py, test_gpu_rsa4096.py,
test_gpu_objects_4096.py), as pairs of 2048-bit primes only -- everything else
of a key follows from (p, q) and e = 65537.

The same eight kinds of key as make_rsa_keys.py builds at 1024 bits, for the
same reasons: both orders of p and q (q > p reaches the m2 mod p step of the
CRT recombination), primes next to 2^2048 (limbs all ones) and next to 2^2047
(limbs almost all zero; 2^2048 close to 2m, where the input reduction needs
both corrections most often), ordinary primes, and a pair with long runs of
ones and of zeros that end inside a limb.

Every prime is derived here by search from its definition and proved with
Miller-Rabin, 40 rounds with bases from a SHA-256 counter stream of a fixed
seed; "usable" means also gcd(65537, p - 1) = 1.  Nothing is read from
anywhere.  Run: python tests/golden/make_rsa_keys_4096.py
"""
import hashlib
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
E = 65537
BITS = 2048
ROUNDS = 40
SMALL = [p for p in range(3, 2000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]


def stream_int(nbytes, *tag):
    t = "/".join(str(x) for x in tag).encode()
    out = b""
    ctr = 0
    while len(out) < nbytes:
        out += hashlib.sha256(t + b"#" + ctr.to_bytes(4, "big")).digest()
        ctr += 1
    return int.from_bytes(out[:nbytes], "big")


BASES = [stream_int(BITS // 8 + 8, "rsa_keys_4096.json miller-rabin base", r) for r in range(ROUNDS)]


def is_prime(n, rounds=ROUNDS):
    """Miller-Rabin with `rounds` bases drawn from a fixed-seed stream."""
    if n < 2000:
        return n == 2 or n in SMALL
    if n % 2 == 0 or any(n % p == 0 for p in SMALL):
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for r in range(rounds):
        a = 2 + BASES[r] % (n - 3)
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def usable(n):
    return n.bit_length() == BITS and math.gcd(E, n - 1) == 1 and is_prime(n)


def search(start, step, count=1):
    """The first `count` usable primes at start, start + step, ... (start odd, step +-2)."""
    out = []
    n = start
    while len(out) < count:
        if usable(n):
            out.append(n)
        n += step
    return out


def stream_primes(seed, count):
    """Usable primes from a SHA-256 counter stream: 256 bytes per candidate,
    only the top bit and the low bit forced."""
    out = []
    i = 0
    while len(out) < count:
        n = stream_int(BITS // 8, seed, i) | (1 << (BITS - 1)) | 1
        i += 1
        if usable(n):
            out.append(n)
    return out


def main():
    top_a, top_b = search((1 << BITS) - 1, -2, 2)            # the two largest
    bot_a, bot_b = search((1 << (BITS - 1)) + 1, 2, 2)       # the two smallest
    pl = stream_primes("rsa_keys_4096.json plain primes", 4)
    hole_hi = search((1 << BITS) - (1 << 200) - 1, -2)[0]
    hole_lo = search((1 << (BITS - 1)) + (1 << 500) + 1, 2)[0]

    def form(n):
        for base, nm in ((1 << BITS, "2^2048"), (1 << (BITS - 1), "2^2047"),
                         ((1 << BITS) - (1 << 200), "2^2048 - 2^200"),
                         ((1 << (BITS - 1)) + (1 << 500), "2^2047 + 2^500")):
            if abs(n - base) < 1 << 32:
                return "%s %s %d" % (nm, "+" if n > base else "-", abs(n - base))
        return "from the SHA-256 stream"

    keys = [
        ("top", top_a, top_b, "the two largest usable primes below 2^2048: limbs all ones, p > q"),
        ("top_swapped", top_b, top_a, "the same primes with p < q"),
        ("bottom", bot_b, bot_a, "the two smallest usable primes above 2^2047: limbs almost all zero, 2^2048 close "
                                 "to 2m, so the input reduction often needs both corrections; p > q"),
        ("wide_q_gt_p", bot_a, top_a, "smallest p, largest q: m2 >= p for about half of all inputs, so the "
                                      "recombination must reduce m2 mod p"),
        ("wide_p_gt_q", top_a, bot_a, "the same primes with p > q"),
        ("plain_q_gt_p", min(pl[0], pl[1]), max(pl[0], pl[1]), "ordinary primes, only the top bit forced; p < q as "
                                                               "Go's rsa.GenerateKey may give"),
        ("plain_p_gt_q", max(pl[2], pl[3]), min(pl[2], pl[3]), "ordinary primes, only the top bit forced; p > q"),
        ("holes", hole_hi, hole_lo, "a long run of ones ending at bit 200 (inside a 28-bit limb) and a long run of "
                                    "zeros ending at bit 500 (inside a 32-bit limb)"),
    ]
    rows = []
    for name, p, q, why in keys:
        assert p != q and usable(p) and usable(q), name
        why += " (p = %s, q = %s)" % (form(p), form(q))
        rows.append({"name": name, "why": why, "p": "%x" % p, "q": "%x" % q})
        print("%-14s p = %s, q = %s" % (name, form(p), form(q)))
    with open(os.path.join(HERE, "rsa_keys_4096.json"), "w") as f:
        json.dump({"keys": rows}, f, indent=1)
        f.write("\n")
    print("wrote %d keys" % len(rows))


if __name__ == "__main__":
    main()
