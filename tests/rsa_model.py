"""Pure-Python statement of the RSA-OAEP key unwrap as the reference runs it
(rsaEncryptor.Decrypt = rsa.DecryptOAEP(sha256.New(), rand, privKey, wrapped,
[]byte("keys")), pkg/object/encrypt.go:124-134), for the RSA tests.  Python
integers and hashlib's SHA-256: nothing of the engine, no ctypes, no libcrypto.

The private operation is pow(c, d, n), deliberately without the CRT, so the
model shares no structure with jfsx_rsa.h.  The predicates below read
only the model's own integers; the tests use them to prove that their inputs
reach the paths of jfsx_rsa.h they are meant to reach.

fixed_keys() and case_set() build the fixed keys of tests/golden/rsa_keys.json
and, per key, the ciphertext set every RSA test submits (from fixed seeds,
cached: pow(c, d, n) costs milliseconds in Python)."""
import collections
import functools
import hashlib
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rsa_keys.json")

E = 65537
K = 256          # modulus bytes (RSA-2048)
HLEN = 32        # SHA-256
R = 1 << 1024    # the radix of reduce_2048's split c = hi R + lo

Key = collections.namedtuple("Key", "p q n d dp dq qinv")


def key(p, q):
    """The private key of primes p, q for e = 65537 (Go's Primes[0], Primes[1],
    D, Precomputed.Dp, Dq, Qinv)."""
    if math.gcd(E, p - 1) != 1 or math.gcd(E, q - 1) != 1:
        raise ValueError("e = 65537 is not invertible mod p - 1 or q - 1")
    if p == q:
        raise ValueError("p == q")
    d = pow(E, -1, (p - 1) * (q - 1) // math.gcd(p - 1, q - 1))
    return Key(p, q, p * q, d, pow(E, -1, p - 1), pow(E, -1, q - 1), pow(q, -1, p))


def components(k, nbytes=128):
    """(p, q, dp, dq, qinv), big-endian, nbytes each: what Engine.rsa_key takes."""
    return tuple(v.to_bytes(nbytes, "big") for v in (k.p, k.q, k.dp, k.dq, k.qinv))


def mgf1(seed, n):
    out = b""
    c = 0
    while len(out) < n:
        out += hashlib.sha256(bytes(seed) + c.to_bytes(4, "big")).digest()
        c += 1
    return out[:n]


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def oaep_encode(msg, seed, label=b"keys", patch=None, k=K):
    """EME-OAEP encoding (RFC 8017 7.1.1 step 2) with SHA-256 as hash and MGF1
    hash; `patch(db)` edits the data block before masking (to build encodings
    a conforming sender never makes).  Returns the k-byte EM as a bytearray."""
    if len(msg) > k - 2 * HLEN - 2 or len(seed) != HLEN:
        raise ValueError("message too long or bad seed")
    db = bytearray(hashlib.sha256(label).digest() + bytes(k - len(msg) - 2 * HLEN - 2) + b"\x01" + bytes(msg))
    if patch:
        patch(db)
    mdb = _xor(db, mgf1(seed, len(db)))
    mseed = _xor(seed, mgf1(mdb, HLEN))
    return bytearray(b"\0" + mseed + mdb)


def oaep_decode(em, label=b"keys"):
    """RFC 8017 7.1.2 step 3 as Go's decryptOAEP: the message, or None for the
    one decryption error (nonzero first byte, wrong label hash, no 0x01
    separator, or a nonzero byte in the padding before it)."""
    em = bytes(em)
    seed = _xor(em[1:1 + HLEN], mgf1(em[1 + HLEN:], HLEN))
    db = _xor(em[1 + HLEN:], mgf1(seed, len(em) - 1 - HLEN))
    if em[0] != 0 or db[:HLEN] != hashlib.sha256(label).digest():
        return None
    rest = db[HLEN:].lstrip(b"\0")
    if not rest or rest[0] != 1:
        return None
    return rest[1:]


def encrypt_em(k, em):
    """RSAEP of an encoded message, as an integer."""
    return pow(int.from_bytes(bytes(em), "big"), E, k.n)


def decrypt(k, ct, label=b"keys"):
    """rsa.DecryptOAEP: the message, or None for "crypto/rsa: decryption
    error".  A ciphertext longer than the modulus is an error, a shorter one is
    a big-endian integer all the same, c >= n is an error."""
    ct = bytes(ct)
    if len(ct) > K:
        return None
    c = int.from_bytes(ct, "big")
    if c >= k.n:
        return None
    return oaep_decode(pow(c, k.d, k.n).to_bytes(K, "big"), label)


# ---------------------------------------------------------------------------
# which paths of the CRT unwrap an input reaches, from the model's integers
# ---------------------------------------------------------------------------
def m2_ge_p(k, c):
    """c^dq mod q >= p: the recombination has to reduce m2 mod p (q > p only)."""
    return pow(c, k.dq, k.q) >= k.p


def m1_lt_m2(k, c):
    """m1 < (m2 mod p): m1 - m2 borrows and p is added back."""
    return pow(c, k.dp, k.p) < pow(c, k.dq, k.q) % k.p


def reduce_corrections(m, c):
    """How many times m comes off ((c >> 1024) 2^1024 mod m) + (c mod 2^1024),
    the sum the input reduction forms for a 1024-bit m: 0, 1 or 2."""
    t = ((c >> 1024) * R) % m + c % R
    assert t // m <= 2
    return t // m


# ---------------------------------------------------------------------------
# the fixed keys and their ciphertext sets
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixed_keys():
    """name -> Key, in the file's order."""
    with open(GOLDEN) as f:
        rows = json.load(f)["keys"]
    return {r["name"]: key(int(r["p"], 16), int(r["q"], 16)) for r in rows}


def _stream(*tag):
    """A reproducible byte source: SHA-256 in counter mode over a tag."""
    t = "/".join(str(x) for x in tag).encode()
    ctr = 0
    while True:
        yield from hashlib.sha256(t + b"#" + ctr.to_bytes(4, "big")).digest()
        ctr += 1


def det_bytes(n, *tag):
    s = _stream(*tag)
    return bytes(next(s) for _ in range(n))


def ct256(c):
    return c.to_bytes(K, "big")


Case = collections.namedtuple("Case", "name ct expect")

VALID_LENGTHS = (0, 1, 31, 32, 33, 190)
VALID_SEEDS = 7  # 6 lengths x 7 seeds = 42 valid messages per key


@functools.lru_cache(maxsize=None)
def valid_ints(name):
    """[(case name, message, ciphertext integer)] of the valid messages."""
    k = fixed_keys()[name]
    out = []
    for n in VALID_LENGTHS:
        for s in range(VALID_SEEDS):
            msg = det_bytes(n, name, "msg", n, s)
            c = encrypt_em(k, oaep_encode(msg, det_bytes(HLEN, name, "seed", n, s)))
            out.append(("valid len %d seed %d" % (n, s), msg, c))
    return out


@functools.lru_cache(maxsize=None)
def short_ciphertext(name):
    """(message, c) with c < 2^2040, so its big-endian form has a zero first byte."""
    k = fixed_keys()[name]
    for s in range(100000):
        msg = det_bytes(32, name, "short msg", s)
        c = encrypt_em(k, oaep_encode(msg, det_bytes(HLEN, name, "short seed", s)))
        if c < 1 << 2040:
            return msg, c
    raise AssertionError("no short ciphertext for " + name)


def _set(db, i, v):
    db[i] = v


@functools.lru_cache(maxsize=None)
def case_set(name):
    """Every Case of one fixed key under the label "keys"; expect is the
    model's decrypt (bytes or None)."""
    k = fixed_keys()[name]
    items = [(nm, ct256(c)) for nm, _, c in valid_ints(name)]
    # short ciphertexts: Go takes any length up to the modulus as an integer
    _, c = short_ciphertext(name)
    items += [("short as 256 bytes", ct256(c)), ("short as 255 bytes", c.to_bytes(K - 1, "big")),
              ("short as 257 bytes", b"\0" + ct256(c)), ("empty ciphertext", b"")]
    # range edges
    p, q, n = k.p, k.q, k.n
    edges = [("0", 0), ("1", 1), ("2", 2), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("2^2048-1", (1 << 2048) - 1),
             ("p", p), ("q", q), ("p(q-1)", p * (q - 1)), ("q(p-1)", q * (p - 1)), ("p-1", p - 1), ("q+1", q + 1),
             ("2^1024", R), ("2^1024-1", R - 1)]
    items += [("edge c = " + nm, ct256(v)) for nm, v in edges]
    # arithmetically valid, bad OAEP: the failure is found by the masked decode
    msg = det_bytes(32, name, "bad msg")

    def seed(i):
        return det_bytes(HLEN, name, "bad seed", i)
    bad = [("other label", oaep_encode(msg, seed(0), label=b"other"))]
    em = oaep_encode(msg, seed(1))
    em[0] = 1
    if int.from_bytes(em, "big") < n:
        bad.append(("first byte 1", em))
    bad.append(("no separator", oaep_encode(b"", seed(2), patch=lambda db: _set(db, len(db) - 1, 0))))
    bad.append(("0x02 in the padding", oaep_encode(msg, seed(3), patch=lambda db: _set(db, 40, 2))))
    bad.append(("0x07 in the padding", oaep_encode(msg, seed(4), patch=lambda db: _set(db, 40, 7))))
    items += [("bad oaep: " + nm, ct256(encrypt_em(k, em))) for nm, em in bad]
    return tuple(Case(nm, ct, decrypt(k, ct)) for nm, ct in items)


@functools.lru_cache(maxsize=None)
def empty_label_case_set(name):
    """Cases for a key created with an empty label (label_len 0)."""
    k = fixed_keys()[name]
    items = []
    for n in (0, 32, 190):
        em = oaep_encode(det_bytes(n, name, "nolabel msg", n), det_bytes(HLEN, name, "nolabel seed", n), label=b"")
        items.append(("empty label, len %d" % n, ct256(encrypt_em(k, em))))
    items.append(('made for "keys"', ct256(valid_ints(name)[3 * VALID_SEEDS][2])))
    return tuple(Case(nm, ct, decrypt(k, ct, label=b"")) for nm, ct in items)


@functools.lru_cache(maxsize=None)
def path_stats(name):
    """Counts over the valid messages of one key, from the predicates above."""
    k = fixed_keys()[name]
    cs = [c for _, _, c in valid_ints(name)]
    ge = [m2_ge_p(k, c) for c in cs]
    lt = [m1_lt_m2(k, c) for c in cs]
    return {"valid": len(cs), "m2_ge_p": sum(ge), "m1_lt_m2": sum(lt),
            "m2_ge_p_and_m1_lt_m2": sum(a and b for a, b in zip(ge, lt)),
            "corrections_p": tuple(sum(reduce_corrections(k.p, c) == i for c in cs) for i in range(3)),
            "corrections_q": tuple(sum(reduce_corrections(k.q, c) == i for c in cs) for i in range(3))}


def assert_reaches_paths(name):
    """The inputs of case_set(name) reach the paths the key is there for.
    Read from the model alone, before any engine result is looked at; if a
    condition fails, the seeds change, not the condition."""
    s = path_stats(name)
    assert s["valid"] >= 40, (name, s)
    assert 0 < s["m1_lt_m2"] < s["valid"], (name, s)  # m1 - m2 with and without the borrow
    if name == "wide_q_gt_p":
        assert s["m2_ge_p"] >= 8, (name, s)
        # m2 >= p and m1 < m2 - p: the inputs whose result changes if m2 is not reduced mod p
        assert s["m2_ge_p_and_m1_lt_m2"] >= 4, (name, s)
    if name == "plain_q_gt_p":  # an ordinary key's primes are close: few such inputs, but not none
        assert s["m2_ge_p_and_m1_lt_m2"] >= 1, (name, s)
    if name == "bottom":
        assert s["corrections_p"][2] >= 1 and s["corrections_q"][2] >= 1, (name, s)
    exp = {c.name: c.expect for c in case_set(name)}
    msg, _ = short_ciphertext(name)
    assert exp["short as 256 bytes"] == exp["short as 255 bytes"] == msg
    assert exp["short as 257 bytes"] is None and exp["empty ciphertext"] is None
    assert all(v is None for nm, v in exp.items() if nm.startswith("bad oaep"))
    assert all(exp[nm] == m for nm, m, _ in valid_ints(name))
    assert [c.expect is None for c in empty_label_case_set(name)] == [False, False, False, True]
