"""tests/rsa_model.py at k = 512: the pure-Python statement of the RSA-OAEP key
unwrap and wrap for a 4096-bit key (rsa.DecryptOAEP / rsa.EncryptOAEP with
SHA-256 and the label "keys", pkg/object/encrypt.go:124-134), for the RSA-4096
tests.  Python integers and hashlib only; what rsa_model.py already takes a
length for (the OAEP encoding, MGF1, the key derivation, the byte streams) is
imported from there.

The private operation is pow(c, d, n), without the CRT, so the model shares no
structure with jfsx_rsa.h.  The predicates read the model's own integers; the
tests use them to prove that their inputs reach the paths they are meant to.

fixed_keys() and case_set() build the fixed keys of
tests/golden/rsa_keys_4096.json and, per key, the ciphertext set every wide RSA
test submits (cached: pow(c, d, n) costs tens of milliseconds in Python)."""
import functools
import json
import os

from tests.rsa_model import (Case, E, HLEN, Key, components as _components, det_bytes,  # noqa: F401
                             key, m1_lt_m2, m2_ge_p, oaep_decode)
from tests.rsa_model import oaep_encode as _oaep_encode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rsa_keys_4096.json")

K = 512            # modulus bytes (RSA-4096)
PRIME_BYTES = 256
MAX_MSG = K - 2 * HLEN - 2   # 446
R = 1 << 2048      # the radix of the input reduction's split c = hi R + lo


def components(k):
    """(p, q, dp, dq, qinv), big-endian, 256 bytes each: what Engine.rsa_key takes."""
    return _components(k, PRIME_BYTES)


def oaep_encode(msg, seed, label=b"keys", patch=None):
    return _oaep_encode(msg, seed, label=label, patch=patch, k=K)


def ct512(c):
    return c.to_bytes(K, "big")


# pow(c, d, n) at 4096 bits costs 0.2 s in Python, and the case sets hold
# hundreds of ciphertexts.  Those the model made itself it need not take apart
# again: RSADP inverts RSAEP (c = m^e mod n with m < n gives m back, RFC 8017
# 5.1), so decrypt() looks such a c up.  test_rsa4096.py checks the lookup
# against pow(c, d, n) on a sample of every kind; every other ciphertext (range
# edges, short ones) goes through pow.
_MADE = {}


def encrypt_em(k, em):
    """RSAEP of an encoded message (or any integer below n), as an integer."""
    m = em if isinstance(em, int) else int.from_bytes(bytes(em), "big")
    assert m < k.n
    c = pow(m, E, k.n)
    _MADE[(k.n, c)] = m
    return c


def rsadp(k, c, lookup=True):
    m = _MADE.get((k.n, c)) if lookup else None
    return pow(c, k.d, k.n) if m is None else m


def encrypt(k, msg, seed, label=b"keys"):
    """rsa.EncryptOAEP with the 32 bytes it would read from rand: the 512-byte
    ciphertext, or None for "message too long for RSA key size"."""
    if len(msg) > MAX_MSG:
        return None
    return ct512(encrypt_em(k, oaep_encode(msg, seed, label=label)))


def decrypt(k, ct, label=b"keys", lookup=True):
    """rsa.DecryptOAEP: the message, or None for "crypto/rsa: decryption
    error".  A ciphertext longer than the modulus is an error, a shorter one is
    a big-endian integer all the same (an empty one as well: the engine takes
    ct_len 0 as the error, and 0 decodes to it anyway), c >= n is an error."""
    ct = bytes(ct)
    if len(ct) > K or not ct:
        return None
    c = int.from_bytes(ct, "big")
    if c >= k.n:
        return None
    return oaep_decode(rsadp(k, c, lookup).to_bytes(K, "big"), label)


def reduce_corrections(m, c):
    """How many times m comes off ((c >> 2048) 2^2048 mod m) + (c mod 2^2048),
    the sum the input reduction forms for a 2048-bit m: 0, 1 or 2."""
    t = ((c >> 2048) * R) % m + c % R
    assert t // m <= 2
    return t // m


@functools.lru_cache(maxsize=None)
def fixed_keys():
    """name -> Key, in the file's order."""
    with open(GOLDEN) as f:
        rows = json.load(f)["keys"]
    return {r["name"]: key(int(r["p"], 16), int(r["q"], 16)) for r in rows}


VALID_LENGTHS = (0, 1, 31, 32, 33, MAX_MSG)
VALID_SEEDS = 3  # 6 lengths x 3 seeds = 18 valid messages per key


def valid_inputs(name):
    """[(case name, message, seed)] of the valid messages: what a wrap test submits."""
    return [("valid len %d seed %d" % (n, s), det_bytes(n, name, "wide msg", n, s),
             det_bytes(HLEN, name, "wide seed", n, s)) for n in VALID_LENGTHS for s in range(VALID_SEEDS)]


@functools.lru_cache(maxsize=None)
def valid_ints(name):
    """[(case name, message, ciphertext integer)] of the valid messages."""
    k = fixed_keys()[name]
    return [(nm, msg, encrypt_em(k, oaep_encode(msg, seed))) for nm, msg, seed in valid_inputs(name)]


@functools.lru_cache(maxsize=None)
def short_ciphertext(name):
    """(message, seed, c) with c < 2^4088, so its big-endian form has a zero first byte."""
    k = fixed_keys()[name]
    for s in range(100000):
        msg, seed = det_bytes(32, name, "wide short msg", s), det_bytes(HLEN, name, "wide short seed", s)
        c = encrypt_em(k, oaep_encode(msg, seed))
        if c < 1 << 4088:
            return msg, seed, c
    raise AssertionError("no short ciphertext for " + name)


def _set(db, i, v):
    db[i] = v


def _flip(db, i):
    db[i] ^= 0x80


@functools.lru_cache(maxsize=None)
def case_set(name):
    """Every Case of one fixed key under the label "keys"; expect is the
    model's decrypt (bytes or None)."""
    k = fixed_keys()[name]
    n = k.n
    items = [(nm, ct512(c)) for nm, _, c in valid_ints(name)]
    # lengths: Go takes any length up to the modulus as an integer
    _, _, c = short_ciphertext(name)
    items += [("short as 512 bytes", ct512(c)), ("short as 511 bytes", c.to_bytes(K - 1, "big")),
              ("513 bytes", b"\0" + ct512(c)), ("empty ciphertext", b""),
              ("256 bytes", det_bytes(256, name, "wide 256-byte ciphertext")), ("1 byte", b"\x02")]
    # range edges
    made = [("0", 0), ("1", 1), ("n-1", n - 1), ("p^e", k.p), ("(q(p-1))^e", k.q * (k.p - 1))]
    items += [("edge c = " + nm, ct512(encrypt_em(k, v))) for nm, v in made]  # 0, 1 and n - 1 are their own powers
    edges = [("n", n), ("n+1", n + 1), ("2^4096-1", (1 << 4096) - 1), ("p", k.p), ("2^2048", R)]
    items += [("edge c = " + nm, ct512(v)) for nm, v in edges]
    # arithmetically valid, bad OAEP, each rejection alone
    msg = det_bytes(32, name, "wide bad msg")

    def seed(i):
        return det_bytes(HLEN, name, "wide bad seed", i)
    bad = [("wrong label hash", oaep_encode(msg, seed(0), patch=lambda db: _flip(db, 5)))]
    em = oaep_encode(msg, seed(1))
    em[0] = 1
    assert int.from_bytes(em, "big") < n  # 2^4089 > EM >= 2^4088, n > 2^4094
    bad.append(("first byte 1", em))
    bad.append(("no separator", oaep_encode(b"", seed(2), patch=lambda db: _set(db, len(db) - 1, 0))))
    bad.append(("0x02 before the separator", oaep_encode(msg, seed(3), patch=lambda db: _set(db, 40, 2))))
    items += [("bad oaep: " + nm, ct512(encrypt_em(k, em))) for nm, em in bad]
    return tuple(Case(nm, ct, decrypt(k, ct)) for nm, ct in items)


CRT_PATH_KEYS = ("top", "wide_q_gt_p", "plain_q_gt_p")


@functools.lru_cache(maxsize=None)
def path_stats(name):
    """Counts over the valid messages of one key, from the predicates above."""
    k = fixed_keys()[name]
    cs = [c for _, _, c in valid_ints(name)]
    # the CRT halves cost a 2048-bit pow each: only for the keys whose paths are asserted
    crt = name in CRT_PATH_KEYS
    ge = [m2_ge_p(k, c) for c in cs] if crt else []
    lt = [m1_lt_m2(k, c) for c in cs] if crt else []
    return {"valid": len(cs), "m2_ge_p": sum(ge), "m1_lt_m2": sum(lt),
            "m2_ge_p_and_m1_lt_m2": sum(a and b for a, b in zip(ge, lt)),
            "corrections_p": tuple(sum(reduce_corrections(k.p, c) == i for c in cs) for i in range(3)),
            "corrections_q": tuple(sum(reduce_corrections(k.q, c) == i for c in cs) for i in range(3))}


def assert_reaches_paths(name):
    """The inputs of case_set(name) reach the paths the key is there for.
    Read from the model alone, before any engine result is looked at; if a
    condition fails, the seeds change, not the condition."""
    s = path_stats(name)
    assert s["valid"] == len(VALID_LENGTHS) * VALID_SEEDS, (name, s)
    if name in CRT_PATH_KEYS:
        assert 0 < s["m1_lt_m2"] < s["valid"], (name, s)  # m1 - m2 with and without the borrow
    if name == "wide_q_gt_p":
        assert s["m2_ge_p"] >= 4, (name, s)
        # m2 >= p and m1 < m2 - p: the inputs whose result changes if m2 is not reduced mod p
        assert s["m2_ge_p_and_m1_lt_m2"] >= 2, (name, s)
    if name == "bottom":  # both corrections of the input reduction, for either prime
        assert s["corrections_p"][2] >= 1 and s["corrections_q"][2] >= 1, (name, s)
        assert s["corrections_p"][1] >= 1 and s["corrections_q"][1] >= 1, (name, s)
    if name == "top":     # and none at all
        assert s["corrections_p"][0] >= 1 and s["corrections_q"][0] >= 1, (name, s)
    exp = {c.name: c.expect for c in case_set(name)}
    msg, _, _ = short_ciphertext(name)
    assert exp["short as 512 bytes"] == exp["short as 511 bytes"] == msg
    assert exp["513 bytes"] is None and exp["empty ciphertext"] is None
    assert exp["256 bytes"] is None and exp["1 byte"] is None
    assert exp["edge c = n-1"] is None and exp["edge c = 0"] is None
    assert exp["edge c = n"] is None and exp["edge c = n+1"] is None and exp["edge c = 2^4096-1"] is None
    assert all(v is None for nm, v in exp.items() if nm.startswith("bad oaep"))
    assert all(exp[nm] == m for nm, m, _ in valid_ints(name))
