"""Generate tests/golden/big_blocks.json -- OpenSSL's results for the three big blocks.

Run on the development machine, never on the GPU box (it needs libcrypto and
about 2 GiB of memory; a minute or so):
    python tests/golden/make_big_blocks.py

Source of truth: OpenSSL 3 libcrypto through ctypes, EVP aes-256-gcm and
chacha20-poly1305, as tests/golden/make_golden.py.  Neither the oracle nor a
kernel is involved.  The cases and the plaintext stream come from
tests/big_block_cases.py; the stream's first words are checked here against
SplitMix64 in Python integers, and the SHA-256 of every plaintext is kept, so
the fixture pins the generator too.

Per case the file keeps the parameters, the tag, the SHA-256 of the whole
ciphertext and the ciphertext bytes 64 either side of each edge
(big_block_cases.windows).  For the GCM cases it also keeps the tag of the
message of the same length whose ciphertext is all zero (the plaintext is the
keystream): E_K(J0) ^ (length block) * H, with no bulk GHASH in it.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import big_block_cases as BB  # noqa: E402
from tests.golden.make_golden import OpenSSL, mix64, GOLDEN  # noqa: E402

PIECE = 64 << 20  # bytes per EVP_EncryptUpdate: its length is an int


def seal(ssl, algo, key, nonce, p):
    """(ciphertext as uint8 array, tag) of the numpy bytes p, fed in pieces."""
    L = ssl.L
    ctx = L.EVP_CIPHER_CTX_new()
    cipher = L.EVP_aes_256_gcm() if algo == BB.GCM else L.EVP_chacha20_poly1305()
    assert L.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
    assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, len(nonce), None) == 1
    assert L.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
    p = np.ascontiguousarray(p)
    c = np.empty(p.size + 32, np.uint8)
    outl, total = ctypes.c_int(), 0
    for off in range(0, p.size, PIECE):
        n = min(PIECE, p.size - off)
        assert L.EVP_EncryptUpdate(ctx, ctypes.c_void_p(c.ctypes.data + total), ctypes.byref(outl),
                                   ctypes.c_void_p(p.ctypes.data + off), n) == 1
        total += outl.value
    assert L.EVP_EncryptFinal_ex(ctx, ctypes.c_void_p(c.ctypes.data + total), ctypes.byref(outl)) == 1
    total += outl.value
    tag = ctypes.create_string_buffer(16)
    assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tag) == 1
    L.EVP_CIPHER_CTX_free(ctx)
    assert total == p.size
    return c[:total], tag.raw


def main():
    ssl = OpenSSL()
    cases = {}
    for name, cs in BB.CASES.items():
        key, nonce = BB.key_nonce(name)
        p = BB.case_plaintext(name)
        # the stream against Python integers: the first words, and a few at the far end
        words = p[:p.size // 8 * 8].view("<u8")
        for k in list(range(64)) + [words.size - 1, words.size // 2, (1 << 25) + 5]:
            assert int(words[k]) == mix64(cs["seed"] + GOLDEN * (k + 1)), (name, k)
        assert np.array_equal(BB.plaintext(cs["seed"], 4096 + 3, start=BB.TOP), p[BB.TOP:BB.TOP + 4099])
        c, tag = seal(ssl, cs["algo"], key, nonce, p)
        v = {"algo": cs["algo"], "len": cs["len"], "seed": cs["seed"], "key": cs["key"], "nonce": cs["nonce"],
             "p_sha256": hashlib.sha256(p).hexdigest(), "c_sha256": hashlib.sha256(c).hexdigest(), "tag": tag.hex(),
             "samples": [{"edge": e, "lo": lo, "hi": hi, "c": c[lo:hi].tobytes().hex()}
                         for e, lo, hi in BB.windows(name)]}
        if cs["algo"] == BB.GCM:
            ks, _ = seal(ssl, cs["algo"], key, nonce, np.zeros(cs["len"], np.uint8))
            z, ztag = seal(ssl, cs["algo"], key, nonce, ks)
            assert not z.any()
            v["zero_c_tag"] = ztag.hex()
        cases[name] = v
        print(name, cs["algo"], cs["len"], tag.hex(), v["c_sha256"][:16])
    with open(BB.GOLDEN_JSON, "w") as f:
        json.dump({"generator": "tests/golden/make_big_blocks.py (OpenSSL EVP; plaintext of tests/big_block_cases.py)",
                   "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
