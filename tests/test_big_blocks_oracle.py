"""The oracle on the three big blocks of tests/big_block_cases.py, against OpenSSL and the definitions.

Every large GPU comparison is made with oracle.seal(..., fast=True), whose
AES-NI path had met nothing else at a counter above 2^20 or a length above
2^32 bits.  Here it (and for ChaCha the plain path) reproduces OpenSSL's tag,
ciphertext hash and edge samples (tests/golden/big_blocks.json) for blocks of
256 MiB and 512 MiB.  Two checks use the definitions alone: the keystream at
every sampled GCM position is E_K(nonce || BE32(2 + offset / 16)), and the tag
of an all-zero ciphertext of a block's length is E_K(J0) ^ (length block) * H,
which holds the 64-bit length encoding and no bulk GHASH.  The last test
asserts the plans that tests/test_gpu_big_blocks.py relies on.

Each block is generated and sealed once for the module, one block at a time.
"""
import hashlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import big_block_cases as BB

GOLD = BB.load_golden()
ORC = {BB.GCM: orc.AES256GCM, BB.CHACHA: orc.CHACHA20P1305}
GCM_CASES = [n for n, c in BB.CASES.items() if c["algo"] == BB.GCM]


@pytest.fixture(scope="module", params=list(BB.CASES))
def sealed(request):
    """(name, P, the oracle's C, its tag): one block alive at a time"""
    name = request.param
    key, nonce = BB.key_nonce(name)
    p = BB.case_plaintext(name)
    c, tag = orc.seal(ORC[BB.CASES[name]["algo"]], key, nonce, p, fast=True)
    return name, p, np.frombuffer(c, np.uint8), tag


def p_range(name, lo, hi):
    a = lo // 8 * 8
    return BB.plaintext(BB.CASES[name]["seed"], hi - a, start=a)[lo - a:]


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def test_plaintext_is_the_pinned_stream(sealed):
    name, p, _, _ = sealed
    assert p.size == BB.CASES[name]["len"]
    assert hashlib.sha256(p).hexdigest() == GOLD[name]["p_sha256"]
    # any range of it on its own (the keystream test reads only the windows)
    for _, lo, hi in BB.windows(name):
        assert np.array_equal(p_range(name, lo, hi), p[lo:hi]), (lo, hi)


def test_oracle_seal_matches_openssl(sealed):
    name, _, c, tag = sealed
    g = GOLD[name]
    for w in g["samples"]:
        got, want = c[w["lo"]:w["hi"]], np.frombuffer(bytes.fromhex(w["c"]), np.uint8)
        assert np.array_equal(got, want), "%s: ciphertext at the %s edge, bytes %d..%d: %s" % (
            name, w["edge"], w["lo"], w["hi"], BB.describe_mismatch(g["algo"], got, want))
    assert hashlib.sha256(c).hexdigest() == g["c_sha256"], name + ": ciphertext differs from OpenSSL's outside the samples"
    assert tag.hex() == g["tag"], name + ": tag"


def test_oracle_open_matches_openssl(sealed):
    name, p, c, _ = sealed
    key, nonce = BB.key_nonce(name)
    algo = ORC[BB.CASES[name]["algo"]]
    got = orc.open_(algo, key, nonce, c, bytes.fromhex(GOLD[name]["tag"]), fast=True)
    assert got is not None, name + ": OpenSSL's tag rejected"
    assert BB.describe_mismatch(BB.CASES[name]["algo"], np.frombuffer(got, np.uint8), p) is None
    del got
    bad = bytearray.fromhex(GOLD[name]["tag"])
    bad[15] ^= 0x01
    assert orc.open_(algo, key, nonce, c, bytes(bad), fast=True) is None, name + ": a flipped tag bit accepted"


@pytest.mark.parametrize("name", GCM_CASES)
def test_gcm_keystream_at_the_sampled_counters(name):
    """C ^ P of OpenSSL's samples is E_K(nonce || BE32(2 + offset / 16)), block by block."""
    key, nonce = BB.key_nonce(name)
    seen = set()
    for w in GOLD[name]["samples"]:
        lo, hi = w["lo"], w["hi"]
        ks = xor(bytes.fromhex(w["c"]), p_range(name, lo, hi).tobytes())
        for b in range(lo // 16, -(-hi // 16)):
            ctr = 2 + b
            want = orc.aes256_encrypt_block(key, nonce + ctr.to_bytes(4, "big"))
            a, e = max(lo, 16 * b), min(hi, 16 * b + 16)
            assert ks[a - lo:e - lo] == want[a - 16 * b:e - 16 * b], "%s: keystream of counter 0x%08x (%s edge)" % (
                name, ctr, w["edge"])
            seen.add(ctr)
    # both sides of each carry, and for B the far side of 512 MiB
    for ctr in (2, 0xFFFF, 0x10000, 0xFFFFFF, 0x1000000) + ((0x2000001, 0x2000002) if name == "B" else ()):
        assert ctr in seen, hex(ctr)
    assert max(seen) == 2 + (BB.CASES[name]["len"] - 1) // 16


@pytest.mark.parametrize("name", GCM_CASES)
def test_gcm_length_block(name):
    """With an all-zero ciphertext GHASH is (length block) * H alone, so the tag
    is E_K(J0) ^ L * H, L = 0^64 || BE64(8 * len); the tag of the empty message
    is E_K(J0).  For B the high word of the bit count is 1."""
    key, nonce = BB.key_nonce(name)
    n = BB.CASES[name]["len"]
    assert (8 * n) >> 32 == (1 if name == "B" else 0)
    ej0 = orc.aes256_encrypt_block(key, nonce + b"\x00\x00\x00\x01")
    h = orc.aes256_encrypt_block(key, bytes(16))
    for fast in (True, False):
        assert orc.seal(orc.AES256GCM, key, nonce, np.zeros(0, np.uint8), fast=fast) == (b"", ej0)
    want = xor(ej0, orc.gf128_mul(bytes(8) + (8 * n).to_bytes(8, "big"), h))
    assert want.hex() == GOLD[name]["zero_c_tag"], "the definition against OpenSSL"
    ks, _ = orc.seal(orc.AES256GCM, key, nonce, np.zeros(n, np.uint8), fast=True)
    ks = np.frombuffer(ks, np.uint8)
    c, tag = orc.seal(orc.AES256GCM, key, nonce, ks, fast=True)
    assert not np.frombuffer(c, np.uint8).any()
    assert tag == want, name + ": the oracle's length block"


@pytest.mark.parametrize("name,layout", [("A", "alone"), ("B", "alone"), ("C", "alone"), ("A", "whole")])
def test_plans_the_gpu_test_relies_on(name, layout):
    tb, nslots, mine = BB.check_plan(name, layout)
    want = {("A", "alone"): 576 * BB.KIB, ("B", "alone"): 1088 * BB.KIB, ("C", "alone"): 256 * BB.KIB,
            ("A", "whole"): 4 * BB.MIB}[name, layout]
    assert tb == want, "task bytes"
