"""Both ciphers on blocks past 256 MiB and 512 MiB, bit for bit against the oracle and OpenSSL.

The blocks are those of tests/big_block_cases.py: the smallest lengths at
which the GCM counter's top byte, the high word of the GCM length block and
the lift exponents above bit 20 (GHASH: H^(2^k), Poly1305: r^(2^k)) are not
trivially zero.  A Seal / Open round trip cannot see a defect the two share,
so every output is compared with a reference: the tag with OpenSSL's
(tests/golden/big_blocks.json), the whole ciphertext with the oracle's and its
SHA-256 with OpenSSL's (tests/test_big_blocks_oracle.py ties the oracle to
OpenSSL and to the definitions at these counters), the CRC array with
checksum().

Per run: Seal with CRC_GEN; Open with one tag bit flipped, from the ciphertext
onto the buffer that holds the plaintext (ETAG, all zero); Open with
CRC_VERIFY in place (OK, the plaintext).  A and B run on the default context
and on a CTX_BITSLICE one, C on the default one.  Two layouts, asserted with
debug_plan (big_block_cases.check_plan):

  * alone: the block is the whole batch, cut into tasks of about len / 512
    (ChaCha: len / 2048), so tasks start at nonzero counters on both sides of
    the carry, one task has the carry inside it, and the block's thousands of
    partial slots take several rounds of the finalize.
  * whole (A): 1.75 GiB of device-generated, unchecked filler behind the block
    keeps 4 MiB tasks: every wave runs 256 KiB, 64 four-row periods and a
    refill of the counter window with U >= 0x10000; the task that holds
    offset 256 MiB - 32 is a full one.

One more GCM test seals the keystream of A's and B's length, so that the
ciphertext is all zero and the tag is E_K(J0) ^ (length block) * H with no
lift in it: it tells a wrong length block from wrong powers.

Each run is made once for the module (MEM_DEVICE only); the tests read its
results.  One block's host copies are alive at a time.  A ciphertext mismatch
is reported as the first and last differing block with their counters, the
first one's row mod 4 and lane, and its side of the top-byte carry.
"""
import hashlib

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import big_block_cases as BB

pytestmark = pytest.mark.gpu

GOLD = BB.load_golden()
ALGO = {BB.GCM: (E.AES256GCM, orc.AES256GCM), BB.CHACHA: (E.CHACHA20P1305, orc.CHACHA20P1305)}
CTX = {"default": 0, "bitslice": E.CTX_BITSLICE}
RUNS = [("A", "default", "alone"), ("A", "bitslice", "alone"), ("A", "default", "whole"), ("A", "bitslice", "whole"),
        ("B", "default", "alone"), ("B", "bitslice", "alone"), ("C", "default", "alone")]
FSEED = 0x42494746  # the filler's data and keys

_host = {}  # name -> the block's host values; at most one entry


def nseg(n):
    return max(1, -(-n // E.SEG))


def host(name):
    """P, the oracle's C, tag and checksum(P) of a block, computed once; asking for another block drops this one."""
    if name not in _host:
        _host.clear()
        key, nonce = BB.key_nonce(name)
        p = BB.case_plaintext(name)
        c, tag = orc.seal(ALGO[BB.CASES[name]["algo"]][1], key, nonce, p, fast=True)
        assert tag.hex() == GOLD[name]["tag"], "the oracle's tag is not OpenSSL's (tests/test_big_blocks_oracle.py)"
        _host[name] = {"key": key, "nonce": nonce, "p": p, "c": np.frombuffer(c, np.uint8), "tag": tag,
                       "crc": np.frombuffer(orc.checksum(p, hw=True), np.uint8)}
    return _host[name]


@pytest.fixture(scope="module", autouse=True)
def _drop_host_copies():
    yield
    _host.clear()


def run(name, ctx, layout):
    """Everything one engine computes for one block in one layout, reduced to what the tests assert."""
    BB.check_plan(name, layout)
    h, algo = host(name), BB.CASES[name]["algo"]
    n, cbytes = BB.CASES[name]["len"], 4 * nseg(BB.CASES[name]["len"])
    fill = BB.WHOLE_FILL if layout == "whole" else []
    eng = E.Engine(0, CTX[ctx])
    bufs = []

    def alloc(nbytes):
        bufs.append(eng.alloc(nbytes))
        return bufs[-1]

    def blocks(src, dst, tag, ftags=None):
        specs = [{"key": h["key"], "nonce": h["nonce"], "src": src.ptr, "dst": dst.ptr, "len": n, "crc": crc.ptr,
                  "tag": tag}]
        off = coff = 0
        for i, fn in enumerate(fill):  # in place, whatever it holds by now: never looked at
            specs.append({"key": fkeys[i][0], "nonce": fkeys[i][1], "src": fsrc.ptr + off, "dst": fsrc.ptr + off,
                          "len": fn, "crc": fcrc.ptr + coff, "tag": ftags[i] if ftags else None})
            off += fn
            coff += 4 * nseg(fn)
        return eng.make_blocks(specs)

    res = {}
    try:
        src, dst, crc = alloc(n), alloc(n), alloc(cbytes)
        if fill:
            fsrc, fcrc = alloc(sum(fill)), alloc(sum(4 * nseg(fn) for fn in fill))
            fkeys = [orc.gen_key(FSEED, i) for i in range(len(fill))]
            assert len(set(fill)) == 1
            eng.gen_synthetic_batch(fsrc, fill[0], fill, FSEED, 0)
        src.upload(h["p"])
        crc.upload(np.full(cbytes, 0xEE, np.uint8))
        # Seal with CRC_GEN
        arr, k = blocks(src, dst, None)
        eng.seal_batch(ALGO[algo][0], arr, k, E.CRC_GEN, E.MEM_DEVICE)
        res["seal"] = (arr[0].status, arr[0].crc_bad_seg, bytes(arr[0].tag))
        ftags = [bytes(arr[1 + i].tag) for i in range(len(fill))]
        got = dst.download(n)
        res["c_sha256"] = hashlib.sha256(got).hexdigest()
        res["c_diff"] = BB.describe_mismatch(algo, got, h["c"])
        del got
        got = crc.download(cbytes)
        res["crc_bad_segs"] = np.nonzero((got != h["crc"]).reshape(-1, 4).any(axis=1))[0][:8].tolist()
        # Open with one tag bit flipped: from the ciphertext onto the plaintext's buffer
        bad = bytearray(h["tag"])
        bad[7] ^= 0x10
        arr, k = blocks(dst, src, bytes(bad), ftags)
        eng.open_batch(ALGO[algo][0], arr, k, E.CRC_VERIFY, E.MEM_DEVICE)
        res["open_bad"] = (arr[0].status, int(np.count_nonzero(src.download(n))))
        # Open with CRC_VERIFY, in place, with OpenSSL's tag
        arr, k = blocks(dst, dst, bytes.fromhex(GOLD[name]["tag"]), ftags)
        eng.open_batch(ALGO[algo][0], arr, k, E.CRC_VERIFY, E.MEM_DEVICE)
        res["open"] = (arr[0].status, arr[0].crc_bad_seg)
        res["p_diff"] = BB.describe_mismatch(algo, dst.download(n), h["p"])
    finally:
        for b in bufs:
            b.free()
        eng.close()
    return res


@pytest.fixture(scope="module", params=RUNS, ids=["-".join(r) for r in RUNS])
def r(request):
    name, ctx, layout = request.param
    return dict(run(name, ctx, layout), name=name, what="%s (%s context, %s)" % request.param)


def test_seal_tag_is_openssls(r):
    status, bad_seg, tag = r["seal"]
    assert (status, bad_seg) == (E.OK, -1), r["what"]
    assert tag.hex() == GOLD[r["name"]]["tag"], r["what"] + ": tag"


def test_seal_ciphertext_is_the_oracles(r):
    if r["c_diff"] is not None:
        pytest.fail("%s: ciphertext: %s" % (r["what"], r["c_diff"]))
    assert r["c_sha256"] == GOLD[r["name"]]["c_sha256"], r["what"] + ": SHA-256 of the ciphertext against OpenSSL's"


def test_seal_crc_array_is_checksum(r):
    assert r["crc_bad_segs"] == [], "%s: CRC array differs from checksum() in segments %s" % (
        r["what"], r["crc_bad_segs"])


def test_open_verify_in_place(r):
    assert r["open"] == (E.OK, -1), r["what"]
    if r["p_diff"] is not None:
        pytest.fail("%s: opened plaintext: %s" % (r["what"], r["p_diff"]))


def test_open_with_a_flipped_tag_bit_releases_nothing(r):
    status, nonzero = r["open_bad"]
    assert status == E.ETAG, r["what"]
    assert nonzero == 0, "%s: %d nonzero output bytes after ETAG" % (r["what"], nonzero)


@pytest.mark.parametrize("name", [n for n, c in BB.CASES.items() if c["algo"] == BB.GCM])
def test_tag_of_an_all_zero_ciphertext_is_the_length_block(name):
    """Seal of zeros gives the keystream, Seal of the keystream gives zeros: every
    GHASH partial is zero and nothing is lifted, so the tag is E_K(J0) ^ (length
    block) * H (OpenSSL's value) whatever the keystream and the finalize's
    powers are.  A wrong tag here is the keysetup's length block (B: its high
    word); a right one next to a wrong tag above is the lifts."""
    key, nonce = BB.key_nonce(name)
    n = BB.CASES[name]["len"]
    eng = E.Engine(0)
    buf, crc = eng.alloc(n), eng.alloc(4 * nseg(n))
    try:
        buf.upload(np.zeros(n, np.uint8))
        for _ in range(2):  # in place: zeros -> keystream -> zeros
            arr, k = eng.make_blocks([{"key": key, "nonce": nonce, "src": buf.ptr, "dst": buf.ptr, "len": n,
                                       "crc": crc.ptr}])
            eng.seal_batch(E.AES256GCM, arr, k, E.CRC_NONE, E.MEM_DEVICE)
            assert arr[0].status == E.OK
        tag = bytes(arr[0].tag)
        nonzero = int(np.count_nonzero(buf.download(n)))
    finally:
        buf.free()
        crc.free()
        eng.close()
    assert nonzero == 0, "Seal of the keystream left %d nonzero bytes" % nonzero
    assert tag.hex() == GOLD[name]["zero_c_tag"], name + ": E_K(J0) ^ (length block) * H"
