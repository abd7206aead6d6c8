"""Three blocks past 256 MiB and 512 MiB: the cases, their data and what a mismatch means.

The GCM counter of a 16-byte block is 2 + offset / 16, and the interface has
no way to start a block at a higher counter, so the smallest block whose
counter has a nonzero top byte is 256 MiB - 32 bytes long, and the smallest
whose length block has a nonzero high word is 512 MiB long.  Three blocks
reach what shorter ones cannot:

  A  GCM     256 MiB + 96 KiB + 1000   the counter's carry into its top byte
                                       (offset 256 MiB - 32: lanes 62 and 63 of
                                       a row = 3 mod 4), then full rows and a
                                       ragged tail with the top byte set
  B  GCM     512 MiB + 64 KiB + 17     all of A's points, bits >> 32 = 1 in the
                                       length block, more than 2^25 16-byte
                                       blocks (GHASH lift exponents to bit 25)
  C  ChaCha  256 MiB + 96 KiB + 1000   Poly1305 slot exponents up to bit 24
                                       (ChaCha's own counter, 1 + offset / 64,
                                       stays below 2^24: its top byte needs 1 GiB)

tests/golden/big_blocks.json holds, from OpenSSL (tests/golden/make_big_blocks.py),
each block's tag, the SHA-256 of its ciphertext and the ciphertext 64 bytes
either side of each edge.  The plaintext is a function of (seed, length) alone:
SplitMix64 in 64-bit integer arithmetic, word k = mix64(seed + GOLDEN * (k + 1)),
little-endian, cut to the length.
"""
import json
import os

import numpy as np

KIB, MIB = 1 << 10, 1 << 20
GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_blocks.json")

GCM, CHACHA = "aes256gcm", "chacha20poly1305"
TOP = 256 * MIB - 32  # the GCM counter becomes 0x01000000 here

CASES = {
    "A": {"algo": GCM, "len": 256 * MIB + 96 * KIB + 1000, "seed": 0x4249474131,
          "key": "6a09e667f3bcc908bb67ae8584caa73b3c6ef372fe94f82ba54ff53a5f1d36f1",
          "nonce": "510e527fade682d19b05688c"},
    "B": {"algo": GCM, "len": 512 * MIB + 64 * KIB + 17, "seed": 0x4249474232,
          "key": "cbbb9d5dc1059ed8629a292a367cd5079159015a3070dd17152fecd8f70e5939",
          "nonce": "67332667ffc00b318eb44a87"},
    "C": {"algo": CHACHA, "len": 256 * MIB + 96 * KIB + 1000, "seed": 0x4249474333,
          "key": "2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe",
          "nonce": "243f6a8885a308d313198a2e"},
}


# "whole tasks": enough unchecked filler behind A that the plan keeps 4 MiB GCM tasks
WHOLE_FILL = [8 * MIB] * 224


def key_nonce(name):
    c = CASES[name]
    return bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"])


def cipher_block(algo):
    """bytes per counter step"""
    return 16 if algo == GCM else 64


def counter_at(algo, off):
    """the block counter of the cipher block that holds byte off"""
    return 2 + off // 16 if algo == GCM else 1 + off // 64


def edges(name):
    """(edge name, offset) in offset order.  The carry edges name the first byte
    whose counter has the new byte set; "top" is that of the GCM counter's top
    byte (for C a position marker only: ChaCha's counter is 0x400000 there)."""
    c = CASES[name]
    n, gcm = c["len"], c["algo"] == GCM
    e = [("start", 0), ("byte2", MIB - 32 if gcm else 4 * MIB - 64), ("top", TOP)]
    if n > 512 * MIB:
        e.append(("len32", 512 * MIB))
    return e + [("end", n)]


def windows(name):
    """(edge name, lo, hi): the sampled byte ranges, 64 bytes either side of each edge"""
    n = CASES[name]["len"]
    return [(e, max(0, off - 64), min(n, off + 64)) for e, off in edges(name)]


# ---------------------------------------------------------------------------
# plaintext

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_CHUNK = 1 << 17  # words per pass: the temporaries stay in the cache


def plaintext(seed, length, start=0):
    """Bytes [start, start + length) of the stream of `seed` (start a multiple of 8)."""
    assert start % 8 == 0
    nw = (length + 7) // 8
    out = np.empty(nw, np.uint64)
    k = np.arange(1, _CHUNK + 1, dtype=np.uint64)
    t = np.empty(_CHUNK, np.uint64)
    s30, s27, s31 = np.uint64(30), np.uint64(27), np.uint64(31)
    with np.errstate(over="ignore"):
        for w0 in range(0, nw, _CHUNK):
            m = min(_CHUNK, nw - w0)
            z, tt = out[w0:w0 + m], t[:m]
            # seed + GOLDEN * (k + 1) mod 2^64, k the word's index in the stream
            base = (seed + 0x9E3779B97F4A7C15 * (start // 8 + w0)) & 0xFFFFFFFFFFFFFFFF
            np.multiply(k[:m], _GOLDEN, out=z)
            z += np.uint64(base)
            np.right_shift(z, s30, out=tt)
            z ^= tt
            z *= _M1
            np.right_shift(z, s27, out=tt)
            z ^= tt
            z *= _M2
            np.right_shift(z, s31, out=tt)
            z ^= tt
    return out.astype("<u8", copy=False).view(np.uint8)[:length]


def case_plaintext(name):
    c = CASES[name]
    return plaintext(c["seed"], c["len"])


def load_golden():
    with open(GOLDEN_JSON) as f:
        g = json.load(f)
    for name, c in CASES.items():
        v = g["cases"][name]
        assert (v["algo"], v["len"], v["seed"], v["key"], v["nonce"]) == (
            c["algo"], c["len"], c["seed"], c["key"], c["nonce"]), "big_blocks.json was made for other cases: " + name
        assert [(w["edge"], w["lo"], w["hi"]) for w in v["samples"]] == windows(name), name
    return g["cases"]


# ---------------------------------------------------------------------------
# the two batch layouts, as the planner cuts them


def batch_lens(name, layout):
    return [CASES[name]["len"]] + (WHOLE_FILL if layout == "whole" else [])


def check_plan(name, layout):
    """Assert what the GPU test relies on in the plan of the batch (host only).

    alone: the block is the whole batch, so it is cut into about 512 (GCM) or
    2048 (ChaCha) tasks: tasks start at nonzero counters with the top byte
    clear and (B) set, one GCM task has the carry inside it, and the block
    has thousands of partial slots, several rounds of the 1024-thread GCM
    finalize, with lift exponents as long as the block's count of 16-byte
    blocks.  whole (GCM): 4 MiB tasks, and the one that holds the carry is a
    full one, so every wave runs 256 KiB of it.  Returns (task bytes, slots,
    the block's tasks)."""
    from juicefs_amd import engine as E

    c = CASES[name]
    n, gcm = c["len"], c["algo"] == GCM
    tb, nslots, tasks = E.debug_plan(E.PLAN_GCM if gcm else E.PLAN_CHACHA, batch_lens(name, layout))
    mine = [(c0, c1) for b, c0, c1 in tasks if b == 0]
    assert sorted(mine) == [(c0, min(c0 + tb, n)) for c0 in range(0, n, tb)], "the block's tasks tile it"
    if layout == "whole":
        assert gcm and tb == 4 * MIB, "the filler keeps 4 MiB tasks"
        assert (TOP // tb * tb, TOP // tb * tb + 4 * MIB) in mine, "the task with the top-byte carry is a full one"
        assert (256 * MIB, n) in mine, "and the next one starts with the counter's top byte set"
        return tb, nslots, mine
    unit, want = (64 * KIB, 512) if gcm else (128 * KIB, 2048)
    assert tb == -(-(n // want) // unit) * unit and tb < (4 * MIB if gcm else MIB), "a small batch: cut for the CUs"
    assert len(tasks) == len(mine) and nslots == (16 if gcm else 4) * len(mine)
    assert nslots > 4 * 1024, "several rounds of a 1024-thread finalize"
    assert any(0 < c0 < TOP for c0, _ in mine), "a task starts at a nonzero counter below 2^24"
    if gcm:
        assert any(c0 < TOP - 1024 and c1 > TOP + 1024 for c0, c1 in mine), "the carry lies inside a task"
        # (A's 576 KiB task with the carry is its last one; its whole layout has the task from 256 MiB)
        assert name == "A" or any(c0 >= TOP + 32 for c0, _ in mine), "a task starts with the counter's top byte set"
    assert ((n + 15) // 16).bit_length() >= (26 if n > 512 * MIB else 25), "lift exponents up to this bit"
    return tb, nslots, mine


# ---------------------------------------------------------------------------
# what a mismatch says


def describe_mismatch(algo, got, want):
    """None if the arrays are equal; else where they differ, in the kernels'
    terms: the first and last differing cipher block with their counters, the
    first one's row and lane (rows of 64 cipher blocks from the block's start,
    as the T-table GCM kernel and the ChaCha kernel walk them; tasks start on
    multiples of 64 rows), and on which side of the top-byte carry the
    differences lie.  No buffer contents."""
    if got.size != want.size:
        return "%d bytes, expected %d" % (got.size, want.size)
    if np.array_equal(got, want):
        return None
    d = got != want
    first, last = int(d.argmax()), int(d.size - 1 - d[::-1].argmax())
    cb = cipher_block(algo)
    pad = np.zeros(-(-d.size // cb) * cb, bool)
    pad[:d.size] = d
    nbad = int(pad.reshape(-1, cb).any(axis=1).sum())
    fb, lb = first // cb, last // cb
    row = fb // 64  # a wave's row: 64 lanes, one cipher block each
    if algo == GCM:
        where = "row %d (= %d mod 4), lane %d" % (row, row % 4, fb % 64)
        side = ("all at or after the top-byte carry (block 0x%x)" % (TOP // 16) if first >= TOP else
                "all before the top-byte carry" if last < TOP else "on both sides of the top-byte carry")
    else:
        where = "row %d, lane %d" % (row, fb % 64)
        side = "ChaCha has no counter edge in this block"
    return "%d of %d %d-byte blocks differ: first block 0x%x (counter 0x%08x, byte %d, %s), last block 0x%x " \
           "(counter 0x%08x); %s" % (nbad, -(-d.size // cb), cb, fb, counter_at(algo, first), first, where, lb,
                                     counter_at(algo, last), side)
