"""The ChaCha20-Poly1305 kernels on ciphertexts crafted to drive their Poly1305
limb arithmetic to its carry edges (tests/poly_cases.py): a final accumulator
of 0, 1, 4, p - 1, p - 5, 2^128 - 1, 2^128, h + s rippling through every word
or through none; a lane's lifted partial of 0 or p - 1; two partner lanes of
the wave sum adding up to exactly p or 2p - 2; a whole wave summing to zero
(the zero-partial skip of finalize); all-0xFF and all-0x00 data.  Random bytes
reach none of these (2^-26 or less per operation).

Poly1305 runs over the ciphertext: Open is given the crafted bytes, Seal the
plaintext crafted ^ keystream.  The expected tag is tests/poly_model.py's, on
Python integers; plaintext bytes and CRCs are the oracle's.  That the inputs
reach the states they are named for is shown on the CPU by
tests/test_poly1305.py::test_emulation_on_crafted_ciphertexts."""
import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import poly_cases as PC

pytestmark = pytest.mark.gpu

CP = E.CHACHA20P1305


def nseg(n):
    return max(1, -(-n // E.SEG))


class Run:
    """Every case as one block of three device batches: Open with the true
    tag, Open with one tag bit flipped, Seal of the oracle's plaintext."""

    def __init__(self, eng):
        self.cases = cs = PC.cases()
        assert max(c.n for c in cs) <= 256 << 10
        lens = [c.n for c in cs]
        # the single-block layouts the cases were crafted for hold in the batch: the same task size
        assert E.debug_plan(E.PLAN_CHACHA, lens)[0] == E.debug_plan(E.PLAN_CHACHA, [lens[0]])[0] == 128 << 10
        self.plain = [orc.open_(orc.CHACHA20P1305, c.key, c.nonce, c.c, c.tag) for c in cs]
        off, o = [], 0
        for n in lens:
            off.append(o)
            o += (n + 255) & ~255
        coff, co = [], 0
        for n in lens:
            coff.append(co)
            co += 4 * nseg(n)
        src, dst, crc = eng.alloc(o), eng.alloc(o), eng.alloc(co)

        def batch(op, datas, tags):
            dst.upload(np.full(o, 0xA5, np.uint8))
            crc.upload(np.full(co, 0xA5, np.uint8))
            for c, d, f in zip(cs, datas, off):
                src.upload(np.frombuffer(d, np.uint8), f)
            arr, n = eng.make_blocks({"key": c.key, "nonce": c.nonce, "src": src.ptr + f, "dst": dst.ptr + f,
                                      "len": c.n, "tag": t, "crc": crc.ptr + g}
                                     for c, t, f, g in zip(cs, tags, off, coff))
            op(CP, arr, n, E.CRC_GEN, E.MEM_DEVICE)
            return [(arr[i].status, bytes(arr[i].tag), dst.download(c.n, off[i]).tobytes(),
                     crc.download(4 * nseg(c.n), coff[i]).tobytes()) for i, c in enumerate(cs)]

        try:
            self.open = batch(eng.open_batch, [c.c for c in cs], [c.tag for c in cs])
            self.open_bad = batch(eng.open_batch, [c.c for c in cs], [flip(c.tag, i) for i, c in enumerate(cs)])
            self.seal = batch(eng.seal_batch, self.plain, [None] * len(cs))
        finally:
            for b in (src, dst, crc):
                b.free()


def flip(tag, i):
    """one bit of the tag, a different one from case to case"""
    bit = (37 * i + 5) % 128
    t = bytearray(tag)
    t[bit // 8] ^= 1 << (bit % 8)
    return bytes(t)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def run(eng):
    return Run(eng)


@pytest.mark.parametrize("i", range(len(PC.NAMES)), ids=PC.NAMES)
def test_open_crafted_ciphertext(run, i):
    cs, p = run.cases[i], run.plain[i]
    assert p is not None  # the oracle accepts the model's tag
    st, _, out, crc = run.open[i]
    assert st == E.OK
    assert out == p
    assert crc == orc.checksum(np.frombuffer(p, np.uint8), hw=True)
    # one flipped tag bit: refused, nothing released
    st, _, out, crc = run.open_bad[i]
    assert st == E.ETAG
    assert out == bytes(cs.n) and crc == bytes(len(crc))


@pytest.mark.parametrize("i", range(len(PC.NAMES)), ids=PC.NAMES)
def test_seal_reaches_crafted_ciphertext(run, i):
    cs, p = run.cases[i], run.plain[i]
    st, tag, out, crc = run.seal[i]
    assert st == E.OK
    assert out == cs.c
    assert tag == cs.tag
    assert crc == orc.checksum(np.frombuffer(p, np.uint8), hw=True)


def test_host_memory_pass(eng, run):
    """The same list through MEM_HOST (the staged host path plans its own batches)."""
    for i, (cs, p) in enumerate(zip(run.cases, run.plain)):
        c, tag, crc = eng.seal(CP, cs.key, cs.nonce, np.frombuffer(p, np.uint8), crc=True)
        assert (c, tag) == (cs.c, cs.tag), cs.name
        assert crc == orc.checksum(np.frombuffer(p, np.uint8), hw=True), cs.name
        assert eng.open(CP, cs.key, cs.nonce, cs.c, cs.tag, crc=crc) == p, cs.name
        assert eng.open(CP, cs.key, cs.nonce, cs.c, flip(cs.tag, i)) is None, cs.name
