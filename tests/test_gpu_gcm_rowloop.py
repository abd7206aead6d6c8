"""The two-row loop of the 16-wave AES-GCM kernel against the oracle.

The loop takes rounds 1-2 of a row's AES from a per-task table P[256] (indexed
by the counter's low byte) and, where the CRC covers the loaded side, keeps
the lane CRCs in B form (already shifted to the lane's next piece; composed
tables, tests/test_crc_composed.py has the arithmetic).  Modes on that path:
Seal with the plaintext CRC, GEN and VERIFY (a clean image, and one with a
wrong stored CRC that must report its segment), and Open with JFSX_CRC_CT.
Each runs on the default context and on a JFSX_CTX_CRC_LDS context, whose CRC
keeps the all-LDS A-form path and serves as the control.  Tags, outputs, CRC
arrays and reports are compared with the oracle's.

Lengths, the smallest at which each piece can go wrong: 32 KiB (every wave
runs exactly one loop iteration and ends in B form), 64 KiB (a segment end
inside the loop), 96 KiB + 2 KiB (an odd pair count: a single row follows B
form), 64 KiB + 1000 and 1 MiB + 17 (a ragged tail after B form), 4 MiB,
31 KiB (no loop iteration at all), and one block that the plan cuts into
tasks, so a task starts at a nonzero offset and counter.  Every row above
4 KiB crosses a wrap of the counter's low byte.  A second batch of 600 blocks
of 32 KiB, each with a key of its own, makes every workgroup take several
tasks and rebuild P between them.  In a small batch the plan cuts a 4 MiB
block into 64 KiB tasks; the third batch adds 2 GiB of unchecked filler
blocks, so that the 4 MiB block is one task: whole segments per wave, and
each wave's 256 KiB run the counter's upper bits through a window refill.
"""
import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
SEG = E.SEG
SPLIT = 192 * KIB + 1000  # the plan cuts it: asserted in the fixture
LENS = [32 * KIB, 64 * KIB, 96 * KIB + 2 * KIB, 64 * KIB + 1000, MIB + 17, 4 * MIB, 31 * KIB, SPLIT]
PATHS = (("default", 0), ("lds", E.CTX_CRC_LDS))


def nseg(n):
    return max(1, -(-n // SEG))


class Ref:
    """A batch and its oracle values, computed once for all engines."""

    def __init__(self, seed, lens, bad_blk, bad_seg, fill=()):
        self.lens, self.n = lens, len(lens)
        self.fill = list(fill)  # unchecked blocks behind the n checked ones, in place in a buffer of their own
        self.bad_blk, self.bad_seg = bad_blk, bad_seg
        self.keys = [orc.gen_key(seed, i) for i in range(self.n)]
        self.p = [orc.gen_block(seed, i, n) for i, n in enumerate(lens)]
        self.c, self.tag, self.crc_p, self.crc_c = [], [], [], []
        for (key, nonce), p in zip(self.keys, self.p):
            c, tag = orc.seal(orc.AES256GCM, key, nonce, p, fast=True)
            self.c.append(np.frombuffer(c, np.uint8))
            self.tag.append(tag)
            self.crc_p.append(orc.checksum(p, hw=True))
            self.crc_c.append(orc.checksum(self.c[-1], hw=True))
        self.off, off = [], 0
        for n in lens:
            self.off.append(off)
            off += (n + 255) & ~255
        self.bytes = off
        self.coff, off = [], 0
        for n in lens:
            self.coff.append(off)
            off += 4 * nseg(n)
        self.cbytes = off

    def pack(self, datas):
        host = np.zeros(self.bytes, np.uint8)
        for off, d in zip(self.off, datas):
            host[off:off + len(d)] = d
        return host

    def pack_crcs(self, crcs):
        host = np.zeros(self.cbytes, np.uint8)
        for off, c in zip(self.coff, crcs):
            host[off:off + len(c)] = np.frombuffer(bytes(c), np.uint8)
        return host


@pytest.fixture(scope="module")
def ref_lens():
    r = Ref(0x5239, LENS, LENS.index(4 * MIB), 77)
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    blk = LENS.index(SPLIT)
    starts = sorted(c0 for b, c0, _ in tasks if b == blk)
    assert len(starts) > 1 and starts[0] == 0 and starts[1] > 0, "the plan cuts the block: a task starts inside it"
    return r


FILL = 8 * MIB


@pytest.fixture(scope="module")
def ref_big_task():
    r = Ref(0x5241, [4 * MIB], 0, 77, fill=[FILL] * 255)
    tb, _, tasks = E.debug_plan(E.PLAN_GCM, r.lens + r.fill)
    assert tb == 4 * MIB and (0, 0, 4 * MIB) in tasks, "the 4 MiB block is one task"
    return r


@pytest.fixture(scope="module")
def ref_keys():
    r = Ref(0x5240, [32 * KIB] * 600, 311, 0)
    assert len({k for k, _ in r.keys}) == r.n, "a key of its own per block"
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    assert len(tasks) == 600, "one task per block: more than twice the device's compute units"
    return r


class Run:
    """Everything one engine computes for a batch, mode by mode."""

    def __init__(self, ref, flags):
        self.ref, self.out = ref, {}
        self.eng = E.Engine(0, flags)
        self.src, self.dst = self.eng.alloc(ref.bytes), self.eng.alloc(ref.bytes)
        self.crc = self.eng.alloc(ref.cbytes)
        self.bufs = [self.src, self.dst, self.crc]
        try:
            if ref.fill:
                self.fsrc = self.eng.alloc(sum(ref.fill))
                self.bufs.append(self.fsrc)
                self.fcrc = self.eng.alloc(sum(4 * nseg(n) for n in ref.fill))
                self.bufs.append(self.fcrc)
            self.run()
        finally:
            for b in self.bufs:
                b.free()
            self.eng.close()

    def blocks(self, tags=None):
        r = self.ref
        blks = [
            {"key": r.keys[i][0], "nonce": r.keys[i][1], "src": self.src.ptr + r.off[i], "dst": self.dst.ptr + r.off[i],
             "len": r.lens[i], "crc": self.crc.ptr + r.coff[i], "tag": tags[i] if tags else None}
            for i in range(r.n)]
        off = coff = 0
        for n in r.fill:  # whatever the memory holds: their reports are not looked at
            blks.append({"key": r.keys[0][0], "nonce": r.keys[0][1], "src": self.fsrc.ptr + off,
                         "dst": self.fsrc.ptr + off, "len": n, "crc": self.fcrc.ptr + coff,
                         "tag": tags[0] if tags else None})
            off += n
            coff += 4 * nseg(n)
        return self.eng.make_blocks(blks)

    def keep(self, mode, arr, crcs=True):
        r = self.ref
        self.out[mode] = {
            "report": [(arr[i].status, arr[i].crc_bad_seg, arr[i].crc_got, arr[i].crc_expect) for i in range(r.n)],
            "tags": [bytes(arr[i].tag) for i in range(r.n)],
            "data": self.dst.download(r.bytes),
            "crcs": self.crc.download(r.cbytes) if crcs else None,
        }

    def run(self):
        r, gcm, dev = self.ref, E.AES256GCM, E.MEM_DEVICE
        stale = np.full(r.cbytes, 0xEE, np.uint8)
        self.src.upload(r.pack(r.p))
        self.crc.upload(stale)
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_GEN, dev)
        self.keep("seal_gen", arr)
        self.crc.upload(r.pack_crcs(r.crc_p))
        self.dst.upload(np.zeros(r.bytes, np.uint8))
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_VERIFY, dev)
        self.keep("seal_verify", arr, crcs=False)
        crcs = [bytearray(c) for c in r.crc_p]
        crcs[r.bad_blk][4 * r.bad_seg + 2] ^= 0x10
        self.crc.upload(r.pack_crcs(crcs))
        self.dst.upload(np.zeros(r.bytes, np.uint8))
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_VERIFY, dev)
        self.keep("seal_verify_bad", arr, crcs=False)
        self.src.upload(r.pack(r.c))
        self.crc.upload(stale)
        arr, n = self.blocks(r.tag)
        self.eng.open_batch(gcm, arr, n, E.CRC_GEN | E.CRC_CT, dev)
        self.keep("open_ct", arr)


def check_against_oracle(r, out, what):
    ok = [(E.OK, -1)] * r.n
    c, p = r.pack(r.c), r.pack(r.p)
    crc_p, crc_c = r.pack_crcs(r.crc_p), r.pack_crcs(r.crc_c)

    def same(got, want, where, unit, offs):
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            blk = max(i for i in range(r.n) if offs[i] <= at)
            raise AssertionError("%s %s: block %d (len %d) differs at %s %d" % (
                what, where, blk, r.lens[blk], unit, (at - offs[blk]) // (SEG if unit == "segment" else 4)))

    for mode, data, crcs in (("seal_gen", c, crc_p), ("seal_verify", c, None), ("open_ct", p, crc_c)):
        o = out[mode]
        assert [x[:2] for x in o["report"]] == ok, "%s %s status" % (what, mode)
        assert o["tags"] == r.tag, "%s %s tags" % (what, mode)
        same(o["data"], data, mode + " output", "segment", r.off)
        if crcs is not None:
            same(o["crcs"], crcs, mode + " CRC array", "CRC", r.coff)
    o = out["seal_verify_bad"]
    b, s = r.bad_blk, r.bad_seg
    want_bad = (E.ECRC, s, orc.crc32c(r.p[b][s * SEG:(s + 1) * SEG].tobytes()),
                int.from_bytes(r.crc_p[b][4 * s:4 * s + 4], "big") ^ 0x1000)
    for i in range(r.n):
        if i == b:
            assert o["report"][i] == want_bad, "%s seal_verify_bad: the wrong stored CRC of block %d" % (what, i)
        else:
            assert o["report"][i][:2] == (E.OK, -1), "%s seal_verify_bad: block %d (len %d)" % (what, i, r.lens[i])
    assert o["tags"] == r.tag, what + " seal_verify_bad tags"
    same(o["data"], c, "seal_verify_bad output", "segment", r.off)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_loop_lengths_match_oracle(ref_lens, path):
    check_against_oracle(ref_lens, Run(ref_lens, dict(PATHS)[path]).out, "lengths/" + path)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_loop_whole_4mib_task_match_oracle(ref_big_task, path):
    check_against_oracle(ref_big_task, Run(ref_big_task, dict(PATHS)[path]).out, "4 MiB task/" + path)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_loop_rebuilds_round_table_per_key(ref_keys, path):
    check_against_oracle(ref_keys, Run(ref_keys, dict(PATHS)[path]).out, "600 keys/" + path)
