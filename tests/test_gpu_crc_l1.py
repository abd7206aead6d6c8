"""The GCM kernel's fused CRC32C with part of its slice lookups through the
vector L1 (JFSX_CTX_CRC_L1) against the all-LDS path (JFSX_CTX_CRC_LDS): one
process, one engine per path, the same small batch through every CRC mode.

The L1 path lives in the two-row loop of the 16-wave T-table kernel and only
where the CRC covers the side the kernel loads: Seal with the plaintext CRC
(GEN and VERIFY) and Open with JFSX_CRC_CT.  Seal with JFSX_CRC_CT, Open with
the plaintext CRC and the whole bitsliced context must not notice the flag.
Every ciphertext, tag, CRC array, status and bad-segment report is compared
with the oracle's and between the two engines.

Lengths: 1, 15, 16, 1023, 1024 never reach the row loop; 32 KiB gives every
wave exactly one two-row iteration; 33 KiB and 34 KiB - 1 leave an odd row to
the single-row loop; 64 KiB and 64 KiB + 17 have segments two waves share;
96 KiB + 2049, 1 MiB - 1, 4 MiB and 4 MiB - 32769 are cut into several tasks.
Three copies of each, so the persistent queue hands a workgroup several tasks.
"""
import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
SEG = E.SEG
LENS = [1, 15, 16, 1023, 1024, 32 * KIB, 33 * KIB, 34 * KIB - 1, 64 * KIB, 64 * KIB + 17, 96 * KIB + 2049, MIB - 1,
        4 * MIB, 4 * MIB - 32769]
COPIES = 3
SEED = 0x4C31
PATHS = (("l1", E.CTX_CRC_L1), ("lds", E.CTX_CRC_LDS))


def nseg(n):
    return max(1, -(-n // SEG))


class Ref:
    """The batch and its oracle values, computed once for all engines."""

    def __init__(self):
        self.lens = [n for n in LENS for _ in range(COPIES)]
        self.n = len(self.lens)
        self.keys = [orc.gen_key(SEED, i) for i in range(self.n)]
        self.p = [orc.gen_block(SEED, i, n) for i, n in enumerate(self.lens)]
        self.c, self.tag, self.crc_p, self.crc_c = [], [], [], []
        for (key, nonce), p in zip(self.keys, self.p):
            c, tag = orc.seal(orc.AES256GCM, key, nonce, p, fast=True)
            self.c.append(np.frombuffer(c, np.uint8))
            self.tag.append(tag)
            self.crc_p.append(orc.checksum(p, hw=True))
            self.crc_c.append(orc.checksum(self.c[-1], hw=True))
        self.off, off = [], 0
        for n in self.lens:
            self.off.append(off)
            off += (n + 255) & ~255
        self.bytes = off
        self.coff, off = [], 0
        for n in self.lens:
            self.coff.append(off)
            off += 4 * nseg(n)
        self.cbytes = off
        # Seal VERIFY: one stored CRC is wrong, in a segment deep inside a
        # 4 MiB block (whole segments per wave run, found in the row loop)
        self.bad_blk = self.lens.index(4 * MIB) + 1
        self.bad_seg = 77

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
def ref():
    r = Ref()
    assert len(E.debug_plan(E.PLAN_GCM, r.lens)[2]) > 256, "more tasks than the device has compute units"
    return r


class Run:
    """Everything one engine computes for the batch, mode by mode."""

    def __init__(self, ref, flags):
        self.ref, self.out = ref, {}
        self.eng = E.Engine(0, flags)
        self.src, self.dst = self.eng.alloc(ref.bytes), self.eng.alloc(ref.bytes)
        self.crc = self.eng.alloc(ref.cbytes)
        try:
            self.run()
        finally:
            for b in (self.src, self.dst, self.crc):
                b.free()
            self.eng.close()

    def blocks(self, tags=None):
        r = self.ref
        return self.eng.make_blocks([
            {"key": r.keys[i][0], "nonce": r.keys[i][1], "src": self.src.ptr + r.off[i], "dst": self.dst.ptr + r.off[i],
             "len": r.lens[i], "crc": self.crc.ptr + r.coff[i], "tag": tags[i] if tags else None}
            for i in range(r.n)])

    def keep(self, mode, arr, data=True, crcs=True):
        r = self.ref
        self.out[mode] = {
            "report": [(arr[i].status, arr[i].crc_bad_seg, arr[i].crc_got, arr[i].crc_expect) for i in range(r.n)],
            "tags": [bytes(arr[i].tag) for i in range(r.n)],
            "data": self.dst.download(r.bytes) if data else None,
            "crcs": self.crc.download(r.cbytes) if crcs else None,
        }

    def run(self):
        r, gcm, dev = self.ref, E.AES256GCM, E.MEM_DEVICE
        stale = np.full(r.cbytes, 0xEE, np.uint8)
        # Seal: GEN, VERIFY (one wrong stored CRC), GEN | CT
        self.src.upload(r.pack(r.p))
        self.crc.upload(stale)
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_GEN, dev)
        self.keep("seal_gen", arr)
        crcs = [bytearray(c) for c in r.crc_p]
        crcs[r.bad_blk][4 * r.bad_seg + 2] ^= 0x10
        self.crc.upload(r.pack_crcs(crcs))
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_VERIFY, dev)
        self.keep("seal_verify", arr)
        self.crc.upload(stale)
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_GEN | E.CRC_CT, dev)
        self.keep("seal_ct", arr)
        # Open: GEN | CT, then VERIFY over the plaintext (the untouched path)
        self.src.upload(r.pack(r.c))
        self.crc.upload(stale)
        arr, n = self.blocks(r.tag)
        self.eng.open_batch(gcm, arr, n, E.CRC_GEN | E.CRC_CT, dev)
        self.keep("open_ct", arr)
        self.crc.upload(r.pack_crcs(r.crc_p))
        arr, n = self.blocks(r.tag)
        self.eng.open_batch(gcm, arr, n, E.CRC_VERIFY, dev)
        self.keep("open_verify", arr)


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

    for mode, data, crcs in (("seal_gen", c, crc_p), ("seal_ct", c, crc_c), ("open_ct", p, crc_c)):
        o = out[mode]
        assert [x[:2] for x in o["report"]] == ok, "%s %s status" % (what, mode)
        assert o["tags"] == r.tag, "%s %s tags" % (what, mode)
        same(o["data"], data, mode + " output", "segment", r.off)
        same(o["crcs"], crcs, mode + " CRC array", "CRC", r.coff)
    o = out["seal_verify"]
    want_bad = (E.ECRC, r.bad_seg,
                orc.crc32c(r.p[r.bad_blk][r.bad_seg * SEG:(r.bad_seg + 1) * SEG].tobytes()),
                int.from_bytes(r.crc_p[r.bad_blk][4 * r.bad_seg:4 * r.bad_seg + 4], "big") ^ 0x1000)
    for i in range(r.n):
        if i == r.bad_blk:
            assert o["report"][i] == want_bad, "%s seal_verify: the wrong stored CRC of block %d" % (what, i)
        else:
            assert o["report"][i][:2] == (E.OK, -1), "%s seal_verify: block %d (len %d)" % (what, i, r.lens[i])
    assert o["tags"] == r.tag, what + " seal_verify tags"
    same(o["data"], c, "seal_verify output", "segment", r.off)
    o = out["open_verify"]
    assert [x[:2] for x in o["report"]] == ok, what + " open_verify status"
    same(o["data"], p, "open_verify output", "segment", r.off)


@pytest.mark.parametrize("kind", ["ttable", "bitslice"])
def test_crc_l1_and_lds_paths_agree_with_oracle(ref, kind):
    base = E.CTX_BITSLICE if kind == "bitslice" else 0
    outs = {}
    for name, flag in PATHS:
        outs[name] = Run(ref, base | flag).out
        check_against_oracle(ref, outs[name], "%s/%s" % (kind, name))
    a, b = outs["l1"], outs["lds"]
    for mode in a:
        assert a[mode]["report"] == b[mode]["report"], "%s %s: reports differ between the paths" % (kind, mode)
        assert a[mode]["tags"] == b[mode]["tags"], "%s %s: tags differ between the paths" % (kind, mode)
        for k in ("data", "crcs"):
            assert np.array_equal(a[mode][k], b[mode][k]), "%s %s: %s differ between the paths" % (kind, mode, k)


def test_crc_path_flags_exclude_each_other():
    with pytest.raises(E.EngineError):
        E.Engine(0, E.CTX_CRC_L1 | E.CTX_CRC_LDS)
