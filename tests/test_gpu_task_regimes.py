"""The AEAD and CRC kernels at every task size the planner picks.

The main kernels work on tasks that plan_batch (jfsx_api.cpp) cuts from the
blocks, and the task size follows the batch's total bytes alone: GCM 64 KiB ..
4 MiB, ChaCha 128 KiB .. 1 MiB, crc_segments_k 512 KiB .. 4 MiB.  The task size
decides how a task is split among the waves -- which segments two waves share,
which waves are empty on a short last task, which exponents lift the GHASH /
Poly1305 partials -- so a kernel can be right at one size and wrong at another.

Filler plus probes: a batch of unchecked filler blocks (synthetic data, sealed
in place on one 2 GiB device buffer) brings the total into the band of the
wanted task size, and a few small probe blocks in the same batch are compared
bit for bit with the oracle.  engine.debug_plan asserts the task size each
batch really gets, so a change of planner constants fails here instead of
silently losing the coverage.

Every comparison is exact: ciphertext, tag, CRC arrays, statuses, first
failing segment and its got / expect.
"""
import functools

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
SEG = E.SEG
GCM, CP, CRC = E.PLAN_GCM, E.PLAN_CHACHA, E.PLAN_CRC
ALGO = {GCM: E.AES256GCM, CP: E.CHACHA20P1305}
ORC = {GCM: orc.AES256GCM, CP: orc.CHACHA20P1305}
NAME = {GCM: "gcm", CP: "chacha", CRC: "crc"}
UNIT = {GCM: 64 * KIB, CP: 128 * KIB, CRC: 512 * KIB}
WANT = {GCM: 512, CP: 2048, CRC: 512}  # tasks a small batch is cut into

GCM_K = [3, 4, 6, 7, 9, 20, 31, 47, 64]  # x 64 KiB: k mod 8 in {3, 4, 6, 7, 1, 4, 7, 7, 0}
CP_K = [3, 5, 8]                         # x 128 KiB
CRC_T = [3 * 512 * KIB, 4 * MIB]
SWEEP = [(GCM, k) for k in GCM_K] + [(CP, k) for k in CP_K]
# one middle and the largest task size per algorithm, for the other CRC modes
MODES_AT = [(GCM, 20), (GCM, 64), (CP, 5), (CP, 8)]
# the crc_segments_k task of those batches' CRC_BOTH ciphertext pass: their totals / 512, in 512 KiB steps
CT_TASK = {(GCM, 20): 1536 * KIB, (GCM, 64): 4 * MIB, (CP, 5): 2560 * KIB, (CP, 8): 4 * MIB}
EDGES_AT =[(GCM, 3), (GCM, 64), (CP, 3), (CP, 8)]
FAILS_AT = [(GCM, 47), (CP, 8)]
SHAPES = ["many", "one"]

FILL_CAP = 2048 * MIB
PROBE_CAP = 160 * MIB
CRC_CAP = 1 * MIB
FSEED = 0x52454749  # filler data and keys


def _id(v):
    return "%s-%dK" % (NAME[v[0]], v[1] * UNIT[v[0]] // KIB)


def nseg(n):
    return max(1, -(-n // SEG))


class Gpu:
    """One engine with the module's device buffers."""

    def __init__(self, kind):
        self.kind = kind
        self.eng = E.Engine(0, E.CTX_BITSLICE if kind == "bitslice" else 0)
        self.fill = self.eng.alloc(FILL_CAP)
        self.psrc = self.eng.alloc(PROBE_CAP)
        self.pdst = self.eng.alloc(PROBE_CAP)
        self.crc = [self.eng.alloc(CRC_CAP), self.eng.alloc(CRC_CAP)]

    def close(self):
        for b in [self.fill, self.psrc, self.pdst] + self.crc:
            b.free()
        self.eng.close()


@pytest.fixture(scope="module", params=["ttable", "bitslice"])
def g(request):
    """Both AES-GCM keystream kernels (the ChaCha and CRC paths ignore the flag)."""
    gpu = Gpu(request.param)
    yield gpu
    gpu.close()


# ---------------------------------------------------------------------------
# probes and their oracle values


def probe_lens(T):
    tails = [1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 32767, 32768, 32769, 36869, T // 2 + 3,
             T - 32769, T - 2049, T - 17, T - 16, T - 1]
    seen, lens = set(), []
    for t in tails:
        if 0 < t < T and t not in seen:
            seen.add(t)
            lens.append((len(lens) % 3) * T + t)
    return lens + [T, 2 * T]


class Probe:
    """One block with its oracle values: C, tag, checksum(P), checksum(C)."""

    def __init__(self, kind, key, nonce, p):
        self.key, self.nonce, self.p, self.n = key, nonce, p, p.size
        self.c, self.tag = orc.seal(ORC[kind], key, nonce, p, fast=True)
        self.crc_p = orc.checksum(p, hw=True)
        self.crc_c = orc.checksum(np.frombuffer(self.c, np.uint8), hw=True)


@functools.lru_cache(maxsize=2)
def sweep_probes(kind, T):
    """The probe set of task size T: computed once, shared by the filler shapes and the modes."""
    seed = 0x5052 + 131 * kind + T // KIB
    return [Probe(kind, *orc.gen_key(seed, i), orc.gen_block(seed, i, n)) for i, n in enumerate(probe_lens(T))]


def edge_targets(n):
    """Ciphertexts no random stream produces (name, bytes)."""
    zero = np.zeros(n, np.uint8)
    last = zero.copy()
    last[(n - 1) // 16 * 16:] = np.arange(1, n - (n - 1) // 16 * 16 + 1, dtype=np.uint8)
    first = zero.copy()
    first[0] = 0x80
    return [("zero", zero), ("ff", np.full(n, 0xFF, np.uint8)), ("last16", last), ("first", first)]


@functools.lru_cache(maxsize=2)
def edge_probes(kind, T):
    """Plaintexts whose ciphertext is a chosen byte string: the keystream is
    XORed, so Seal of the target is that plaintext.  All-zero C: every GHASH
    partial is zero and the Poly1305 blocks are only the 2^128 bit; all-0xFF
    C: the largest Poly1305 limbs."""
    out = []
    for n in (T + 36869, 32768):
        for j, (name, target) in enumerate(edge_targets(n)):
            key, nonce = orc.gen_key(0x4544 + kind, 16 * (n % 251) + j)
            p = np.frombuffer(orc.seal(ORC[kind], key, nonce, target, fast=True)[0], np.uint8)
            pr = Probe(kind, key, nonce, p)
            assert pr.c == target.tobytes(), (name, n)  # the construction itself
            out.append(pr)
    return out


# ---------------------------------------------------------------------------
# batches


def filler_lens(kind, T, shape, probe_total):
    """Filler that puts filler + probes in the middle of the band of totals that
    yields task size T: total / WANT within (T - unit, T]."""
    fill = (T - UNIT[kind] // 2) * WANT[kind] - probe_total
    assert 2 * T <= fill <= FILL_CAP
    # many: 2 tasks per block, so every block of the batch has <= 4 tasks (the
    # 64-thread GCM finalize); one: thousands of slots on one ragged block
    return [2 * T] * (fill // (2 * T)) if shape == "many" else [fill - 7]


def gen_filler(g, T, flens):
    """Synthetic blocks 0.. of stream FSEED at a stride of 2T over g.fill."""
    if len(flens) == 1:
        g.eng.gen_synthetic(g.fill, flens[0], FSEED, 0)
    else:
        g.eng.gen_synthetic_batch(g.fill, 2 * T, flens, FSEED, 0)


class Batch:
    """Filler blocks over g.fill (in place) and probes at 256-byte aligned
    offsets of g.psrc / g.pdst; per block a CRC array with room for the two
    halves of CRC_BOTH."""

    def __init__(self, g, kind, T, shape, probes):
        self.g, self.kind, self.T, self.probes = g, kind, T, probes
        self.flens = filler_lens(kind, T, shape, sum(p.n for p in probes))
        self.nf = len(self.flens)
        self.lens = self.flens + [p.n for p in probes]
        tb, _, _ = E.debug_plan(kind, self.lens)
        assert tb == T, "planner: wanted %d-byte %s tasks, got %d" % (T, NAME[kind], tb)
        self.foff = [2 * T * i for i in range(self.nf)]
        self.poff, off = [], 0
        for p in probes:
            self.poff.append(off)
            off += (p.n + 255) & ~255
        self.pbytes = off
        assert off <= PROBE_CAP
        self.coff, off = [], 0
        for n in self.lens:
            self.coff.append(off)
            off += 8 * nseg(n)
        self.cbytes = off
        assert off <= CRC_CAP
        self.fkeys = [orc.gen_key(FSEED, i) for i in range(self.nf)]

    def gen_filler(self):
        gen_filler(self.g, self.T, self.flens)

    def upload(self, buf, datas):
        host = np.zeros(self.pbytes, np.uint8)
        for off, d in zip(self.poff, datas):
            host[off:off + len(d)] = np.frombuffer(d, np.uint8) if isinstance(d, bytes) else d
        buf.upload(host)

    def upload_crcs(self, cbuf, crcs, fill=0):
        """Probe CRC arrays into cbuf (the filler's part of it is left alone)."""
        lo = self.coff[self.nf]
        host = np.full(self.cbytes - lo, fill, np.uint8)
        for i, c in enumerate(crcs):
            o = self.coff[self.nf + i] - lo
            host[o:o + len(c)] = np.frombuffer(bytes(c), np.uint8)
        cbuf.upload(host, offset=lo)

    def blocks(self, cbuf, src, dst, tags=None, only_filler=False):
        """jfsx_blk array: filler in place, probe i from src to dst (device buffers)."""
        specs = []
        for i in range(self.nf):
            k, nc = self.fkeys[i]
            p = self.g.fill.ptr + self.foff[i]
            specs.append({"key": k, "nonce": nc, "src": p, "dst": p, "len": self.flens[i],
                          "crc": cbuf.ptr + self.coff[i], "tag": tags[i] if tags else None})
        for i, pr in enumerate([] if only_filler else self.probes):
            specs.append({"key": pr.key, "nonce": pr.nonce, "src": src.ptr + self.poff[i],
                          "dst": dst.ptr + self.poff[i], "len": pr.n, "crc": cbuf.ptr + self.coff[self.nf + i],
                          "tag": tags[self.nf + i] if tags else None})
        return self.g.eng.make_blocks(specs)

    def tags_of(self, arr):
        return [bytes(arr[i].tag) for i in range(len(self.lens))]

    def where(self, i, what):
        return "%s %s T=%d len=%d: %s" % (self.g.kind, NAME[self.kind], self.T, self.probes[i].n, what)

    def check_bytes(self, buf, wants, what):
        """Probe i's bytes in buf equal wants[i]; a mismatch names the first differing segment."""
        host = buf.download(self.pbytes)
        for i, w in enumerate(wants):
            got = host[self.poff[i]:self.poff[i] + len(w)]
            w = np.frombuffer(w, np.uint8) if isinstance(w, bytes) else w
            if not np.array_equal(got, w):
                at = int(np.nonzero(got != w)[0][0])
                raise AssertionError(self.where(i, "%s differs from byte %d (segment %d)" % (what, at, at // SEG)))

    def check_crcs(self, cbuf, wants, what, half=0):
        """Probe i's CRC array (half 1: the ciphertext half of CRC_BOTH) equals wants[i]."""
        host = cbuf.download(self.cbytes)
        for i, w in enumerate(wants):
            o = self.coff[self.nf + i] + half * 4 * nseg(self.probes[i].n)
            got = host[o:o + len(w)].tobytes()
            if got != w:
                bad = [s for s in range(len(w) // 4) if got[4 * s:4 * s + 4] != w[4 * s:4 * s + 4]]
                raise AssertionError(self.where(i, "%s CRC differs in segments %s" % (what, bad[:8])))

    def check_status(self, arr, what, tags=None):
        for i in range(len(self.lens)):
            b = arr[i]
            assert (b.status, b.crc_bad_seg) == (E.OK, -1), "%s %s T=%d block %d (len %d): %s status %d seg %d" % (
                self.g.kind, NAME[self.kind], self.T, i, self.lens[i], what, b.status, b.crc_bad_seg)
        if tags is not None:
            for i, pr in enumerate(self.probes):
                assert bytes(arr[self.nf + i].tag) == tags[i], self.where(i, what + " tag")


# ---------------------------------------------------------------------------
# the main sweep: Seal + CRC_GEN against the oracle, Open + CRC_VERIFY in place


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("at", SWEEP, ids=_id)
def test_seal_gen_open_verify_at_task_size(g, at, shape):
    kind, T = at[0], at[1] * UNIT[at[0]]
    probes = sweep_probes(kind, T)
    bt = Batch(g, kind, T, shape, probes)
    bt.gen_filler()
    bt.upload(g.psrc, [p.p for p in probes])
    arr, n = bt.blocks(g.crc[0], g.psrc, g.pdst)
    g.eng.seal_batch(ALGO[kind], arr, n, E.CRC_GEN, E.MEM_DEVICE)
    bt.check_status(arr, "seal", [p.tag for p in probes])
    bt.check_bytes(g.pdst, [p.c for p in probes], "ciphertext")
    bt.check_crcs(g.crc[0], [p.crc_p for p in probes], "seal GEN")
    if kind == GCM and shape == "one" and T == GCM_K[0] * UNIT[GCM]:
        # the one place a very long block's lifts meet an independent reference
        # (a Seal / Open round trip alone would agree with itself)
        ftags, fcrcs, _ = orc.expect_batch(ORC[kind], 1, bt.flens, FSEED, 0, 4 * nseg(bt.flens[0]))
        assert bytes(arr[0].tag) == ftags[0].tobytes(), "filler tag (%d bytes)" % bt.flens[0]
        got = g.crc[0].download(4 * nseg(bt.flens[0]), offset=bt.coff[0])
        assert np.array_equal(got, fcrcs[0]), "filler CRCs, segments %s" % np.nonzero(
            (got != fcrcs[0]).reshape(-1, 4).any(axis=1))[0][:8]
    # Open of the whole batch in place, verifying the CRCs Seal wrote
    oarr, n = bt.blocks(g.crc[0], g.pdst, g.pdst, bt.tags_of(arr))
    g.eng.open_batch(ALGO[kind], oarr, n, E.CRC_VERIFY, E.MEM_DEVICE)
    bt.check_status(oarr, "open VERIFY")
    bt.check_bytes(g.pdst, [p.p for p in probes], "opened plaintext")


# ---------------------------------------------------------------------------
# the other CRC modes on the same probes


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("at", MODES_AT, ids=_id)
def test_crc_modes_at_task_size(g, at, shape):
    """Seal CRC_VERIFY, Seal / Open CRC_GEN | CRC_CT, Open CRC_GEN and Seal /
    Open CRC_GEN | CRC_BOTH (whose ciphertext pass is a crc_segments_k launch
    with its own task size), the filler riding along in place."""
    kind, T = at[0], at[1] * UNIT[at[0]]
    algo = ALGO[kind]
    probes = sweep_probes(kind, T)
    bt = Batch(g, kind, T, shape, probes)
    # the ciphertext pass of BOTH is planned from the same lengths
    assert E.debug_plan(CRC, bt.lens)[0] == CT_TASK[at]
    bt.gen_filler()
    bt.upload(g.psrc, [p.p for p in probes])
    A, B = g.crc
    ps, cs, tags = [p.p for p in probes], [p.c for p in probes], [p.tag for p in probes]
    crc_p, crc_c = [p.crc_p for p in probes], [p.crc_c for p in probes]

    # Seal GEN | BOTH: checksum(P) || checksum(C) per block, into A
    arr, n = bt.blocks(A, g.psrc, g.pdst)
    g.eng.seal_batch(algo, arr, n, E.CRC_GEN | E.CRC_BOTH, E.MEM_DEVICE)
    bt.check_status(arr, "seal BOTH", tags)
    bt.check_bytes(g.pdst, cs, "seal BOTH ciphertext")
    bt.check_crcs(A, crc_p, "seal BOTH plaintext")
    bt.check_crcs(A, crc_c, "seal BOTH ciphertext", half=1)
    ftags = bt.tags_of(arr)
    # Open GEN | BOTH in place, into B: the same arrays again, the filler's too
    oarr, n = bt.blocks(B, g.pdst, g.pdst, ftags)
    g.eng.open_batch(algo, oarr, n, E.CRC_GEN | E.CRC_BOTH, E.MEM_DEVICE)
    bt.check_status(oarr, "open BOTH")
    bt.check_bytes(g.pdst, ps, "open BOTH plaintext")
    bt.check_crcs(B, crc_p, "open BOTH plaintext")
    bt.check_crcs(B, crc_c, "open BOTH ciphertext", half=1)
    assert np.array_equal(A.download(bt.cbytes), B.download(bt.cbytes)), "filler CRCs of seal and open BOTH differ"

    # Seal VERIFY against the plaintext CRCs in A (the first half of each array)
    arr, n = bt.blocks(A, g.psrc, g.pdst)
    g.eng.seal_batch(algo, arr, n, E.CRC_VERIFY, E.MEM_DEVICE)
    bt.check_status(arr, "seal VERIFY", tags)
    assert bt.tags_of(arr) == ftags
    bt.check_bytes(g.pdst, cs, "seal VERIFY ciphertext")
    bt.check_crcs(A, crc_p, "seal VERIFY (expected array rewritten)")
    # Open GEN | CT in place, into B: the CRCs of the ciphertext read
    bt.upload_crcs(B, [], fill=0xEE)
    oarr, n = bt.blocks(B, g.pdst, g.pdst, ftags)
    g.eng.open_batch(algo, oarr, n, E.CRC_GEN | E.CRC_CT, E.MEM_DEVICE)
    bt.check_status(oarr, "open CT")
    bt.check_bytes(g.pdst, ps, "open CT plaintext")
    bt.check_crcs(B, crc_c, "open CT")
    # Seal GEN | CT: the CRCs of the ciphertext written
    bt.upload_crcs(B, [], fill=0xEE)
    arr, n = bt.blocks(B, g.psrc, g.pdst)
    g.eng.seal_batch(algo, arr, n, E.CRC_GEN | E.CRC_CT, E.MEM_DEVICE)
    bt.check_status(arr, "seal CT", tags)
    bt.check_bytes(g.pdst, cs, "seal CT ciphertext")
    bt.check_crcs(B, crc_c, "seal CT")
    # Open GEN: checksum() of the plaintext
    bt.upload_crcs(B, [], fill=0xEE)
    oarr, n = bt.blocks(B, g.pdst, g.pdst, ftags)
    g.eng.open_batch(algo, oarr, n, E.CRC_GEN, E.MEM_DEVICE)
    bt.check_status(oarr, "open GEN")
    bt.check_bytes(g.pdst, ps, "open GEN plaintext")
    bt.check_crcs(B, crc_p, "open GEN")


# ---------------------------------------------------------------------------
# failure reporting at a large task size


def shared_segment(kind, T):
    """A segment of a task that meets the boundary between waves 0 and 1.  The
    T-table GCM kernel gives each of 16 waves T / 16 KiB rows of 1 KiB, and
    a segment is 32 rows: when the run is no whole number of segments, the
    segment holding row T / 16 KiB is shared by both waves.  ChaCha gives
    each of 4 waves whole segments: the first segment of wave 1."""
    rows = T // (16 * KIB) if kind == GCM else T // (4 * KIB)
    return rows // 32


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("at", FAILS_AT, ids=_id)
def test_failures_reported_at_large_task_size(g, at, shape):
    kind, T = at[0], at[1] * UNIT[at[0]]
    algo = ALGO[kind]
    seed = 0x4641 + kind
    lens = [2 * T + 36869, T + 5, 2 * T + 36869, 2 * T + 36869, T + 17]
    probes = [Probe(kind, *orc.gen_key(seed, i), orc.gen_block(seed, i, n)) for i, n in enumerate(lens)]
    bt = Batch(g, kind, T, shape, probes)
    sh = T // SEG + shared_segment(kind, T)  # in the second task
    if kind == GCM:
        assert (T // (16 * KIB)) % 32, "pick a task size whose wave runs end inside a segment"
    last = nseg(lens[0]) - 1
    assert lens[0] - last * SEG < SEG  # a short last segment
    crcs = [bytearray(p.crc_p) for p in probes]
    tags = [p.tag for p in probes]
    for s in (1, sh, last):          # probe 0: first task, shared in the second task, short last
        crcs[0][4 * s + 1] ^= 0x21
    crcs[1][2] ^= 0x04               # probe 1: wrong CRC and wrong tag
    tags[1] = bytes([tags[1][0] ^ 1]) + tags[1][1:]
    crcs[2][4 * last + 3] ^= 0x80    # probe 2: only the short last segment
    crcs[3][4 * sh] ^= 0x01          # probe 3: only the shared segment
    # the filler sealed on the GPU (in place), then one Open of everything
    bt.gen_filler()
    farr, n = bt.blocks(g.crc[0], g.psrc, g.pdst, only_filler=True)
    g.eng.seal_batch(algo, farr, n, E.CRC_GEN, E.MEM_DEVICE)
    bt.upload(g.pdst, [p.c for p in probes])
    bt.upload(g.psrc, [np.full(p.n, 0xA5, np.uint8) for p in probes])
    bt.upload_crcs(g.crc[0], crcs)
    arr, n = bt.blocks(g.crc[0], g.pdst, g.psrc, [bytes(farr[i].tag) for i in range(bt.nf)] + tags)
    g.eng.open_batch(algo, arr, n, E.CRC_VERIFY, E.MEM_DEVICE)
    for i in range(bt.nf):
        assert (arr[i].status, arr[i].crc_bad_seg) == (E.OK, -1), "filler %d" % i
    out = g.psrc.download(bt.pbytes)

    def report(i):
        b = arr[bt.nf + i]
        return b.status, b.crc_bad_seg, b.crc_got, b.crc_expect

    def want(i, s):
        return (E.ECRC, s, orc.crc32c(probes[i].p[s * SEG:(s + 1) * SEG].tobytes()),
                int.from_bytes(crcs[i][4 * s:4 * s + 4], "big"))

    assert report(0) == want(0, 1), bt.where(0, "lowest of three bad segments")
    assert arr[bt.nf + 1].status == E.ETAG, bt.where(1, "bad tag and bad CRC")
    assert not out[bt.poff[1]:bt.poff[1] + lens[1]].any(), bt.where(1, "output not zeroed")
    assert report(2) == want(2, last), bt.where(2, "short last segment")
    assert report(3) == want(3, sh), bt.where(3, "shared segment %d" % sh)
    assert report(4)[:2] == (E.OK, -1), bt.where(4, "good block")
    assert out[bt.poff[4]:bt.poff[4] + lens[4]].tobytes() == probes[4].p.tobytes()


# ---------------------------------------------------------------------------
# ciphertexts the synthetic stream never produces


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("at", EDGES_AT, ids=_id)
def test_crafted_ciphertexts_at_task_size(g, at, shape):
    kind, T = at[0], at[1] * UNIT[at[0]]
    probes = edge_probes(kind, T)
    bt = Batch(g, kind, T, shape, probes)
    bt.gen_filler()
    bt.upload(g.psrc, [p.p for p in probes])
    arr, n = bt.blocks(g.crc[0], g.psrc, g.pdst)
    g.eng.seal_batch(ALGO[kind], arr, n, E.CRC_GEN, E.MEM_DEVICE)
    bt.check_status(arr, "seal", [p.tag for p in probes])
    bt.check_bytes(g.pdst, [p.c for p in probes], "ciphertext")
    bt.check_crcs(g.crc[0], [p.crc_p for p in probes], "seal GEN")
    oarr, n = bt.blocks(g.crc[0], g.pdst, g.pdst, bt.tags_of(arr))
    g.eng.open_batch(ALGO[kind], oarr, n, E.CRC_VERIFY, E.MEM_DEVICE)
    bt.check_status(oarr, "open VERIFY")
    bt.check_bytes(g.pdst, [p.p for p in probes], "opened plaintext")


# ---------------------------------------------------------------------------
# crc_segments_k alone


@functools.lru_cache(maxsize=2)
def crc_probes(T):
    ps = [orc.gen_block(0x4352 + T // KIB, i, n) for i, n in enumerate(probe_lens(T))]
    return [(p, orc.checksum(p, hw=True)) for p in ps]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("T", CRC_T, ids=lambda t: "crc-%dK" % (t // KIB))
def test_crc_only_at_task_size(g, T, shape):
    probes = crc_probes(T)
    flens = filler_lens(CRC, T, shape, sum(p.size for p, _ in probes))
    lens = flens + [p.size for p, _ in probes]
    assert E.debug_plan(CRC, lens)[0] == T
    gen_filler(g, T, flens)
    poff, off = [], 0
    for p, _ in probes:
        poff.append(off)
        off += (p.size + 255) & ~255
    assert off <= PROBE_CAP
    host = np.zeros(off, np.uint8)
    for o, (p, _) in zip(poff, probes):
        host[o:o + p.size] = p
    g.psrc.upload(host)
    arr = (E.jfsx_range * len(lens))()
    coff, co = [], 0
    for i, n in enumerate(lens):
        nf = len(flens)
        arr[i].data = g.fill.ptr + 2 * T * i if i < nf else g.psrc.ptr + poff[i - nf]
        arr[i].len, arr[i].crc = n, g.crc[0].ptr + co
        coff.append(co)
        co += 4 * nseg(n)
    assert co <= CRC_CAP
    g.eng.crc32c_segments(arr, len(lens), E.CRC_GEN, E.MEM_DEVICE)
    got = g.crc[0].download(co)
    for i, (p, want) in enumerate(probes):
        o = coff[len(flens) + i]
        have = got[o:o + len(want)].tobytes()
        assert have == want, "%s crc T=%d len=%d: segments %s" % (
            g.kind, T, p.size, [s for s in range(len(want) // 4) if have[4 * s:4 * s + 4] != want[4 * s:4 * s + 4]][:8])
    g.eng.crc32c_segments(arr, len(lens), E.CRC_VERIFY, E.MEM_DEVICE)
    for i in range(len(lens)):
        assert (arr[i].status, arr[i].bad_seg) == (E.OK, -1), (i, lens[i])


# ---------------------------------------------------------------------------
# the regimes this file stands for


def test_every_named_task_size_is_planned():
    """Every (kind, task size) the sweep names is the size debug_plan gives its
    batch, for both filler shapes (host only: the lengths alone decide)."""
    got = set()
    for kind, sizes in ((GCM, [k * UNIT[GCM] for k in GCM_K]), (CP, [k * UNIT[CP] for k in CP_K]), (CRC, CRC_T)):
        for T in sizes:
            plens = probe_lens(T)
            for shape in SHAPES:
                tb, nslots, tasks = E.debug_plan(kind, filler_lens(kind, T, shape, sum(plens)) + plens)
                assert tb == T, (NAME[kind], T, shape, tb)
                got.add((NAME[kind], tb // KIB))
    assert got == ({("gcm", 64 * k) for k in (3, 4, 6, 7, 9, 20, 31, 47, 64)} |
                   {("chacha", 128 * k) for k in (3, 5, 8)} | {("crc", 1536), ("crc", 4096)})
