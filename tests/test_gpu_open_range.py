"""jfsx_open_range_batch on the GPU: the tag checked over all of C, the window
alone decrypted and released.

Expected bytes come from the oracle alone: oracle.seal makes C and the tag,
oracle.open_ the plaintext, sliced by Go's rule (encrypt.go:246-253), restated
in window() below.  engine.debug_range_plan asserts that a shape reaches what
the test claims of it (which kernel reads a byte, how many tasks, which auth
task size), so a change of planner constants fails here instead of silently
losing the coverage.  Every comparison is exact.
"""
import functools

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
SEG = E.SEG
L = 384 * KIB + 1000
LENS = [0, 1, 15, 16, 17, 32768, 32769, L]
KINDS = [E.PLAN_GCM, E.PLAN_CHACHA]
ALGO = {E.PLAN_GCM: E.AES256GCM, E.PLAN_CHACHA: E.CHACHA20P1305}
ORC = {E.PLAN_GCM: orc.AES256GCM, E.PLAN_CHACHA: orc.CHACHA20P1305}
NAME = {E.PLAN_GCM: "gcm", E.PLAN_CHACHA: "chacha"}
MEMS = [E.MEM_DEVICE, E.MEM_HOST]
MEM_NAME = {E.MEM_DEVICE: "device", E.MEM_HOST: "host"}
CT = E.CRC_GEN | E.CRC_CT
SENT = 0xC3
PAD = 48  # bytes of dst_cap past n, and sentinel bytes in front of dst

# every edge the kernels have, as (off, limit) on a block of L bytes
WINDOWS = [
    (5, 1), (15, 2),                      # the 16 B AES block
    (63, 2),                              # the 64 B ChaCha block
    (1023, 2),                            # the 1 KiB GCM row
    (4095, 2),                            # the 4 KiB ChaCha row
    (32768 - 7, 14),                      # the segment
    (65535, 2), (131071, 2),              # both minimum task sizes
    (32768, 32768),                       # exactly one widened segment
    (65536 - 5, 32768 + 10),              # three widened segments
    (0, -1),                              # the whole block
    (L - 1, 1), (L - 17, -1), (L - 1000, 5000),  # the ragged tail (the last one is clamped)
    (L, 7), (L + 9, -1), (3, 0),          # n = 0
]


def window(length, off, limit):
    o = min(off, length)
    n = length - o if limit == -1 or limit > length - o else limit
    return o, n


def nseg(n):
    return max(1, -(-n // SEG))


class Block:
    """One block with its oracle values."""

    def __init__(self, kind, seed, i, n):
        self.kind, self.n = kind, n
        self.key, self.nonce = orc.gen_key(seed, i)
        p = orc.gen_block(seed, i, n)[:n]
        self.c, self.tag = orc.seal(ORC[kind], self.key, self.nonce, p, fast=True)
        self.p = orc.open_(ORC[kind], self.key, self.nonce, self.c, self.tag, fast=True) if n else b""
        assert self.p == p.tobytes()


@functools.lru_cache(maxsize=None)
def block(kind, n, i=0):
    return Block(kind, 0x52414E47 + kind, 1000 * i + n % 997, n)


class Item:
    """One record of a call: a block, its window, and what was done to C or the tag."""

    def __init__(self, blk, off, limit, flip_c=None, flip_tag=False):
        self.blk, self.off, self.limit = blk, off, limit
        self.o, self.n = window(blk.n, off, limit)
        c = bytearray(blk.c)
        if flip_c is not None:
            c[flip_c] ^= 0x10
        tag = bytearray(blk.tag)
        if flip_tag:
            tag[7] ^= 1
        self.c, self.tag = bytes(c), bytes(tag)
        self.bad = flip_c is not None or flip_tag
        self.want = bytes(self.n) if self.bad else blk.p[self.o:self.o + self.n]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def lay_out(items, odd):
    """Offsets of every record's C, dst and CRC array in three flat buffers;
    dst regions are PAD sentinel bytes, then dst_cap = n + PAD bytes."""
    so, do, co, s, d, c = [], [], [], 1 if odd else 0, 0, 0
    for it in items:
        so.append(s)
        s += (len(it.c) + 255) // 256 * 256 + (2 if odd else 0)
        do.append(d + PAD + (1 if odd else 0))
        d += (it.n + 2 * PAD + 255) // 256 * 256 + 256
        co.append(c)
        c += (4 * nseg(it.blk.n) + 15) // 16 * 16
    return so, do, co, max(s, 1), max(d, 1), max(c, 16)


def run_range(eng, kind, items, crc_mode, mem):
    """The ranged call on items; returns (rblk array, dst buffer, dst offsets,
    crc buffer, crc offsets) with the buffers as host arrays."""
    host = mem == E.MEM_HOST
    so, do, co, sb, db, cb = lay_out(items, host)
    src = np.zeros(sb, np.uint8)
    for it, o in zip(items, so):
        src[o:o + len(it.c)] = np.frombuffer(it.c, np.uint8)
    dst = np.full(db, SENT, np.uint8)
    crc = np.full(cb, SENT, np.uint8)
    if host:
        sp, dp, cp, bufs = src.ctypes.data, dst.ctypes.data, crc.ctypes.data, []
        assert all((sp + o) & 1 and (dp + o2) & 1 for o, o2 in zip(so, do)) or not items
    else:
        bufs = [eng.alloc(sb), eng.alloc(db), eng.alloc(cb)]
        for b, h in zip(bufs, (src, dst, crc)):
            b.upload(h)
        sp, dp, cp = (b.ptr for b in bufs)
    specs = [{"key": it.blk.key, "nonce": it.blk.nonce, "tag": it.tag, "src": sp + so[i] if it.blk.n else None,
              "len": it.blk.n, "off": it.off, "limit": it.limit, "dst": dp + do[i] if it.n else None,
              "dst_cap": it.n + PAD if it.n else 0, "crc": cp + co[i] if crc_mode else None}
             for i, it in enumerate(items)]
    arr, n = E.Engine.make_rblocks(specs)
    for i in range(n):
        arr[i].status, arr[i].out_len = 77, 78
    try:
        eng.open_range_batch(ALGO[kind], arr, n, crc_mode, mem)
        if not host:
            dst = bufs[1].download(db)
            crc = bufs[2].download(cb)
    finally:
        for b in bufs:
            b.free()
    return arr, dst, do, crc, co


def check(items, arr, dst, do):
    """Statuses, lengths, the windows' bytes, and the sentinel everywhere else."""
    keep = np.ones(dst.size, bool)
    for i, it in enumerate(items):
        what = (i, it.blk.n, it.off, it.limit, it.bad)
        assert arr[i].status == (E.ETAG if it.bad else E.OK), what
        assert arr[i].out_len == (0 if it.bad else it.n), what
        assert dst[do[i]:do[i] + it.n].tobytes() == it.want, what
        keep[do[i]:do[i] + it.n] = False
    assert (dst[keep] == SENT).all(), "bytes outside dst[0, n) were written"


def kernel_of(plan, blk, byte):
    """Which kernel's task covers `byte` of block blk (0 main, 1 auth), exactly one."""
    hit = [t for t in plan["tasks"] if t[0] == blk and t[2] <= byte < t[3]]
    assert len(hit) == 1
    return hit[0][1]


def plan_of(kind, items):
    return E.debug_range_plan(kind, [it.blk.n for it in items], [it.off for it in items], [it.limit for it in items])


@pytest.mark.parametrize("mem", MEMS, ids=MEM_NAME.get)
@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_windows_on_a_block_of_several_tasks(eng, kind, mem):
    b = block(kind, L)
    alone = plan_of(kind, [Item(b, 0, -1)])
    assert alone["blocks"][0]["n_main"] >= 2 and alone["blocks"][0]["n_auth"] == 0
    one, three = plan_of(kind, [Item(b, 32768, 32768)]), plan_of(kind, [Item(b, 65536 - 5, 32768 + 10)])
    assert (one["blocks"][0]["w0"], one["blocks"][0]["w1"]) == (32768, 65536)
    assert (three["blocks"][0]["w0"], three["blocks"][0]["w1"]) == (32768, 131072)
    for off, limit in WINDOWS:
        it = Item(b, off, limit)
        pl = plan_of(kind, [it])["blocks"][0]
        assert (pl["o"], pl["n"]) == (it.o, it.n)
        assert pl["n_main"] + pl["n_auth"] >= 2  # the block is cut into several tasks
        arr, dst, do, _, _ = run_range(eng, kind, [it], E.CRC_NONE, mem)
        check([it], arr, dst, do)


@pytest.mark.parametrize("mem", MEMS, ids=MEM_NAME.get)
@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_whole_block_equals_open_batch(eng, kind, mem):
    b = block(kind, L)
    it = Item(b, 0, -1)
    arr, dst, do, _, _ = run_range(eng, kind, [it], E.CRC_NONE, mem)
    src = np.frombuffer(b.c, np.uint8).copy()
    out = np.zeros(L, np.uint8)
    blks, n = E.Engine.make_blocks([{"key": b.key, "nonce": b.nonce, "tag": b.tag, "src": src.ctypes.data,
                                     "dst": out.ctypes.data, "len": L}])
    eng.open_batch(ALGO[kind], blks, n, E.CRC_NONE, E.MEM_HOST)
    assert blks[0].status == E.OK and arr[0].status == E.OK and arr[0].out_len == L
    assert dst[do[0]:do[0] + L].tobytes() == out.tobytes() == b.p


@pytest.mark.parametrize("mem", MEMS, ids=MEM_NAME.get)
@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_every_length(eng, kind, mem):
    items = []
    for n in LENS:
        b = block(kind, n)
        for off, limit in [(0, -1), (0, 0), (n // 2, 3), (n, 5), (n + 1, -1), (max(n, 1) - 1, 1)]:
            items.append(Item(b, off, limit))
    for it in items:  # one by one: the small-batch plan of each
        arr, dst, do, _, _ = run_range(eng, kind, [it], E.CRC_NONE, mem)
        check([it], arr, dst, do)
    arr, dst, do, _, _ = run_range(eng, kind, items, E.CRC_NONE, mem)
    check(items, arr, dst, do)


@pytest.mark.parametrize("mem", MEMS, ids=MEM_NAME.get)
@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_tag_failures(eng, kind, mem):
    b = block(kind, L)
    far = L - 500
    outside = Item(b, 5, 100, flip_c=far)       # what a keystream-only implementation passes wrongly
    assert kernel_of(plan_of(kind, [outside]), 0, far) == 1 and kernel_of(plan_of(kind, [outside]), 0, 5) == 0
    inside = Item(b, 40000, 300, flip_c=40100)
    assert kernel_of(plan_of(kind, [inside]), 0, 40100) == 0
    tag = Item(b, 70000, 9, flip_tag=True)
    empty = Item(b, 3, 0, flip_c=far)            # n = 0: the tag is still checked
    assert kernel_of(plan_of(kind, [empty]), 0, far) == 1
    for it in (outside, inside, tag, empty, Item(block(kind, 0), 0, -1, flip_tag=True)):
        arr, dst, do, _, _ = run_range(eng, kind, [it], E.CRC_NONE, mem)
        check([it], arr, dst, do)


def mixed_items(kind):
    items = []
    for i in range(64):
        n = LENS[i % len(LENS)]
        b = block(kind, n)
        off, limit = WINDOWS[(5 * i + i // 8) % len(WINDOWS)] if n == L else [(0, -1), (n // 3, 2), (n, 1)][i % 3]
        flip = {0: {}, 1: {"flip_tag": True}, 2: ({"flip_c": n - 1} if n else {"flip_tag": True})}[i % 3 if i % 2 else 0]
        items.append(Item(b, off, limit, **flip))
    return items


@pytest.mark.parametrize("crc_mode", [E.CRC_NONE, CT], ids=["none", "gen_ct"])
@pytest.mark.parametrize("mem", MEMS, ids=MEM_NAME.get)
@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_mixed_batch(eng, kind, mem, crc_mode):
    items = mixed_items(kind)
    assert any(it.bad for it in items) and any(not it.bad and it.n for it in items)
    m0 = eng.metrics()
    arr, dst, do, crc, co = run_range(eng, kind, items, crc_mode, mem)
    m1 = eng.metrics()
    check(items, arr, dst, do)
    assert m1["open_batches"] - m0["open_batches"] == 1
    assert m1["open_blocks"] - m0["open_blocks"] == len(items)
    assert m1["open_bytes"] - m0["open_bytes"] == sum(it.blk.n for it in items)  # the bytes authenticated
    assert m1["open_fail"] - m0["open_fail"] == sum(it.bad for it in items)
    if not crc_mode:
        assert (crc == SENT).all()
        return
    # the CRC bytes jfsx_open_batch returns in the same mode, on good tags and on bad ones
    srcs = [np.frombuffer(it.c, np.uint8).copy() if it.blk.n else np.zeros(1, np.uint8) for it in items]
    outs = [np.zeros(max(it.blk.n, 1), np.uint8) for it in items]
    ref = [np.full(4 * nseg(it.blk.n), SENT, np.uint8) for it in items]
    blks, n = E.Engine.make_blocks([{"key": it.blk.key, "nonce": it.blk.nonce, "tag": it.tag,
                                     "src": srcs[i].ctypes.data if it.blk.n else None, "dst": outs[i].ctypes.data,
                                     "len": it.blk.n, "crc": ref[i].ctypes.data} for i, it in enumerate(items)])
    eng.open_batch(ALGO[kind], blks, n, CT, E.MEM_HOST)
    keep = np.ones(crc.size, bool)
    for i, it in enumerate(items):
        assert blks[i].status == arr[i].status
        w = 4 * nseg(it.blk.n)
        assert crc[co[i]:co[i] + w].tobytes() == ref[i].tobytes(), i
        keep[co[i]:co[i] + w] = False
    assert (crc[keep] == SENT).all()


# ---------------------------------------------------------------------------
# few slots, high exponents, and every task size the auth planner can choose

AUTH_SIZES = {E.PLAN_GCM: [64 * KIB << k for k in range(5)], E.PLAN_CHACHA: [32 * KIB << k for k in range(6)]}
AUTH_WANT = {E.PLAN_GCM: 512, E.PLAN_CHACHA: 2048}
BIG = 2 * MIB


@pytest.mark.parametrize("kind,size", [(k, s) for k in KINDS for s in AUTH_SIZES[k]],
                         ids=lambda v: NAME.get(v, "") if v in NAME else "%dK" % (v // KIB))
def test_auth_task_sizes_and_few_slots(eng, kind, size):
    """A batch of 2 MiB blocks on one device buffer: four checked probes with
    windows in the first and in the last segment, and unchecked filler (more
    records of probe 0's C with an empty window, so they cost no memory and
    must verify too) that sizes the batch for the wanted auth task."""
    b = block(kind, BIG)
    far = MIB + 12345
    probes = [Item(b, 100, 50), Item(b, BIG - 77, -1), Item(b, 9, 3, flip_c=far), Item(b, BIG - 4000, 4000, flip_c=far)]
    top = size == AUTH_SIZES[kind][-1]
    nfill = 0 if size == AUTH_SIZES[kind][0] else int(1.25 * AUTH_WANT[kind] * size / BIG) + 1 - len(probes)
    items = probes + [Item(b, 3, 0)] * nfill
    pl = plan_of(kind, items)
    assert pl["auth_bytes"] == size, "planner: wanted %d-byte auth tasks, got %d" % (size, pl["auth_bytes"])
    assert kernel_of(pl, 2, far) == 1 and kernel_of(pl, 3, far) == 1
    # a slot's lift exponent is the 16-byte blocks behind its wave's run of the
    # task's rows (1 KiB GCM, 4 KiB ChaCha): 2^16 and above in every probe
    row, waves = (1024, 16) if kind == E.PLAN_GCM else (4096, 4)
    assert pl["auth_slots"] == waves
    for i in range(len(probes)):
        exps = []
        for blk, kern, c0, c1, _ in pl["tasks"]:
            if blk == i and kern == 1:
                nrows = -(-(c1 - c0) // row)
                ends = [min(c0 + (w + 1) * nrows // waves * row, c1) for w in range(waves)]
                exps += [BIG // 16 - -(-e // 16) for e in ends]
        assert max(exps) >= 1 << 16, (i, max(exps))
    if top:
        assert all(blk["n_main"] + blk["n_auth"] <= 3 for blk in pl["blocks"])
        assert all(blk["nslots"] <= 64 for blk in pl["blocks"])
    # every record reads the one device copy of C (probe 2 and 3 a tampered one)
    cbuf, tbuf, dbuf = eng.alloc(BIG), eng.alloc(BIG), eng.alloc(len(probes) * 8192)
    try:
        cbuf.upload(np.frombuffer(b.c, np.uint8))
        tbuf.upload(np.frombuffer(probes[2].c, np.uint8))
        dhost = np.full(len(probes) * 8192, SENT, np.uint8)
        dbuf.upload(dhost)
        specs = [{"key": b.key, "nonce": b.nonce, "tag": b.tag, "src": (tbuf if it.bad else cbuf).ptr, "len": BIG,
                  "off": it.off, "limit": it.limit, "dst": dbuf.ptr + 8192 * i + PAD if it.n else None,
                  "dst_cap": it.n + PAD if it.n else 0} for i, it in enumerate(items)]
        arr, n = E.Engine.make_rblocks(specs)
        eng.open_range_batch(ALGO[kind], arr, n, E.CRC_NONE, E.MEM_DEVICE)
        dst = dbuf.download(dhost.size)
    finally:
        for buf in (cbuf, tbuf, dbuf):
            buf.free()
    check(probes, arr, dst, [8192 * i + PAD for i in range(len(probes))])
    assert all(arr[i].status == E.OK and arr[i].out_len == 0 for i in range(len(probes), n))
