"""CPU pin of slice compaction's host side: the layouts of the six records,
header against binding; the exports; jfsx_compact_plan against the independent
planner and the byte model of tests/compact_model.py; its calling convention;
every argument error of jfsx_gather_batch and jfsx_compact_objects with a
context and a key that would fault if they were used; and
juicefs_amd/csrc/jfsx_gather.h, the host build of what gather_pages_k runs on
the GPU, emulated lane by lane against numpy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import compact_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "compact_host.cpp")
I, U32, U64, P = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
PLAN_ARGS = [U32, I, ctypes.POINTER(E.jfsx_slice), I, ctypes.POINTER(E.jfsx_csrc), ctypes.POINTER(I), I,
             ctypes.POINTER(E.jfsx_cpage), ctypes.POINTER(U64), ctypes.POINTER(I), I, ctypes.POINTER(E.jfsx_piece),
             ctypes.POINTER(I)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compact") / "compact_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.compact_plan_host.argtypes = PLAN_ARGS
    L.compact_plan_host.restype = I
    L.gather_host.argtypes = [ctypes.POINTER(E.jfsx_gsrc), I, ctypes.POINTER(E.jfsx_gdst),
                              ctypes.POINTER(E.jfsx_piece), ctypes.POINTER(U64)]
    L.gather_host.restype = U64
    return L


# -- layout and exports ------------------------------------------------------
def test_record_layouts_header_vs_binding(host):
    out = (U64 * 64)()
    k = host.compact_layout(out, 64)
    want = []
    for cls in (E.jfsx_slice, E.jfsx_csrc, E.jfsx_cpage, E.jfsx_piece, E.jfsx_gsrc, E.jfsx_gdst):
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert k == len(want) and list(out[:k]) == want
    assert [ctypes.sizeof(c) for c in (E.jfsx_slice, E.jfsx_csrc, E.jfsx_cpage, E.jfsx_piece, E.jfsx_gsrc,
                                       E.jfsx_gdst)] == [24, 16, 16, 24, 16, 24]
    assert [f for f, _ in E.jfsx_slice._fields_] == ["id", "size", "off", "len", "reserved"]
    assert [f for f, _ in E.jfsx_piece._fields_] == ["src", "reserved", "src_off", "len"]
    c = (I * 5)()
    assert host.compact_constants(c) == 5
    assert tuple(c) == (E.GATHER_TILE, 256, 16, E.ESRC, 9)
    assert E.ESRC == 9 and E.GATHER_TILE % (256 * 16) == 0


def test_library_exports_compaction():
    L = E.load_library()
    for name in ("jfsx_compact_plan", "jfsx_gather_batch", "jfsx_compact_objects"):
        assert name in E.EXPORTS and hasattr(L, name)
    assert L.jfsx_compact_objects.argtypes[6] == ctypes.POINTER(E.jfsx_oblk)
    assert L.jfsx_compact_objects.argtypes[9] == ctypes.POINTER(E.jfsx_soblk)
    assert L.jfsx_abi_version() == 9


# -- the planner against the model ---------------------------------------------
def _host_plan(host, block_size, slices):
    sl = (E.jfsx_slice * max(len(slices), 1))()
    for i, (sid, size, off, ln) in enumerate(slices):
        sl[i].id, sl[i].size, sl[i].off, sl[i].len = sid, size, off, ln
    ns, npg, npc = I(), I(), I()
    assert host.compact_plan_host(block_size, len(slices), sl, 0, None, ns, 0, None, None, npg, 0, None, npc) in (
        0, E.ENOMEM)
    srcs, pages = (E.jfsx_csrc * max(ns.value, 1))(), (E.jfsx_cpage * max(npg.value, 1))()
    plen, pieces = (U64 * max(npg.value, 1))(), (E.jfsx_piece * max(npc.value, 1))()
    assert host.compact_plan_host(block_size, len(slices), sl, ns.value, srcs, ns, npg.value, pages, plen, npg,
                                  npc.value, pieces, npc) == 0
    return ([(srcs[i].id, srcs[i].indx, srcs[i].bsize) for i in range(ns.value)],
            [(pages[j].piece_first, pages[j].piece_count, plen[j]) for j in range(npg.value)],
            [(pieces[k].src, pieces[k].src_off, pieces[k].len) for k in range(npc.value)])


def _check_plan(host, block_size, slices, data):
    want = CM.plan(block_size, slices)
    got = E.compact_plan(block_size, slices)
    assert got[0] == want[0], "sources"
    assert got[2] == want[2], "pieces"
    assert got[1] == want[1], "pages"
    assert _host_plan(host, block_size, slices) == got  # the header as g++ builds it
    # canonical form, restated: no piece crosses a block, and no two neighbours of a page continue each other
    for first, count, ln in got[1]:
        run = got[2][first:first + count]
        assert sum(n for _, _, n in run) == ln and 0 < ln <= block_size
        for (s0, o0, n0), (s1, o1, _) in zip(run, run[1:]):
            assert not (s0 == s1 and (s0 < 0 or o0 + n0 == o1))
        assert all(n > 0 and (s < 0 or o + n <= got[0][s][2]) for s, o, n in run)
    assert len(set(got[0])) == len(got[0])
    pages = CM.apply_plan(*got, CM.slice_blocks(data, block_size))
    assert pages == CM.compact_bytes(slices, data, block_size)
    return got


@pytest.mark.parametrize("block_size", [64, 100, 256])
@pytest.mark.parametrize("seed", range(6))
def test_plan_against_model_small_blocks(host, block_size, seed):
    rng = np.random.default_rng(0xC0DE + 97 * seed + block_size)
    slices, data = CM.seeded_slices(rng, block_size, 12)
    _check_plan(host, block_size, slices, data)


def test_plan_against_model_4mib_blocks(host):
    bs = 4 << 20
    rng = np.random.default_rng(0xC0DE4)
    data = {1: rng.integers(0, 256, bs + 1, dtype=np.uint8).tobytes(),
            2: rng.integers(0, 256, bs - 1, dtype=np.uint8).tobytes(),
            3: rng.integers(0, 256, 7, dtype=np.uint8).tobytes()}
    slices = [(0, 5, 0, 5), (1, bs + 1, 0, bs + 1), (2, bs - 1, bs // 2, bs // 2 - 1), (0, 9, 0, 9),
              (1, bs + 1, bs - 1, 2), (3, 7, 6, 1), (2, bs - 1, 0, 1), (0, 3, 0, 3)]
    srcs, pages, pieces = _check_plan(host, bs, slices, data)
    assert srcs == [(1, 0, bs), (1, 1, 1), (2, 0, bs - 1), (3, 0, 7)]  # one id in several records: each block once
    total = sum(ln for _, _, _, ln in slices)
    assert total == bs + bs // 2 + 21 and [n for _, _, n in pages] == [bs, total - bs]


def test_plan_edges(host):
    # an all-hole list: one merged piece per page
    got = _check_plan(host, 64, [(0, 10, 0, 10), (0, 100, 0, 100), (0, 1, 0, 1)], {})
    assert got == ([], [(0, 1, 64), (1, 1, 47)], [(-1, 0, 64), (-1, 0, 47)])
    # a single-byte slice, and nothing at all
    assert _check_plan(host, 64, [(7, 1, 0, 1)], {7: b"x"}) == ([(7, 0, 1)], [(0, 1, 1)], [(0, 0, 1)])
    assert E.compact_plan(64, []) == ([], [], [])
    # two records of one id that continue each other merge into one piece; a gap keeps them apart
    d = {5: bytes(range(200))}
    assert _check_plan(host, 256, [(5, 200, 0, 50), (5, 200, 50, 30)], d)[2] == [(0, 0, 80)]
    assert _check_plan(host, 256, [(5, 200, 0, 50), (5, 200, 51, 30)], d)[2] == [(0, 0, 50), (0, 51, 30)]
    # ranges that end on, one before and one behind a block boundary
    d = {9: bytes(range(256)) * 2}
    for end in (127, 128, 129, 255, 256, 257):
        srcs, pages, pieces = _check_plan(host, 128, [(9, 512, 3, end - 3)], d)
        assert len(srcs) == -(-end // 128)


def test_reference_testcompact_shape(host):
    """compact_test.go:28-87: 100 slices of 100 + 100 i bytes with ids 0..99 at
    block 256 KiB; id 0 is a hole."""
    bs = 256 << 10
    slices = [(i, 100 + 100 * i, 0, 100 + 100 * i) for i in range(100)]
    rng = np.random.default_rng(0x7E57)
    data = {i: rng.integers(0, 256, 100 + 100 * i, dtype=np.uint8).tobytes() for i in range(1, 100)}
    srcs, pages, pieces = _check_plan(host, bs, slices, data)
    assert len(srcs) == 99 and len(pieces) == 101
    assert pages == [(0, 72, 262144), (72, 29, 242856)]
    assert pieces[0] == (-1, 0, 100)
    assert [p for p in pieces if p[0] == 70] == [(70, 0, 6544), (70, 6544, 656)]
    assert srcs[70] == (71, 0, 7200)


# -- the planner's calling convention ---------------------------------------------
def _slices(*recs):
    sl = (E.jfsx_slice * max(len(recs), 1))()
    for i, r in enumerate(recs):
        sl[i].id, sl[i].size, sl[i].off, sl[i].len = r[:4]
        sl[i].reserved = r[4] if len(r) > 4 else 0
    return sl


def test_plan_two_call_sizing_and_errors():
    L = E.load_library()
    sl = _slices((0, 10, 0, 10), (4, 300, 20, 200), (4, 300, 250, 50))
    ns, npg, npc = I(-1), I(-1), I(-1)
    assert L.jfsx_compact_plan(128, 3, sl, 0, None, ns, 0, None, None, npg, 0, None, npc) == E.ENOMEM
    assert (ns.value, npg.value, npc.value) == (3, 3, 7)
    srcs, pages = (E.jfsx_csrc * 4)(), (E.jfsx_cpage * 4)()
    plen, pieces = (U64 * 4)(), (E.jfsx_piece * 8)()
    for a in (srcs, pages, plen, pieces):
        ctypes.memset(a, 0xA5, ctypes.sizeof(a))
    before = [bytes(a) for a in (srcs, pages, plen, pieces)]
    # every capacity one short in turn: ENOMEM, the counts written, the arrays untouched
    for caps in ((2, 3, 7), (3, 2, 7), (3, 3, 6)):
        ns.value = npg.value = npc.value = -1
        assert L.jfsx_compact_plan(128, 3, sl, caps[0], srcs, ns, caps[1], pages, plen, npg, caps[2], pieces,
                                   npc) == E.ENOMEM
        assert (ns.value, npg.value, npc.value) == (3, 3, 7)
        assert [bytes(a) for a in (srcs, pages, plen, pieces)] == before
    assert L.jfsx_compact_plan(128, 3, sl, 4, srcs, ns, 4, pages, plen, npg, 8, pieces, npc) == 0
    assert [(pages[j].piece_first, pages[j].piece_count, pages[j].src_bad, pages[j].reserved, plen[j])
            for j in range(3)] == [(0, 3, -1, 0, 128), (3, 3, -1, 0, 128), (6, 1, -1, 0, 4)]
    assert bytes(pieces)[7 * 24:] == before[3][7 * 24:] and bytes(srcs)[3 * 16:] == before[0][3 * 16:]
    assert all(pieces[k].reserved == 0 for k in range(7))
    # JFSX_EINVAL
    args = (4, srcs, ns, 4, pages, plen, npg, 8, pieces, npc)
    assert L.jfsx_compact_plan(0, 3, sl, *args) == E.EINVAL  # block_size == 0
    assert L.jfsx_compact_plan(128, -1, sl, *args) == E.EINVAL
    assert L.jfsx_compact_plan(128, 1, None, *args) == E.EINVAL
    assert L.jfsx_compact_plan(128, 1, _slices((4, 300, 0, 10, 1)), *args) == E.EINVAL  # reserved
    assert L.jfsx_compact_plan(128, 1, _slices((4, 300, 0, 0)), *args) == E.EINVAL  # len == 0
    assert L.jfsx_compact_plan(128, 1, _slices((0, 0, 0, 0)), *args) == E.EINVAL  # len == 0 of a hole
    assert L.jfsx_compact_plan(128, 1, _slices((4, 300, 101, 200)), *args) == E.EINVAL  # off + len > size
    assert L.jfsx_compact_plan(128, 1, _slices((4, 300, 0xFFFFFFFF, 2)), *args) == E.EINVAL  # ... without wrapping
    assert L.jfsx_compact_plan(128, 1, _slices((4, 300, 100, 200)), *args) == 0
    assert L.jfsx_compact_plan(128, 1, _slices((0, 5, 100, 200)), *args) == 0  # a hole has no size to exceed
    big = _slices((0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 1))
    assert L.jfsx_compact_plan(1 << 30, 2, big, *args) == E.EINVAL  # a total beyond 2^32 - 1
    assert L.jfsx_compact_plan(1 << 30, 1, big, *args) == 0 and (npg.value, npc.value) == (4, 4)
    # a plan no int can count (2^32 - 1 pages of one byte): JFSX_ENOMEM before anything is built, not an exception
    ns.value = npg.value = npc.value = -1
    assert L.jfsx_compact_plan(1, 1, big, *args) == E.ENOMEM
    assert (ns.value, npg.value, npc.value) == (-1, -1, -1)
    assert L.jfsx_compact_plan(1, 1, _slices((0, 0, 0, 0xFFFFFFFF, 1)), *args) == E.EINVAL  # an argument error first
    assert L.jfsx_compact_plan(2, 1, _slices((0, 0, 0, 0xFFFFFFFF)), *args) == E.ENOMEM  # 2^31 pages
    assert L.jfsx_compact_plan(128, 3, sl, 4, srcs, None, 4, pages, plen, npg, 8, pieces, npc) == E.EINVAL
    assert L.jfsx_compact_plan(128, 3, sl, 4, None, ns, 4, pages, plen, npg, 8, pieces, npc) == E.EINVAL
    assert L.jfsx_compact_plan(128, 3, sl, -1, srcs, ns, 4, pages, plen, npg, 8, pieces, npc) == E.EINVAL
    assert L.jfsx_compact_plan(128, 0, None, 0, None, ns, 0, None, None, npg, 0, None, npc) == 0
    assert (ns.value, npg.value, npc.value) == (0, 0, 0)


# -- argument errors of the two device calls --------------------------------------
def _abuf(n, fill):
    buf = np.full(n + 32, fill, np.uint8)
    return buf, (buf.ctypes.data + 15) & ~15


def test_gather_argument_errors_touch_no_context():
    L = E.load_library()
    fake = P(16)
    sbuf, sp = _abuf(256, 0x5A)
    dbuf, dp = _abuf(256, 0xA5)

    def recs(pieces, dst=(64,), src=(100, 50), first=0, count=None):
        gs = (E.jfsx_gsrc * 2)()
        gs[0].data, gs[0].len, gs[1].data, gs[1].len = sp, src[0], sp + 112, src[1]
        gd = (E.jfsx_gdst * max(len(dst), 1))()
        at = 0
        for j, n in enumerate(dst):
            gd[j].data, gd[j].len = dp + at, n
            at += (n + 15) & ~15
        gd[0].piece_first, gd[0].piece_count = first, len(pieces) if count is None else count
        pa, n = E.make_pieces(pieces)
        return gs, gd, pa, n

    call = L.jfsx_gather_batch
    ok = [(0, 3, 60), (-1, 0, 4)]
    gs, gd, pa, n = recs(ok)
    for mem in (E.MEM_HOST, E.MEM_DEVICE):
        assert call(None, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        assert call(fake, 2, gs, 0, None, n, pa, mem) == 0  # nothing to write: the context is not touched
    assert call(fake, 2, gs, 1, gd, n, pa, 2) == E.EINVAL and call(fake, 2, gs, 1, gd, n, pa, -1) == E.EINVAL
    assert call(fake, -1, gs, 1, gd, n, pa, E.MEM_HOST) == E.EINVAL
    assert call(fake, 2, None, 1, gd, n, pa, E.MEM_HOST) == E.EINVAL
    assert call(fake, 2, gs, 1, None, n, pa, E.MEM_HOST) == E.EINVAL
    assert call(fake, 2, gs, 1, gd, n, None, E.MEM_HOST) == E.EINVAL
    bad = [
        [(2, 0, 60), (-1, 0, 4)],  # a piece index outside [-1, n_src)
        [(-2, 0, 60), (-1, 0, 4)],
        [(0, 41, 60), (-1, 0, 4)],  # src_off + len > src.len
        [(1, 0, 51), (-1, 0, 13)],
        [(0, (1 << 64) - 1, 2), (-1, 0, 62)],  # ... without wrapping
        [(0, 3, 60), (-1, 0, 0), (-1, 0, 4)],  # a piece of len 0
        [(0, 3, 60), (-1, 0, 3)],  # the lengths do not sum to dst.len
        [(0, 3, 60), (-1, 0, 5)],
    ]
    for mem in (E.MEM_HOST, E.MEM_DEVICE):
        for pieces in bad:
            gs, gd, pa, n = recs(pieces)
            assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL, pieces
        gs, gd, pa, n = recs(ok)
        pa[1].reserved = 1
        assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        gs, gd, pa, n = recs(ok, first=1)  # a piece range outside n_piece
        assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        gs, gd, pa, n = recs(ok, first=0xFFFFFFFF, count=2)
        assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        gs, gd, pa, n = recs(ok)
        gd[0].data = None  # bytes to write and nowhere to write them
        assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        gs, gd, pa, n = recs(ok)
        gs[0].data = None
        assert call(fake, 2, gs, 1, gd, n, pa, mem) == E.EINVAL
        gs, gd, pa, n = recs(ok, dst=(64, 0))  # an empty destination may not name pieces
        gd[1].piece_first, gd[1].piece_count = 1, 1
        assert call(fake, 2, gs, 2, gd, n, pa, mem) == E.EINVAL
    # device memory: alignment and overlap
    D = E.MEM_DEVICE
    gs, gd, pa, n = recs(ok)
    gd[0].data = dp + 1
    assert call(fake, 2, gs, 1, gd, n, pa, D) == E.EINVAL
    gs, gd, pa, n = recs(ok)
    gs[1].data = sp + 120
    assert call(fake, 2, gs, 1, gd, n, pa, D) == E.EINVAL
    for where in (sp, sp + 96, sp + 160 - 16):  # a destination over a source: head, tail of src 0, tail of src 1
        gs, gd, pa, n = recs(ok)
        gd[0].data = where
        assert call(fake, 2, gs, 1, gd, n, pa, D) == E.EINVAL, where - sp
    gs, gd, pa, n = recs([(0, 3, 60), (-1, 0, 4), (-1, 0, 32)], dst=(64, 32), count=2)
    gd[1].piece_first, gd[1].piece_count = 2, 1
    gd[1].data = dp + 48  # two destinations that overlap
    assert call(fake, 2, gs, 2, gd, n, pa, D) == E.EINVAL
    gd[1].data = dp  # ... or coincide
    assert call(fake, 2, gs, 2, gd, n, pa, D) == E.EINVAL
    assert (sbuf == 0x5A).all() and (dbuf == 0xA5).all()


def test_compact_objects_argument_errors_touch_no_context():
    """A context and a key that would fault if they were dereferenced:
    JFSX_EINVAL, the records and the buffers unchanged."""
    L = E.load_library()
    fake, fkey = P(16), P(32)
    img = np.full(128, 0x5A, np.uint8)
    hdr = np.frombuffer(bytes([1, 0, 12]) + bytes(268), np.uint8).copy()
    obj = np.full(1024, 0xA5, np.uint8)
    crc = np.full(8, 0xA5, np.uint8)

    def recs(pieces=((0, 0, 100), (-1, 0, 20)), codec=E.CODEC_LZ4, src_len=80, length=100, page=120):
        oarr, _ = E.Engine.make_oblocks([{"hdr": hdr.ctypes.data, "hdr_len": 271, "tag": bytes(16),
                                          "src": img.ctypes.data, "src_len": src_len, "dst": None, "len": length}])
        sarr, _ = E.Engine.make_soblocks([{"key": bytes(32), "nonce": bytes(12), "seed": bytes(32), "src": None,
                                           "len": page, "obj": obj.ctypes.data,
                                           "obj_cap": E.object_bound(codec, page), "crc": crc.ctypes.data}])
        oarr[0].status, oarr[0].out_len, oarr[0].obj_crc, oarr[0].key_len = 77, 78, 79, 80
        sarr[0].status, sarr[0].out_len, sarr[0].img_len, sarr[0].obj_crc = 81, 82, 83, 84
        cp = (E.jfsx_cpage * 1)()
        cp[0].piece_first, cp[0].piece_count, cp[0].src_bad = 0, len(pieces), 55
        pa, n = E.make_pieces(pieces)
        return oarr, sarr, cp, pa, n

    def untouched(oarr, sarr, cp):
        o, s = oarr[0], sarr[0]
        return ((o.status, o.out_len, o.obj_crc, o.key_len, s.status, s.out_len, s.img_len, s.obj_crc, cp[0].src_bad)
                == (77, 78, 79, 80, 81, 82, 83, 84, 55))

    A, Z, G, e = E.AES256GCM, E.CODEC_LZ4, E.CRC_GEN, 65537
    call = L.jfsx_compact_objects

    def run(ctx=fake, key=fkey, ee=e, algo=A, codec=Z, sm=E.CRC_CT, dm=G | E.CRC_CT, edit=None, **kw):
        oarr, sarr, cp, pa, n = recs(codec=codec, **kw)
        n_src = n_dst = 1
        if edit:
            edit(oarr, sarr, cp, pa)
        rc = call(ctx, key, ee, algo, codec, n_src, oarr, sm, n_dst, sarr, cp, dm, n, pa)
        assert untouched(oarr, sarr, cp)
        return rc

    assert run(ctx=None) == E.EINVAL
    # batch-level
    assert run(key=None) == E.EINVAL
    for ee in (0, 1, 1 << 31):
        assert run(ee=ee) == E.EINVAL
    for algo in (E.CIPHER_NONE, 2, -2):  # a volume without a cipher is out of scope
        assert run(algo=algo) == E.EINVAL
    for codec in (3, -1):
        oarr, sarr, cp, pa, n = recs()
        assert call(fake, fkey, e, A, codec, 1, oarr, 0, 1, sarr, cp, G, n, pa) == E.EINVAL
    for sm in (E.CRC_GEN, E.CRC_VERIFY, E.CRC_GEN | E.CRC_CT, 16, -1):  # 0 or CT
        assert run(sm=sm) == E.EINVAL, sm
    for dm in (E.CRC_VERIFY, E.CRC_VERIFY | E.CRC_CT, E.CRC_GEN | E.CRC_VERIFY, 16, -1):  # nothing to verify against
        assert run(dm=dm) == E.EINVAL, dm
    oarr, sarr, cp, pa, n = recs()
    assert call(fake, fkey, e, A, Z, -1, oarr, 0, 1, sarr, cp, G, n, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, oarr, 0, -1, sarr, cp, G, n, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, oarr, 0, 1, sarr, cp, G, -1, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, None, 0, 1, sarr, cp, G, n, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, oarr, 0, 1, None, cp, G, n, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, oarr, 0, 1, sarr, None, G, n, pa) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, oarr, 0, 1, sarr, cp, G, n, None) == E.EINVAL
    assert untouched(oarr, sarr, cp)

    def setter(which, field, value):
        def f(oarr, sarr, cp, pa):
            setattr({"o": oarr, "s": sarr, "c": cp, "p": pa}[which][0], field, value)
        return f

    # the NULL rules, and the two calls' per-block rules for host memory
    for which, field, value, kw in (
            ("o", "dst", obj.ctypes.data, {}), ("o", "crc", crc.ctypes.data, {}),  # the page stays on the device
            ("s", "src", img.ctypes.data, {}),  # the page is assembled
            ("o", "reserved", 1, {}), ("o", "src", None, {}), ("o", "hdr", None, {}),
            ("o", "src_len", 0x7E000001, {}), ("o", "len", 1 << 32, {}),
            ("o", "src_len", 99, {"codec": E.CODEC_NONE}),  # without a codec the image is the page
            ("s", "reserved", 1, {}), ("s", "reserved2", 1, {}), ("s", "obj", None, {}), ("s", "crc", None, {}),
            ("s", "obj_cap", E.object_bound(Z, 120) - 1, {}),
            ("s", "obj_cap", 286 + 120, {"codec": E.CODEC_NONE, "src_len": 100}),
            ("c", "reserved", 1, {}), ("c", "piece_first", 1, {}), ("c", "piece_count", 3, {}),
            ("p", "reserved", 1, {}), ("p", "src", 1, {}), ("p", "src", -2, {}), ("p", "src_off", 1, {}),
            ("p", "len", 101, {}), ("p", "len", 99, {}), ("p", "len", 0, {})):
        assert run(edit=setter(which, field, value), **kw) == E.EINVAL, (which, field, value)
    assert run(pieces=((0, 0, 100), (-1, 0, 21))) == E.EINVAL  # the pieces do not sum to the page
    assert run(pieces=((0, 1, 100), (-1, 0, 20))) == E.EINVAL  # a piece beyond its source's page length
    # n_dst == 0 is a no-op that touches nothing
    oarr, sarr, cp, pa, n = recs()
    assert call(fake, fkey, e, A, Z, 1, oarr, E.CRC_CT, 0, None, None, G, 0, None) == 0
    assert untouched(oarr, sarr, cp)
    assert (img == 0x5A).all() and (obj == 0xA5).all() and (crc == 0xA5).all()


# -- the gather, emulated lane by lane ----------------------------------------------
class HostGather:
    """Sources and destinations in 16-byte aligned host memory with whole chunks
    readable around every source and 0xA5 guards around every destination."""

    def __init__(self, sources, pages, pieces):
        self.sources, self.pages, self.pieces = [bytes(s) for s in sources], list(pages), list(pieces)
        self.keep, self.gs = [], (E.jfsx_gsrc * max(len(sources), 1))()
        for i, s in enumerate(self.sources):
            buf, p = _abuf(len(s) + 32, 0xEE)
            o = p - buf.ctypes.data + 16
            buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
            self.keep.append(buf)
            self.gs[i].data, self.gs[i].len = p + 16, len(s)
        self.gd, self.dst = (E.jfsx_gdst * max(len(pages), 1))(), []
        for j, (first, count, n) in enumerate(self.pages):
            buf, p = _abuf(n + 64, 0xA5)
            o = p - buf.ctypes.data + 32
            self.dst.append((buf, o))
            self.gd[j].data, self.gd[j].len = (p + 32 if n else None), n
            self.gd[j].piece_first, self.gd[j].piece_count = first, count
        self.pa, self.n_piece = E.make_pieces(self.pieces)

    def want(self):
        out = []
        for first, count, n in self.pages:
            parts = [np.zeros(ln, np.uint8) if s < 0 else np.frombuffer(self.sources[s], np.uint8)[o:o + ln]
                     for s, o, ln in self.pieces[first:first + count]]
            out.append(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
        return out

    def check(self):
        for (buf, o), w in zip(self.dst, self.want()):
            assert np.array_equal(buf[o:o + w.size], w)
            assert (buf[:o] == 0xA5).all() and (buf[o + w.size:] == 0xA5).all()


def test_gather_emulated_alignment_matrix(host):
    rng = np.random.default_rng(0x6A7)
    sources = [rng.integers(1, 256, 1024 + 16 + 4097, dtype=np.uint8).tobytes() for _ in range(2)]
    pages, pieces = CM.alignment_matrix(CM.MATRIX_LENGTHS, len(sources[0]), 3 * E.GATHER_TILE + 5)
    assert CM.matrix_seen(pages, pieces) == CM.matrix_full(CM.MATRIX_LENGTHS) and len(pages) > 20
    g = HostGather(sources, pages, pieces)
    loads = U64()
    assert host.gather_host(g.gs, len(pages), g.gd, g.pa, loads) == 0
    g.check()
    total = sum(n for _, _, n in pages)
    assert 0 < loads.value <= 2 * -(-total // 16)  # at most two aligned loads per destination chunk


def test_gather_emulated_shapes(host):
    rng = np.random.default_rng(0x6A8)
    T = E.GATHER_TILE
    src = [rng.integers(1, 256, 4 * T + 16, dtype=np.uint8).tobytes(),
           rng.integers(1, 256, 100, dtype=np.uint8).tobytes()]
    cases = []
    # single-piece pages at src_off 0 and 1; an empty page among them
    plens = [0, 1, 13, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 5]
    pcs, pgs = [], []
    for n in plens:
        for so in (0, 1):
            pgs.append((len(pcs), 1 if n else 0, n))
            if n:
                pcs.append((0, so, n))
    cases.append((pgs, pcs))
    # piece boundaries at k T - 1, k T, k T + 1 in a page of three tiles + 5
    cuts = sorted({k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {0, 3 * T + 5})
    pcs = [(-1 if i % 3 == 2 else 0, 17 * i, b - a) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    cases.append(([(0, len(pcs), 3 * T + 5)], pcs))
    # 4096 one-byte pieces cycling through two sources and a hole; an all-hole page; one range read twice
    pcs = [((k % 3) - 1, k % 97, 1) for k in range(4096)]
    pcs += [(-1, 0, 1000), (-1, 0, 3097)]
    pcs += [(0, 5, 3000), (0, 5, 3000)]
    cases.append(([(0, 4096, 4096), (4096, 2, 4097), (4098, 2, 6000)], pcs))
    for pages, pieces in cases:
        g = HostGather(src, pages, pieces)
        assert host.gather_host(g.gs, len(pages), g.gd, g.pa, None) == 0
        g.check()


def test_sanitized_standalone_run(tmp_path):
    """The harness with its own main under AddressSanitizer and UBSan, as a
    stand-alone program: an alignment matrix, the reference's TestCompact shape
    and the planner's argument errors against memcpy."""
    exe = str(tmp_path / "compact_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "compact_host ok" in r.stdout, (r.stdout, r.stderr)
