"""GPU tests of the one-call paths on host batches whose blocks lie partly in
page-locked and partly in pageable memory: jfsx_load_batch, jfsx_load_objects,
jfsx_store_batch, jfsx_store_objects, jfsx_gather_batch and
jfsx_open_range_batch with MEM_HOST.

A pageable block travels through the context's bounce buffer, a page-locked
one is copied by DMA where it lies; a batch of both takes the per-block branch
of the staging, one of pageable blocks alone (every numpy batch of the other
test modules) the packed branch.  Sources and destinations are carved out of
two arenas, one from Engine.alloc_pinned and one numpy array, both filled with
0xA5.  Every call is checked by comparing both arenas whole against what they
must hold afterwards: the sources as they were, every destination's expected
bytes, and 0xA5 everywhere else, which is the guard in front of and behind
every destination.

Every batch has five blocks:

  block  source    destination  content
  0      pinned    pageable     1 byte
  1      pageable  pageable     4096 bytes
  2      pinned    pinned       65536 + 17 bytes
  3      pageable  pinned       200000 bytes of text
  4      pinned    pinned       empty

in three layouts: "mixed" (the table), "pinned" (everything page-locked) and
"fail" (the table, block 2 made to fail: a flipped tag byte on the load paths
and the ranged Open, a wrong expected CRC word under CRC_VERIFY on the store
paths; without a cipher there is no tag, so jfsx_load_batch gets an image cut
short and jfsx_load_objects an image with a flipped bit under its old
checksum).  The failed block's page, in the page-locked arena, must be all
zero (load, range) or untouched (store), its neighbours as in "mixed".

Expected values come from the per-path modules' checkers (oracle, rsa_model,
zstd_lib, compact_model.gather_want), imported from them, never from the
engine."""
import ctypes
import functools

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import compact_model as CM
from tests import lz4_data
from tests import rsa_model as M
from tests import test_gpu_load as TL
from tests import test_gpu_load_objects as LO
from tests import test_gpu_open_range as TR
from tests import test_gpu_store as TS
from tests import test_gpu_store_objects as SO

pytestmark = pytest.mark.gpu

P, G = "pinned", "pageable"
MIXED = [(P, G), (G, G), (P, P), (G, P), (P, P)]
LAYOUTS = {"mixed": MIXED, "pinned": [(P, P)] * 5, "fail": MIXED}
LENS = [1, 4096, 65536 + 17, 200000, 0]
BAD = 2
GUARD = 64
FILL = 0xA5
GCM_LZ4 = ("gcm-lz4", E.AES256GCM, E.CODEC_LZ4)
NONE_ZSTD = ("none-zstd", E.CIPHER_NONE, E.CODEC_ZSTD)
GCM_NONE = ("gcm-none", E.AES256GCM, E.CODEC_NONE)
GCM_ZSTD = ("gcm-zstd", E.AES256GCM, E.CODEC_ZSTD)  # jfsx_store_objects always has a cipher
ids = lambda c: c[0] if isinstance(c, tuple) else c  # noqa: E731


@functools.lru_cache(maxsize=None)
def pages():
    kinds = ["random", "runs", "random", "text", "text"]
    return tuple(lz4_data.sample(k, n, seed=0x51A + i) for i, (k, n) in enumerate(zip(kinds, LENS)))


def nseg(n):
    return max(1, -(-n // E.SEG))


class Arenas:
    """The page-locked and the pageable arena, and what each must hold after the call."""

    def __init__(self, eng, size=2 << 20):
        self.eng, self.size = eng, size
        self.ptr = eng.alloc_pinned(size)
        self.view = {P: np.frombuffer((ctypes.c_uint8 * size).from_address(self.ptr), np.uint8),
                     G: np.empty(size, np.uint8)}
        self.base = {P: self.ptr, G: self.view[G].ctypes.data}
        self.reset()

    def reset(self):
        for v in self.view.values():
            v[:] = FILL
        self.top = {P: 0, G: 0}
        self.want = {k: np.full(self.size, FILL, np.uint8) for k in self.view}

    def room(self, kind, n):
        """n bytes at a 256-byte-aligned offset with GUARD bytes of 0xA5 on both sides -> (address, offset)."""
        off = (self.top[kind] + GUARD + 255) & ~255
        self.top[kind] = off + n + GUARD
        assert self.top[kind] + 4096 <= self.size
        return self.base[kind] + off, off

    def put(self, kind, data):
        """A source: its address; it must come back unchanged."""
        addr, off = self.room(kind, len(data))
        self.view[kind][off:off + len(data)] = np.frombuffer(bytes(data), np.uint8)
        self.expect(kind, off, data)
        return addr

    def expect(self, kind, off, data):
        """The arena must hold data at off after the call."""
        self.want[kind][off:off + len(data)] = np.frombuffer(bytes(data), np.uint8)

    def check(self):
        for k in (P, G):
            diff = np.flatnonzero(self.view[k] != self.want[k])
            assert diff.size == 0, "%s arena: %d bytes differ, the first at offset %d" % (k, diff.size, diff[0])

    def close(self):
        self.view = None
        self.eng.free_pinned(self.ptr)


class CrcWords:
    """The blocks' CRC arrays (host memory that the engine fills with memcpy), 0xA5 between them."""

    def __init__(self, lens):
        self.off = [16 + sum(4 * nseg(m) + 16 for m in lens[:i]) for i in range(len(lens))]
        self.buf = np.full(self.off[-1] + 4 * nseg(lens[-1]) + 16, FILL, np.uint8)
        self.want = self.buf.copy()

    def addr(self, i):
        return self.buf.ctypes.data + self.off[i]

    def give(self, i, words):
        """CRC_VERIFY: the array the engine reads."""
        self.buf[self.off[i]:self.off[i] + len(words)] = np.frombuffer(bytes(words), np.uint8)
        self.expect(i, words)

    def expect(self, i, words):
        self.want[self.off[i]:self.off[i] + len(words)] = np.frombuffer(bytes(words), np.uint8)

    def check(self):
        assert np.array_equal(self.buf, self.want)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dkey(eng):
    h = eng.rsa_key(*M.components(M.fixed_keys()[LO.KEY_A]))
    yield h
    eng.rsa_key_free(h)


@pytest.fixture(scope="module")
def arenas(eng):
    a = Arenas(eng)
    yield a
    a.close()


# ---------------------------------------------------------------------------
# jfsx_load_batch
# ---------------------------------------------------------------------------
def load_batch(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    _, algo, codec = case
    pg = pages()
    images = [TL._store(algo, 700 + i, TL._compress(codec, p)) for i, p in enumerate(pg)]
    want = [(E.OK, len(p), p) for p in pg]
    if fail:
        key, nonce, c, tag = images[BAD]
        if algo != E.CIPHER_NONE:
            images[BAD] = (key, nonce, c, bytes([tag[0] ^ 0x10]) + tag[1:])
            want[BAD] = (E.ETAG, 0, None)
        else:
            images[BAD] = (None, None, c[:-1], None)
            st, out_len, _ = LO.decode(codec, c[:-1], len(pg[BAD]))
            assert st == E.EFORMAT
            want[BAD] = (st, out_len, None)
    arenas.reset()
    cw = CrcWords(LENS)
    specs = []
    for i, ((key, nonce, c, tag), p) in enumerate(zip(images, pg)):
        dst, off = arenas.room(kinds[i][1], len(p))
        st, _, page = want[i]
        arenas.expect(kinds[i][1], off, page if st == E.OK else bytes(len(p)))
        cw.expect(i, orc.checksum(page, hw=True) if st == E.OK else bytes(4 * nseg(len(p))))
        specs.append({"key": key, "nonce": nonce, "tag": tag, "src": arenas.put(kinds[i][0], c), "src_len": len(c),
                      "dst": dst if len(p) else None, "len": len(p), "crc": cw.addr(i)})
    arr, n = eng.make_lblocks(specs)
    mark()
    eng.load_batch(algo, codec, arr, n, E.CRC_GEN, E.MEM_HOST)
    mark()
    for i, (st, out_len, _) in enumerate(want):
        assert (arr[i].status, arr[i].out_len) == (st, out_len), i
    arenas.check()
    cw.check()


# ---------------------------------------------------------------------------
# jfsx_load_objects
# ---------------------------------------------------------------------------
def load_objects(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    _, algo, codec = case
    pg = pages()
    cipher = algo != E.CIPHER_NONE
    comps = [LO._compress(codec, p) for p in pg]
    if cipher:
        objs = [LO.make_obj(algo, LO.KEY_A, 40 + i, c) for i, c in enumerate(comps)]
    else:
        objs = [(b"", c, None) for c in comps]
    crc_of = LO.crc_of if cipher else (lambda o: int(orc.object_checksum(o[1], hw=True)))
    expect = [crc_of(o) for o in objs]
    want = [(E.OK, len(p), 32 if cipher else 0, p) for p in pg]
    if fail:
        hdr, c, tag = objs[BAD]
        if cipher:  # the object's checksum holds, its tag does not
            objs[BAD] = (hdr, c, bytes([tag[0] ^ 0x10]) + tag[1:])
            expect[BAD] = crc_of(objs[BAD])
            want[BAD] = LO.classify(LO.KEY_A, algo, codec, objs[BAD], expect[BAD], len(pg[BAD]), True)
            assert want[BAD][0] == E.ETAG
        else:
            flipped = bytearray(c)
            flipped[len(c) // 2] ^= 4
            objs[BAD] = (b"", bytes(flipped), None)
            assert crc_of(objs[BAD]) != expect[BAD]
            want[BAD] = (E.ECRC, 0, 0, None)
    arenas.reset()
    cw = CrcWords(LENS)
    hdrs = [np.frombuffer(h, np.uint8).copy() if len(h) else None for h, _, _ in objs]
    specs = []
    for i, ((h, c, tag), p) in enumerate(zip(objs, pg)):
        dst, off = arenas.room(kinds[i][1], len(p))
        st, _, _, page = want[i]
        arenas.expect(kinds[i][1], off, page if st == E.OK else bytes(len(p)))
        cw.expect(i, orc.checksum(page, hw=True) if st == E.OK else bytes(4 * nseg(len(p))))
        src = arenas.put(kinds[i][0], c)
        specs.append({"hdr": hdrs[i].ctypes.data if len(h) else None, "hdr_len": len(h), "tag": tag,
                      "src": src if len(c) else None, "src_len": len(c), "dst": dst if len(p) else None,
                      "len": len(p), "crc": cw.addr(i), "expect_crc": expect[i]})
    arr, n = eng.make_oblocks(specs)
    mark()
    eng.load_objects_batch(dkey if cipher else None, algo, codec, arr, n, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
    mark()
    for i, (st, out_len, key_len, _) in enumerate(want):
        assert (arr[i].status, arr[i].out_len, arr[i].key_len) == (st, out_len, key_len), i
        assert arr[i].obj_crc == crc_of(objs[i]), i
    arenas.check()
    cw.check()


# ---------------------------------------------------------------------------
# jfsx_store_batch
# ---------------------------------------------------------------------------
def _verify_words(pg, cw, fail):
    """CRC_VERIFY: every page's CRC array, block BAD's last word wrong when fail -> (good, given) of BAD."""
    good = [bytes(orc.checksum(p, hw=True)) for p in pg]
    seg = nseg(len(pg[BAD])) - 1
    given = bytearray(good[BAD])
    if fail:
        given[4 * seg + 1] ^= 0x20
    for i, g in enumerate(good):
        cw.give(i, given if i == BAD else g)
    word = lambda b: int.from_bytes(b[4 * seg:4 * seg + 4], "big")  # noqa: E731
    return seg, word(good[BAD]), word(given)


def store_batch(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    _, algo, codec = case
    pg = pages()
    want = [TS._image(algo, 800 + i, TS._compress(codec, p)) for i, p in enumerate(pg)]
    arenas.reset()
    cw = CrcWords(LENS)
    if fail:
        seg, got, given = _verify_words(pg, cw, True)
    hdr = np.frombuffer(TS.HDR, np.uint8).copy()
    specs = []
    for i, (p, (key, nonce, img, _, _)) in enumerate(zip(pg, want)):
        cap = TS._bound(codec, len(p))
        dst, off = arenas.room(kinds[i][1], cap)
        if not (fail and i == BAD):
            arenas.expect(kinds[i][1], off, img)  # dst[0, out_len) alone
        if not fail:
            cw.expect(i, orc.checksum(p, hw=True))
        src = arenas.put(kinds[i][0], p)
        specs.append({"key": key, "nonce": nonce, "src": src if len(p) else None, "len": len(p), "dst": dst,
                      "dst_cap": cap, "crc": cw.addr(i), "hdr": hdr.ctypes.data, "hdr_len": hdr.size})
    arr, n = eng.make_sblocks(specs)
    mark()
    eng.store_batch(algo, codec, arr, n, (E.CRC_VERIFY if fail else E.CRC_GEN) | E.CRC_CT, E.MEM_HOST)
    mark()
    for i, (_, _, img, tag, obj) in enumerate(want):
        s = arr[i]
        if fail and i == BAD:
            assert (s.status, s.out_len, s.crc_bad_seg, s.crc_got, s.crc_expect) == (E.ECRC, 0, seg, got, given)
            assert bytes(s.tag) == bytes(16) and s.obj_crc == 0
        else:
            assert (s.status, s.out_len, s.crc_bad_seg, s.crc_got, s.crc_expect) == (E.OK, len(img), -1, 0, 0), i
            assert bytes(s.tag) == tag and s.obj_crc == obj, i
    arenas.check()
    cw.check()


# ---------------------------------------------------------------------------
# jfsx_store_objects
# ---------------------------------------------------------------------------
def store_objects(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    _, algo, codec = case
    pg = pages()
    blks = [900 + i for i in range(len(pg))]
    want = [SO.expected(algo, codec, SO.KEY_A, b, p) for b, p in zip(blks, pg)]
    arenas.reset()
    cw = CrcWords(LENS)
    if fail:
        seg, got, given = _verify_words(pg, cw, True)
    specs = []
    for i, (p, (obj, _, crc, _)) in enumerate(zip(pg, want)):
        cap = SO._bound(codec, len(p))
        dst, off = arenas.room(kinds[i][1], cap)
        if not (fail and i == BAD):
            arenas.expect(kinds[i][1], off, obj)  # obj[0, out_len) alone
        if not fail:
            cw.expect(i, crc)
        src = arenas.put(kinds[i][0], p)
        key, seed, nonce = SO.draw(blks[i])
        specs.append({"key": key, "nonce": nonce, "seed": seed, "src": src if len(p) else None, "len": len(p),
                      "obj": dst, "obj_cap": cap, "crc": cw.addr(i)})
    arr, n = eng.make_soblocks(specs)
    mark()
    eng.store_objects_batch(dkey, M.E, algo, codec, arr, n, (E.CRC_VERIFY if fail else E.CRC_GEN) | E.CRC_CT,
                            E.MEM_HOST)
    mark()
    for i, (obj, img_len, _, ocrc) in enumerate(want):
        r = arr[i]
        if fail and i == BAD:
            assert (r.status, r.out_len, r.img_len, r.obj_crc) == (E.ECRC, 0, 0, 0)
            assert (r.crc_bad_seg, r.crc_got, r.crc_expect) == (seg, got, given)
        else:
            assert (r.status, r.out_len, r.img_len, r.obj_crc) == (E.OK, len(obj), img_len, ocrc), i
            assert (r.crc_bad_seg, r.crc_got, r.crc_expect) == (-1, 0, 0), i
    arenas.check()
    cw.check()


# ---------------------------------------------------------------------------
# jfsx_gather_batch: no block of it can fail
# ---------------------------------------------------------------------------
def gather_batch(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    sources = pages()
    # (source, src_off, len) runs of every page, -1 a hole; the pages have the table's lengths
    runs = [[(0, 0, 1)],
            [(1, 0, 1000), (-1, 0, 96), (3, 5, 3000)],
            [(2, 17, 30000), (3, 1, 35553)],
            [(3, 0, 100000), (2, 0, 65553), (-1, 0, 4447), (1, 0, 4096), (3, 100000, 25904)],
            []]
    pieces, pg = [], []
    for r, m in zip(runs, LENS):
        assert sum(p[2] for p in r) == m
        pg.append((len(pieces), len(r), m))
        pieces += r
    arenas.reset()
    gs, gd = (E.jfsx_gsrc * 5)(), (E.jfsx_gdst * 5)()
    for i, s in enumerate(sources):
        src = arenas.put(kinds[i][0], s)
        gs[i].data, gs[i].len = (src if len(s) else None), len(s)
    for j, ((first, count, m), w) in enumerate(zip(pg, CM.gather_want(sources, pg, pieces))):
        dst, off = arenas.room(kinds[j][1], m)
        arenas.expect(kinds[j][1], off, w.tobytes())
        gd[j].data, gd[j].len, gd[j].piece_first, gd[j].piece_count = (dst if m else None), m, first, count
    pa, n_piece = E.make_pieces(pieces)
    mark()
    eng.gather_batch(5, gs, 5, gd, n_piece, pa, E.MEM_HOST)
    mark()
    arenas.check()


# ---------------------------------------------------------------------------
# jfsx_open_range_batch
# ---------------------------------------------------------------------------
def open_range_batch(eng, arenas, case, kinds, fail=False, dkey=None, mark=lambda: None):
    windows = [(0, -1), (100, 3000), (5, 40000), (65536 - 5, 32768 + 10), (0, -1)]
    items = [TR.Item(TR.block(E.PLAN_GCM, m, 7 + i), off, limit, flip_tag=fail and i == BAD)
             for i, (m, (off, limit)) in enumerate(zip(LENS, windows))]
    arenas.reset()
    specs = []
    for i, it in enumerate(items):
        dst, off = arenas.room(kinds[i][1], it.n + TR.PAD)
        arenas.expect(kinds[i][1], off, it.want)  # dst[0, n) alone; zeros where the tag failed
        src = arenas.put(kinds[i][0], it.c)
        specs.append({"key": it.blk.key, "nonce": it.blk.nonce, "tag": it.tag, "src": src if it.blk.n else None,
                      "len": it.blk.n, "off": it.off, "limit": it.limit, "dst": dst if it.n else None,
                      "dst_cap": it.n + TR.PAD if it.n else 0, "crc": None})
    arr, n = E.Engine.make_rblocks(specs)
    mark()
    eng.open_range_batch(E.AES256GCM, arr, n, E.CRC_NONE, E.MEM_HOST)
    mark()
    for i, it in enumerate(items):
        assert (arr[i].status, arr[i].out_len) == ((E.ETAG, 0) if it.bad else (E.OK, it.n)), i
    arenas.check()


# ---------------------------------------------------------------------------
# the tests: every call in every layout; scripts/staging_copies.py runs the
# same batches under a copy trace
# ---------------------------------------------------------------------------
CALLS = {"load_batch": (load_batch, [GCM_LZ4, NONE_ZSTD]),
         "load_objects": (load_objects, [GCM_LZ4, GCM_NONE, NONE_ZSTD]),
         "store_batch": (store_batch, [GCM_LZ4, NONE_ZSTD]),
         "store_objects": (store_objects, [GCM_LZ4, GCM_NONE, GCM_ZSTD]),
         "gather_batch": (gather_batch, [None]),
         "open_range_batch": (open_range_batch, [None])}


def _run(call, eng, dkey, arenas, case, layout):
    CALLS[call][0](eng, arenas, case, LAYOUTS[layout], fail=layout == "fail", dkey=dkey)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CALLS["load_batch"][1], ids=ids)
def test_load_batch(eng, dkey, arenas, case, layout):
    _run("load_batch", eng, dkey, arenas, case, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CALLS["load_objects"][1], ids=ids)
def test_load_objects(eng, dkey, arenas, case, layout):
    _run("load_objects", eng, dkey, arenas, case, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CALLS["store_batch"][1], ids=ids)
def test_store_batch(eng, dkey, arenas, case, layout):
    _run("store_batch", eng, dkey, arenas, case, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CALLS["store_objects"][1], ids=ids)
def test_store_objects(eng, dkey, arenas, case, layout):
    _run("store_objects", eng, dkey, arenas, case, layout)


@pytest.mark.parametrize("layout", ["mixed", "pinned"])  # no block of a gather can fail
def test_gather_batch(eng, dkey, arenas, layout):
    _run("gather_batch", eng, dkey, arenas, None, layout)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_open_range_batch(eng, dkey, arenas, layout):
    _run("open_range_batch", eng, dkey, arenas, None, layout)
