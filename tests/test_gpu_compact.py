"""GPU tests of one-call slice compaction (jfsx_compact_objects, and
compress.compact_fused over it): stored objects in, stored objects out, the
pages assembled in device memory.

A stored object is BE16(256) | 12 | wrapped key | nonce | seal(compress(page))
| tag.  No expected value comes from the engine: the plan is
tests/compact_model.plan's, the new pages are its byte model of Compact, the
wrapped keys are tests/rsa_model.py's on the fixed keys of
tests/golden/rsa_keys.json, the compressed bytes oracle.lz4_compress or
tests.zstd_lib.compress_simple, C and the tag oracle.seal, the checksums
oracle.checksum and oracle.object_checksum."""
import functools

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import compact_model as CM
from tests import lz4_data, zstd_lib
from tests import rsa_model as M

pytestmark = pytest.mark.gpu

CIPHERS = [E.AES256GCM, E.CHACHA20P1305]
CODECS = [E.CODEC_NONE, E.CODEC_LZ4, E.CODEC_ZSTD]
CODEC_IDS = ["none", "lz4", "zstd"]
SEED = 0xC0B
KEY_A, KEY_B = "plain_p_gt_q", "wide_q_gt_p"
HDR, TAG = 271, 16
GUARD = 64
BS = 64 << 10


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dkeys(eng):
    h = {nm: eng.rsa_key(*M.components(M.fixed_keys()[nm])) for nm in (KEY_A, KEY_B)}
    yield h
    for v in h.values():
        eng.rsa_key_free(v)


def _orc_algo(algo):
    return orc.AES256GCM if algo == E.AES256GCM else orc.CHACHA20P1305


@functools.lru_cache(maxsize=None)
def _compress(codec, plain):
    if codec == E.CODEC_NONE:
        return bytes(plain)
    return orc.lz4_compress(plain) if codec == E.CODEC_LZ4 else zstd_lib.compress_simple(plain)


def _nseg(n):
    return max(1, -(-n // E.SEG))


def _bound(codec, n):
    """jfsx_object_bound, written out."""
    img = n if codec == E.CODEC_NONE else n + n // 255 + 16 if codec == E.CODEC_LZ4 else \
        n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)
    return HDR + img + TAG


@functools.lru_cache(maxsize=None)
def wrap(name, key, seed):
    return M.ct256(M.encrypt_em(M.fixed_keys()[name], M.oaep_encode(key, seed)))


def draw(blk):
    """(data key, seed, nonce) of block blk; keys repeat every 8 blocks, nonces and seeds do not."""
    key, _ = orc.gen_key(SEED, blk % 8)
    _, nonce = orc.gen_key(SEED, blk)
    return bytes(key), M.det_bytes(32, "compact seed", blk), bytes(nonce)


@functools.lru_cache(maxsize=None)
def sealed(algo, codec, name, key, seed, nonce, page):
    """(object, img_len, page crcs, obj_crc) of one page from the checkers alone."""
    c, tag = orc.seal(_orc_algo(algo), key, nonce, _compress(codec, page), fast=True)
    obj = bytes([1, 0, 12]) + wrap(name, key, seed) + nonce + bytes(c) + bytes(tag)
    return obj, len(c), bytes(orc.checksum(page, hw=True)), int(orc.object_checksum(obj, hw=True))


def expected(algo, codec, name, blk, page):
    return sealed(algo, codec, name, *draw(blk), bytes(page))


def cut(obj):
    return obj[:HDR], obj[HDR:-TAG], obj[-TAG:]


def seeded_case(seed, n_slices=12):
    """About n_slices source slices of one to three blocks of BS plus an odd
    tail, with holes at the head, in the middle and at the tail; one id twice.
    -> (slices, data)."""
    rng = np.random.default_rng(seed)
    data, slices = {}, [(0, 700, 0, 700)]
    for sid in range(1, n_slices + 1):
        size = int(rng.integers(0, 3)) * BS + int(rng.integers(1, BS)) | 1
        data[sid] = lz4_data.sample("text" if sid % 4 else "runs", size, seed=seed + sid)
        off = int(rng.integers(0, max(1, size // 2))) if sid % 3 else 0
        ln = int(rng.integers(1, size - off + 1)) if sid % 3 == 1 else size - off
        slices.append((sid, size, off, ln))
        if sid % 5 == 0:
            slices.append((0, 0, 0, int(rng.integers(1, BS + 100))))
    first = slices[1]
    slices.append((first[0], first[1], 0, min(first[1], 1000)))  # the same id again: its block 0 is shared
    slices.append((0, 0, 0, 33))
    return slices, {k: bytes(v) for k, v in data.items()}


class Scenario:
    """One compaction from the checkers: the plan, the stored source objects
    (block blk0 + i sealed under key `name`) and the new pages."""

    def __init__(self, algo, codec, name, slices, data, blk0, bs=BS):
        self.algo, self.codec, self.name, self.blk0 = algo, codec, name, blk0
        self.sources, self.pages, self.pieces = CM.plan(bs, slices)
        blocks = CM.slice_blocks(data, bs)
        self.src_pages = [blocks[(sid, indx)] for sid, indx, _ in self.sources]
        assert [len(p) for p in self.src_pages] == [b for _, _, b in self.sources]
        self.src_objs = [expected(algo, codec, name, blk0 + i, p)[0] for i, p in enumerate(self.src_pages)]
        self.new_pages = CM.compact_bytes(slices, data, bs)
        assert [len(p) for p in self.new_pages] == [n for _, _, n in self.pages]
        self.new_blks = [blk0 + 5000 + j for j in range(len(self.pages))]

    def want(self, j):
        return expected(self.algo, self.codec, self.name, self.new_blks[j], self.new_pages[j])


class CBatch:
    """The records of one jfsx_compact_objects call.  Object buffers (obj_cap =
    the bound exactly, a guard behind each) and CRC arrays are pre-filled with
    0xA5; images and objects lie at odd offsets."""

    def __init__(self, codec, src_objs, lengths, pages, pieces, new_blks, expect=None, with_crc=True):
        self.codec, self.pages, self.pieces = codec, list(pages), list(pieces)
        self.keep = []
        specs = []
        for i, (obj, n) in enumerate(zip(src_objs, lengths)):
            hdr, c, tag = obj if isinstance(obj, tuple) else cut(obj)
            hb = np.frombuffer(hdr, np.uint8).copy()
            cb = np.zeros(len(c) + 3, np.uint8)
            cb[3:] = np.frombuffer(c, np.uint8)
            self.keep += [hb, cb]
            specs.append({"hdr": hb.ctypes.data, "hdr_len": hb.size, "tag": tag,
                          "src": cb.ctypes.data + 3 if len(c) else None, "src_len": len(c), "dst": None, "len": n,
                          "expect_crc": expect[i] if expect is not None else 0})
        self.oarr, self.n_src = E.Engine.make_oblocks(specs)
        self.caps = [_bound(codec, n) for _, _, n in self.pages]
        self.ooff, self.coff = [], []
        oo = co = 0
        for cap, (_, _, n) in zip(self.caps, self.pages):
            self.ooff.append(oo + 5)
            self.coff.append(co)
            oo += (cap + GUARD + 47) & ~15
            co += 4 * _nseg(n)
        self.obj = np.full(oo + 16, 0xA5, np.uint8)
        self.crc_end = co
        self.cw = np.full(co + GUARD, 0xA5, np.uint8)
        sspecs = []
        for j, (_, _, n) in enumerate(self.pages):
            key, seed, nonce = draw(new_blks[j])
            sspecs.append({"key": key, "nonce": nonce, "seed": seed, "src": None, "len": n,
                           "obj": self.obj.ctypes.data + self.ooff[j], "obj_cap": self.caps[j],
                           "crc": self.cw.ctypes.data + self.coff[j] if with_crc else None})
        self.sarr, self.n_dst = E.Engine.make_soblocks(sspecs)
        self.cp = (E.jfsx_cpage * max(self.n_dst, 1))()
        for j, (first, count, _) in enumerate(self.pages):
            self.cp[j].piece_first, self.cp[j].piece_count, self.cp[j].src_bad = first, count, 77
        self.pa, self.n_piece = E.make_pieces(self.pieces)

    def run(self, eng, key, algo, src_mode, dst_mode, e=M.E):
        eng.compact_objects_batch(key, e, algo, self.codec, self.n_src, self.oarr, src_mode, self.n_dst, self.sarr,
                                  self.cp, dst_mode, self.n_piece, self.pa)
        return self

    def object(self, j):
        return self.obj[self.ooff[j]:self.ooff[j] + self.sarr[j].out_len].tobytes()

    def crcs(self, j):
        return self.cw[self.coff[j]:self.coff[j] + 4 * _nseg(self.pages[j][2])].tobytes()

    def slot_untouched(self, j):
        end = self.ooff[j + 1] if j + 1 < len(self.ooff) else self.obj.size
        return bool((self.obj[self.ooff[j]:end] == 0xA5).all())

    def guards_ok(self):
        at = 0
        for j, o in enumerate(self.ooff):
            if not (self.obj[at:o] == 0xA5).all():
                return False
            at = o + self.sarr[j].out_len
        return bool((self.obj[at:] == 0xA5).all() and (self.cw[self.crc_end:] == 0xA5).all())


def batch_of(sc, expect=True, with_crc=True):
    exp = [int(orc.object_checksum(o, hw=True)) for o in sc.src_objs] if expect else None
    return CBatch(sc.codec, sc.src_objs, [len(p) for p in sc.src_pages], sc.pages, sc.pieces, sc.new_blks,
                  expect=exp, with_crc=with_crc)


def check_all_good(sc, b, gen=True, ct=True):
    for i in range(b.n_src):
        o = b.oarr[i]
        assert (o.status, o.out_len, o.key_len) == (E.OK, len(sc.src_pages[i]), 32), i
    for j in range(b.n_dst):
        obj, img_len, crcs, obj_crc = sc.want(j)
        r = b.sarr[j]
        assert (r.status, b.cp[j].src_bad) == (E.OK, -1), j
        assert (r.out_len, r.img_len) == (len(obj), img_len), j
        assert b.object(j) == obj, j
        if gen:
            assert b.crcs(j) == crcs, j
        if ct:
            assert r.obj_crc == obj_crc, j
    assert b.guards_ok()


def _delta(m0, m1):
    d = {k: m1[k] - m0[k] for k in m1 if isinstance(m1[k], int) and m1[k] != m0[k]}
    d.pop("kernel_launches", None)
    return d


# ---------------------------------------------------------------------------
# the matrix: both ciphers x {none, lz4, zstd} at block 64 KiB
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_matrix(eng, dkeys, algo, codec):
    # another slice list and other bytes per case: what the previous case left in the engine's buffers is wrong here
    case = 3 * CIPHERS.index(algo) + CODECS.index(codec)
    slices, data = seeded_case(0x3A70 + 16 * case)
    sc = Scenario(algo, codec, KEY_A, slices, data, blk0=100 + 40 * case)
    assert len(sc.sources) >= 12 and len(sc.pages) >= 6 and any(s < 0 for s, _, _ in sc.pieces)
    b = batch_of(sc).run(eng, dkeys[KEY_A], algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT)
    check_all_good(sc, b)
    for i in range(b.n_src):
        assert b.oarr[i].obj_crc == int(orc.object_checksum(sc.src_objs[i], hw=True)), i
    # the round trip of what came down, through the checkers, is the byte model
    for j in range(b.n_dst):
        key, _, _ = draw(sc.new_blks[j])
        comp = orc.data_decrypt(_orc_algo(algo), key, b.object(j))
        n = len(sc.new_pages[j])
        page = comp if codec == E.CODEC_NONE else orc.lz4_decompress(comp, n)[1] if codec == E.CODEC_LZ4 else \
            zstd_lib.decompress(comp, n)[1]
        assert bytes(page) == sc.new_pages[j], j


@pytest.mark.parametrize("mode", [(0, E.CRC_NONE), (0, E.CRC_GEN), (E.CRC_CT, E.CRC_CT)], ids=["none", "gen", "ct"])
def test_modes(eng, dkeys, mode):
    slices, data = seeded_case(0x3A8, n_slices=5)
    for codec in CODECS:
        sc = Scenario(E.AES256GCM, codec, KEY_B, slices, data, blk0=300)
        gen, ct = bool(mode[1] & E.CRC_GEN), bool(mode[1] & E.CRC_CT)
        b = batch_of(sc, expect=bool(mode[0]), with_crc=gen).run(eng, dkeys[KEY_B], E.AES256GCM, mode[0], mode[1])
        check_all_good(sc, b, gen=gen, ct=ct)
        assert (b.cw[:b.crc_end] == 0xA5).all() or gen
        if not ct:
            assert all(b.sarr[j].obj_crc == 0 for j in range(b.n_dst))


# ---------------------------------------------------------------------------
# the gate: four failed sources in one batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_gate_failed_sources(eng, dkeys, algo):
    codec = E.CODEC_LZ4
    n_src = 10
    full = [lz4_data.sample("text", 20000 + 1000 * i, seed=400 + i) for i in range(n_src)]
    lengths = [len(p) for p in full]
    objs = [expected(algo, codec, KEY_A, 600 + i, bytes(p))[0] for i, p in enumerate(full)]
    # 1: a corrupted tag; 3: a wrong expect_crc; 5: a corrupted wrapped key; 7: an image that decodes short
    objs[1] = objs[1][:-3] + bytes([objs[1][-3] ^ 0x10]) + objs[1][-2:]
    objs[5] = objs[5][:40] + bytes([objs[5][40] ^ 0x01]) + objs[5][41:]
    objs[7] = expected(algo, codec, KEY_A, 607, bytes(full[7][:15000]))[0]
    expect = [int(orc.object_checksum(o, hw=True)) for o in objs]
    expect[3] ^= 0x00010000
    status = {1: E.ETAG, 3: E.ECRC, 5: E.EKEY, 7: E.ESHORT}
    assert M.decrypt(M.fixed_keys()[KEY_A], objs[5][3:259]) is None  # the checker: this key does not unwrap
    # pages: (pieces) -> the failed source the gate names, in piece order
    runs = [
        ([(0, 0, 5000), (-1, 0, 10), (2, 3, 7000)], -1),
        ([(0, 5, 100), (1, 0, 2000)], 1),
        ([(-1, 0, 64)], -1),
        ([(2, 0, 1), (3, 17, 300), (4, 0, 9)], 3),
        ([(4, 100, 20000), (5, 1, 1)], 5),
        ([(6, 0, 26000), (7, 14999, 2), (1, 0, 1)], 7),  # two failed sources: the first in piece order
        ([(5, 0, 10), (3, 0, 10), (8, 0, 10)], 5),
        ([(8, 1, 27999), (9, 0, 29000), (9, 0, 29000), (-1, 0, 7)], -1),
        ([(7, 0, 100)], 7),  # bytes the short image does hold: the source failed as a whole
    ]
    pages, pieces = [], []
    for run, _ in runs:
        pages.append((len(pieces), len(run), sum(n for _, _, n in run)))
        pieces += run
    new_blks = list(range(700, 700 + len(pages)))
    b = CBatch(codec, objs, lengths, pages, pieces, new_blks, expect=expect)
    m0 = eng.metrics()
    b.run(eng, dkeys[KEY_A], algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT)
    m1 = eng.metrics()
    for i in range(n_src):
        o = b.oarr[i]
        assert o.status == status.get(i, E.OK), i
        assert o.out_len == (lengths[i] if i not in status else 15000 if i == 7 else 0), i
        assert o.obj_crc == int(orc.object_checksum(objs[i], hw=True)), i
    assert b.oarr[5].key_len == -1 and b.oarr[0].key_len == 32
    srcs = [bytes(p) for p in full]
    want_pages = CM.gather_want(srcs, pages, pieces)
    good = []
    for j, (_, bad) in enumerate(runs):
        r = b.sarr[j]
        assert b.cp[j].src_bad == bad, j
        if bad >= 0:
            assert (r.status, r.out_len, r.img_len, r.obj_crc) == (E.ESRC, 0, 0, 0), j
            assert b.slot_untouched(j), j
            continue
        good.append(j)
        obj, img_len, crcs, obj_crc = expected(algo, codec, KEY_A, new_blks[j], want_pages[j].tobytes())
        assert (r.status, r.out_len, r.img_len, r.obj_crc) == (E.OK, len(obj), img_len, obj_crc), j
        assert b.object(j) == obj and b.crcs(j) == crcs, j
    assert b.guards_ok()
    # what jfsx_load_objects counts over the ten sources and jfsx_store_objects over the good pages
    img = [len(o) - HDR - TAG for o in objs]
    decoded = [i for i in range(n_src) if i not in (1, 3, 5)]
    imgs_out = sum(b.sarr[j].img_len for j in good)
    plens = sum(pages[j][2] for j in good)
    want = {"open_batches": 1, "open_blocks": 8, "open_bytes": sum(img[i] for i in range(n_src) if i not in (3, 5)),
            "open_fail": 1, "lz4d_blocks": 7, "lz4d_in": sum(img[i] for i in decoded),
            "lz4d_out": sum(15000 if i == 7 else lengths[i] for i in decoded),
            "crc_batches": 2, "crc_ranges": n_src + len(good), "crc_bytes": sum(img) + plens, "crc_fail": 1,
            "seal_batches": 1, "seal_blocks": len(good), "seal_bytes": imgs_out,
            "lz4c_blocks": len(good), "lz4c_in": plens, "lz4c_out": imgs_out}
    assert _delta(m0, m1) == want


def test_all_sources_failed_stores_nothing(eng, dkeys):
    page = lz4_data.sample("text", 5000, seed=450)
    obj = expected(E.AES256GCM, E.CODEC_NONE, KEY_A, 650, bytes(page))[0]
    obj = obj[:-1] + bytes([obj[-1] ^ 1])
    b = CBatch(E.CODEC_NONE, [obj], [5000], [(0, 1, 4000), (1, 1, 8)], [(0, 3, 4000), (-1, 0, 8)], [750, 751])
    m0 = eng.metrics()
    b.run(eng, dkeys[KEY_A], E.AES256GCM, 0, E.CRC_GEN | E.CRC_CT)
    d = _delta(m0, eng.metrics())
    assert b.oarr[0].status == E.ETAG
    assert (b.sarr[0].status, b.cp[0].src_bad, b.sarr[0].out_len) == (E.ESRC, 0, 0) and b.slot_untouched(0)
    want = expected(E.AES256GCM, E.CODEC_NONE, KEY_A, 751, bytes(8))
    assert (b.sarr[1].status, b.cp[1].src_bad) == (E.OK, -1) and b.object(1) == want[0]  # an all-hole page has no source
    assert d["seal_blocks"] == 1 and d["open_fail"] == 1
    # ... and with that page gone too, no store stage runs at all
    b = CBatch(E.CODEC_NONE, [obj], [5000], [(0, 1, 4000)], [(0, 3, 4000)], [750])
    m0 = eng.metrics()
    b.run(eng, dkeys[KEY_A], E.AES256GCM, 0, E.CRC_GEN | E.CRC_CT)
    d = _delta(m0, eng.metrics())
    assert b.sarr[0].status == E.ESRC and b.slot_untouched(0) and (b.cw == 0xA5).all()
    assert "seal_batches" not in d and "seal_blocks" not in d


def test_all_hole_chunk_has_no_sources(eng, dkeys):
    """A slice list of holes alone: no source, no load stage, pages of zeros."""
    slices = [(0, 0, 0, BS - 5), (0, 0, 0, 700)]
    for codec in CODECS:
        sc = Scenario(E.CHACHA20P1305, codec, KEY_B, slices, {}, blk0=780)
        assert sc.sources == [] and [n for _, _, n in sc.pages] == [BS, 695]
        m0 = eng.metrics()
        b = batch_of(sc).run(eng, dkeys[KEY_B], sc.algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT)
        d = _delta(m0, eng.metrics())
        check_all_good(sc, b)
        assert d["seal_blocks"] == 2 and "open_batches" not in d


# ---------------------------------------------------------------------------
# equality with the separate calls; a shared source block; interleaving
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
def test_equals_the_separate_calls(eng, dkeys, codec):
    algo = E.CHACHA20P1305 if codec == E.CODEC_LZ4 else E.AES256GCM
    slices, data = seeded_case(0x3A9, n_slices=6)
    sc = Scenario(algo, codec, KEY_B, slices, data, blk0=800)
    expect = [int(orc.object_checksum(o, hw=True)) for o in sc.src_objs]
    draws = [draw(k) for k in sc.new_blks]
    m0 = eng.metrics()
    one = eng.compact_objects(dkeys[KEY_B], M.E, algo, codec, [cut(o) for o in sc.src_objs],
                              [len(p) for p in sc.src_pages], draws, sc.pages, sc.pieces, expect=expect)
    m1 = eng.metrics()
    # jfsx_load_objects, numpy assembly, jfsx_store_objects
    loaded = eng.load_objects(dkeys[KEY_B], algo, codec, [cut(o) for o in sc.src_objs],
                              [len(p) for p in sc.src_pages], crc=False, expect=expect)
    assert [st for st, _, _ in loaded] == [E.OK] * len(loaded)
    assembled = CM.gather_want([p for _, p, _ in loaded], sc.pages, sc.pieces)
    stored = eng.store_objects(dkeys[KEY_B], M.E, algo, codec,
                               [(k, s, n, p) for (k, s, n), p in zip(draws, assembled)])
    m2 = eng.metrics()
    assert [(st, obj, crc, ocrc) for st, obj, crc, ocrc, _ in one] == stored
    assert [bad for _, _, _, _, bad in one] == [-1] * len(one)
    assert [o for _, o, _, _, _ in one] == [sc.want(j)[0] for j in range(len(one))]
    assert _delta(m0, m1) == _delta(m1, m2)  # jfsx_metrics counts what the separate calls count


def test_shared_source_block_is_decoded_once(eng, dkeys):
    codec, algo = E.CODEC_LZ4, E.AES256GCM
    data = {9: bytes(lz4_data.sample("text", BS + 501, seed=460))}
    size = len(data[9])
    slices = [(9, size, 10, 300), (0, 0, 0, 5), (9, size, 200, 400), (9, size, BS - 7, 20), (9, size, 0, 64)]
    sc = Scenario(algo, codec, KEY_A, slices, data, blk0=900)
    assert sc.sources == [(9, 0, BS), (9, 1, 501)]  # four records, two stored blocks
    b = batch_of(sc)
    m0 = eng.metrics()
    b.run(eng, dkeys[KEY_A], algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT)
    d = _delta(m0, eng.metrics())
    check_all_good(sc, b)
    assert (d["open_blocks"], d["lz4d_blocks"], d["lz4d_out"]) == (2, 2, size)


def test_interleaved_with_load_and_store_under_two_keys(eng, dkeys):
    codec, algo = E.CODEC_ZSTD, E.AES256GCM
    slices, data = seeded_case(0x3AA, n_slices=4)
    sa = Scenario(algo, codec, KEY_A, slices, data, blk0=1000)
    sb = Scenario(E.CHACHA20P1305, E.CODEC_LZ4, KEY_B, slices, data, blk0=1100)
    pages = [bytes(lz4_data.sample("text", n, seed=470)) for n in (9, 40000, 70000)]
    for _ in range(2):
        check_all_good(sa, batch_of(sa).run(eng, dkeys[KEY_A], algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT))
        got = eng.load_objects(dkeys[KEY_B], sb.algo, sb.codec, [cut(o) for o in sb.src_objs],
                               [len(p) for p in sb.src_pages], crc=True)
        assert [(st, p) for st, p, _ in got] == [(E.OK, p) for p in sb.src_pages]
        check_all_good(sb, batch_of(sb).run(eng, dkeys[KEY_B], sb.algo, E.CRC_CT, E.CRC_GEN | E.CRC_CT))
        st = eng.store_objects(dkeys[KEY_A], M.E, algo, codec, [draw(1200 + i) + (p,) for i, p in enumerate(pages)])
        assert [o for _, o, _, _ in st] == [expected(algo, codec, KEY_A, 1200 + i, p)[0] for i, p in enumerate(pages)]


# ---------------------------------------------------------------------------
# the port of TestCompact (pkg/vfs/compact_test.go:28-87) through compact_fused
# ---------------------------------------------------------------------------
def test_port_of_testcompact(eng):
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as EN
    from juicefs_amd.chunk import block_key
    from tests.test_gpu_rsa_wrap import Rand, pem_of
    name, algo, bs = "wide_p_gt_q", E.AES256GCM, 256 << 10
    rsae = EN.NewRSAEncryptor(EN.ParseRsaPrivateKeyFromPem(pem_of(M.fixed_keys()[name])))
    comp = C.NewCompressor("lz4", eng)
    # 100 slices of 100 + 100 i bytes with ids 0 .. 99; id 0 is a hole, as in the reference's test
    slices = [(i, 100 + 100 * i, 0, 100 + 100 * i) for i in range(100)]
    data = {i: bytes(lz4_data.sample("text", 100 + 100 * i, seed=500 + i)) for i in range(1, 100)}
    store, sums = EN.MemStorage(), {}
    for i in range(1, 100):
        k = block_key(i, 0, len(data[i]))
        assert k == "chunks/0/0/%d_0_%d" % (i, 100 + 100 * i)
        obj = expected(algo, E.CODEC_LZ4, name, 2000 + i, data[i])[0]
        store.Put(k, obj)
        sums[k] = orc.object_checksum(obj, hw=True)
    before = store.List()
    rnd = Rand("compact")
    keys, objs, crcs, osums = C.compact_fused(store, slices, 1000, bs, comp, EN.DataEncryptor(rsae, algo, eng, rand=rnd),
                                              object_checksums=sums)
    model = CM.compact_bytes(slices, data, bs)
    assert [len(p) for p in model] == [262144, 242856]
    assert keys == ["chunks/0/1/1000_0_262144", "chunks/0/1/1000_1_242856"]
    assert rnd.calls == [32, 32, 12] * 2
    replay = Rand("compact")
    for k, o, crc, osum, page in zip(keys, objs, crcs, osums, model):
        key, seed, nonce = replay(32), replay(32), replay(12)
        want = sealed(algo, E.CODEC_LZ4, name, key, seed, nonce, page)
        assert o == want[0] and bytes(store.Get(k, 0, -1)) == o
        assert crc == want[2] and osum == str(want[3])
        assert o[:HDR] == bytes([1, 0, 12]) + wrap(name, key, seed) + nonce
        comp_bytes = orc.data_decrypt(_orc_algo(algo), key, o)
        assert orc.lz4_decompress(comp_bytes, len(page))[1] == page
    assert store.List() == sorted(before + keys)
    # the "failed" half: one source is gone from the store; nothing is Put
    gone = block_key(42, 0, 4300)
    store.Delete(gone)
    for k in keys:
        store.Delete(k)
    left = store.List()
    with pytest.raises(C.CompressError) as ei:
        C.compact_fused(store, slices, 1001, bs, comp, EN.DataEncryptor(rsae, algo, eng, rand=Rand("compact")),
                        object_checksums=sums)
    assert gone in str(ei.value)
    assert store.List() == left
    # ... and a source that is there but does not verify: the error names its key and status
    bad = block_key(7, 0, 800)
    o = bytes(store.Get(bad, 0, -1))
    store.Put(gone, expected(algo, E.CODEC_LZ4, name, 2042, data[42])[0])
    store.Put(bad, o[:-1] + bytes([o[-1] ^ 0x80]))
    sums2 = dict(sums)
    del sums2[bad]
    left = store.List()
    with pytest.raises(C.CompressError) as ei:
        C.compact_fused(store, slices, 1002, bs, comp, EN.DataEncryptor(rsae, algo, eng, rand=Rand("compact")),
                        object_checksums=sums2)
    assert bad in str(ei.value) and "status %d" % E.ETAG in str(ei.value)
    assert store.List() == left
