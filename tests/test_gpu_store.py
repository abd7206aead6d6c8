"""GPU tests of the one-call block store (jfsx_store_batch): verify or
checksum() of the page, compress, Seal and the object checksum of a batch of
pages with the compressed bytes never leaving device memory.

The stored image of a page is seal(algo, key, nonce, compress(page)), or
compress(page) without a cipher; its object checksum is the CRC32C of header ||
image || tag.  Every expected value comes from the suite's checkers
(oracle.lz4_compress, tests.zstd_lib, oracle.seal / checksum / object_checksum,
tests.lz4_data), never from the engine."""
import ctypes

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import lz4_data, zstd_lib

pytestmark = pytest.mark.gpu

ALGOS = [E.AES256GCM, E.CHACHA20P1305, E.CIPHER_NONE]
CODECS = [E.CODEC_LZ4, E.CODEC_ZSTD]
MEMS = [E.MEM_HOST, E.MEM_DEVICE]
# tests/test_gpu_load.py's lengths: a segment edge, the codecs' minimum match
# and end-of-block rules, an AES / ChaCha tail, one multi-task block
LENGTHS = [0, 1, 13, 4095, 32767, 32768, 32769, 65536 + 5, 102400, 1 << 20, (4 << 20) - 1]
KINDS = ["text", "runs", "zeros", "random"]
SEED = 0x570E
HDR = bytes((7 * i + 3) & 0xFF for i in range(271))  # an object header: BE16(256) | 12 | wrapped key | nonce
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _compress(codec, plain):
    return orc.lz4_compress(plain) if codec == E.CODEC_LZ4 else zstd_lib.compress_simple(plain)


def _bound(codec, n):
    return int(E.lz4_bound(n) if codec == E.CODEC_LZ4 else E.zstd_bound(n))


def _orc_algo(algo):
    return orc.AES256GCM if algo == E.AES256GCM else orc.CHACHA20P1305


def _nseg(n):
    return max(1, -(-n // E.SEG))


def _image(algo, blk, comp, hdr=HDR):
    """(key, nonce, image, tag, object checksum) of a compressed block."""
    if algo == E.CIPHER_NONE:
        return None, None, bytes(comp), bytes(16), int(orc.object_checksum(hdr + bytes(comp), hw=True))
    key, nonce = orc.gen_key(SEED, blk)
    c, tag = orc.seal(_orc_algo(algo), key, nonce, comp, fast=True)
    c, tag = bytes(c), bytes(tag)
    return key, nonce, c, tag, int(orc.object_checksum(hdr + c + tag, hw=True))


_cache = {}


def _grid(codec):
    """(page, compressed, checksum) of every (kind, length), computed once."""
    if ("grid", codec) not in _cache:
        out = []
        for kind in KINDS:
            for n in LENGTHS:
                p = lz4_data.sample(kind, n, seed=7)
                out.append((p, _compress(codec, p), orc.checksum(p, hw=True)))
        _cache[("grid", codec)] = out
    return _cache[("grid", codec)]


def _images(codec, algo):
    if ("img", codec, algo) not in _cache:
        _cache[("img", codec, algo)] = [_image(algo, i, c) for i, (_, c, _) in enumerate(_grid(codec))]
    return _cache[("img", codec, algo)]


class Batch:
    """A batch of pages laid out in host or device memory.  dst of block i has
    dst_cap = the codec's bound and a GUARD behind it; dst and the CRC arrays
    are pre-filled with 0xA5 so that an untouched byte is caught."""

    def __init__(self, eng, codec, pages, keys, mem, crcs=None, hdr=HDR, src_skew=0, dst_skew=0):
        self.eng, self.codec, self.mem = eng, codec, mem
        self.lens = [len(p) for p in pages]
        self.caps = [_bound(codec, n) for n in self.lens]
        al = lambda x: (x + 31) & ~15  # noqa: E731  16-byte slots with room for a skew
        self.soff, self.doff, self.coff = [], [], []
        so = do = co = 0
        for ln, cap in zip(self.lens, self.caps):
            self.soff.append(so + src_skew)
            self.doff.append(do + dst_skew)
            self.coff.append(co)
            so += al(ln)
            do += al(cap + GUARD)
            co += 4 * _nseg(ln)
        src = np.zeros(max(so, 16), np.uint8)
        for p, o in zip(pages, self.soff):
            src[o:o + len(p)] = np.frombuffer(p, np.uint8)
        fill_d = np.full(max(do, 16), 0xA5, np.uint8)
        fill_c = np.full(max(co, 16), 0xA5, np.uint8)
        if crcs is not None:  # VERIFY: the arrays to check against
            for c, o in zip(crcs, self.coff):
                fill_c[o:o + len(c)] = np.frombuffer(c, np.uint8)
        self.crc_in = fill_c.copy()
        self.hdr = np.frombuffer(hdr, np.uint8).copy() if hdr else None
        if mem == E.MEM_DEVICE:
            self.sbuf, self.dbuf, self.cbuf = eng.alloc(src.size), eng.alloc(fill_d.size), eng.alloc(fill_c.size)
            self.sbuf.upload(src)
            self.dbuf.upload(fill_d)
            self.cbuf.upload(fill_c)
            sp, dp, cp = self.sbuf.ptr, self.dbuf.ptr, self.cbuf.ptr
        else:
            self.src, self.dst, self.cw = src, fill_d, fill_c
            sp, dp, cp = src.ctypes.data, self.dst.ctypes.data, self.cw.ctypes.data
        specs = []
        for i, ln in enumerate(self.lens):
            key, nonce = keys[i] if keys is not None else (None, None)
            specs.append({"key": key, "nonce": nonce, "src": sp + self.soff[i] if ln else None, "len": ln,
                          "dst": dp + self.doff[i], "dst_cap": self.caps[i], "crc": cp + self.coff[i],
                          "hdr": self.hdr.ctypes.data if self.hdr is not None else None,
                          "hdr_len": self.hdr.size if self.hdr is not None else 0})
        self.arr, self.n = eng.make_sblocks(specs)

    def fetch(self):
        if self.mem == E.MEM_DEVICE:
            self.dst, self.cw = self.dbuf.download(), self.cbuf.download()

    def run(self, algo, crc_mode):
        self.eng.store_batch(algo, self.codec, self.arr, self.n, crc_mode, self.mem)
        self.fetch()
        return self

    def image(self, i):
        return self.dst[self.doff[i]:self.doff[i] + self.arr[i].out_len].tobytes()

    def crcs(self, i):
        return self.cw[self.coff[i]:self.coff[i] + 4 * _nseg(self.lens[i])].tobytes()

    def dst_untouched(self, host_exact):
        """Host: every byte outside the blocks' dst[0, out_len) still holds 0xA5.
        Device: every byte outside dst[0, dst_cap) does (the compressor may use
        its capacity), and all of dst of a block that is not OK."""
        m = np.ones(self.dst.size, bool)
        for i in range(self.n):
            if self.arr[i].status != E.OK:
                continue
            m[self.doff[i]:self.doff[i] + (self.arr[i].out_len if host_exact else self.caps[i])] = False
        return bool((self.dst[m] == 0xA5).all())

    def crc_outside_untouched(self, written):
        m = np.ones(self.cw.size, bool)
        if written:
            for i, ln in enumerate(self.lens):
                m[self.coff[i]:self.coff[i] + 4 * _nseg(ln)] = False
        return bool((self.cw[m] == self.crc_in[m]).all())

    def free(self):
        if self.mem == E.MEM_DEVICE:
            for b in (self.sbuf, self.dbuf, self.cbuf):
                b.free()


# ---------------------------------------------------------------------------
# lengths and kinds: one batch of 44 pages per (codec, cipher, memory), GEN | CT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("algo", ALGOS, ids=["gcm", "chacha", "none"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_lengths_and_kinds(eng, codec, algo, mem):
    grid, want = _grid(codec), _images(codec, algo)
    assert any(len(c) > len(p) for p, c, _ in grid)  # random: the image is longer than the page
    host = mem == E.MEM_HOST
    # odd offsets where the rule allows: host anywhere; device never here (the
    # page CRC reads src, the Seal / the image CRC touch dst)
    b = Batch(eng, codec, [p for p, _, _ in grid], [(k, nn) for k, nn, _, _, _ in want] if algo != E.CIPHER_NONE
              else None, mem, src_skew=3 if host else 0, dst_skew=5 if host else 0)
    try:
        b.run(algo, E.CRC_GEN | E.CRC_CT)
        for i, ((p, _, crc), (_, _, img, tag, obj)) in enumerate(zip(grid, want)):
            tagd = (KINDS[i // len(LENGTHS)], len(p))
            s = b.arr[i]
            assert (s.status, s.out_len, s.crc_bad_seg, s.crc_got, s.crc_expect) == (E.OK, len(img), -1, 0, 0), tagd
            assert b.image(i) == img, tagd
            assert bytes(s.tag) == tag, tagd
            assert b.crcs(i) == crc, tagd
            assert s.obj_crc == obj, tagd
        assert b.dst_untouched(host_exact=host)
        assert b.crc_outside_untouched(written=True)
    finally:
        b.free()


# ---------------------------------------------------------------------------
# the staged upload: VERIFY, two pages whose CRC arrays do not match
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("algo", [E.AES256GCM, E.CIPHER_NONE], ids=["gcm", "none"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_staged_upload_verify(eng, codec, algo, mem):
    shapes = [("text", 70001), ("runs", 32768), ("text", 200001), ("random", 40000), ("zeros", 1), ("text", 20000),
              ("text", 0), ("runs", 131072)]
    pages = [lz4_data.sample(k, n, seed=80 + i) for i, (k, n) in enumerate(shapes)]
    good = [orc.checksum(p, hw=True) for p in pages]
    crcs = [bytearray(c) for c in good]
    # block 2: 7 segments, the last one's word flipped; block 5: one segment (<= 32 KiB), its only word
    bad = {2: _nseg(200001) - 1, 5: 0}
    assert bad[2] == 6 and len(pages[5]) <= E.SEG
    for i, seg in bad.items():
        crcs[i][4 * seg + 1] ^= 0x20
    want = [_image(algo, 500 + i, _compress(codec, p)) for i, p in enumerate(pages)]
    keys = [(k, nn) for k, nn, _, _, _ in want] if algo != E.CIPHER_NONE else None
    b = Batch(eng, codec, pages, keys, mem, crcs=[bytes(c) for c in crcs])
    m0 = eng.metrics()
    try:
        b.run(algo, E.CRC_VERIFY | E.CRC_CT)
        m1 = eng.metrics()
        for i, (_, _, img, tag, obj) in enumerate(want):
            s = b.arr[i]
            if i in bad:
                seg = bad[i]
                assert (s.status, s.out_len, s.crc_bad_seg) == (E.ECRC, 0, seg), i
                assert s.crc_got == int.from_bytes(good[i][4 * seg:4 * seg + 4], "big"), i
                assert s.crc_expect == int.from_bytes(crcs[i][4 * seg:4 * seg + 4], "big"), i
                assert bytes(s.tag) == bytes(16) and s.obj_crc == 0, i
                d0 = b.doff[i]
                assert (b.dst[d0:d0 + b.caps[i] + GUARD] == 0xA5).all(), i  # all of dst_cap, and the guard
            else:
                assert (s.status, s.out_len, s.crc_bad_seg, s.crc_got, s.crc_expect) == (E.OK, len(img), -1, 0, 0), i
                assert b.image(i) == img and bytes(s.tag) == tag and s.obj_crc == obj, i
        assert b.dst_untouched(host_exact=mem == E.MEM_HOST)
        assert (b.cw == b.crc_in).all()  # VERIFY reads the arrays
        d = {k: m1[k] - m0[k] for k in m0 if isinstance(m0[k], int)}
        cb = "lz4c_blocks" if codec == E.CODEC_LZ4 else "zstdc_blocks"
        assert d["crc_fail"] == 2 and d[cb] == 6
        ok = [i for i in range(8) if i not in bad]
        assert d[cb.replace("blocks", "in")] == sum(len(pages[i]) for i in ok)
        assert d[cb.replace("blocks", "out")] == sum(len(want[i][2]) for i in ok)
        if algo != E.CIPHER_NONE:
            assert d["seal_blocks"] == 6 and d["seal_batches"] == 1
            assert d["seal_bytes"] == sum(len(want[i][2]) for i in ok)
            assert (d["crc_batches"], d["crc_ranges"], d["crc_bytes"]) == (1, 8, sum(len(p) for p in pages))
        else:
            assert d["seal_blocks"] == 0
            # the image CRC launch that JFSX_CRC_CT adds counts as jfsx_crc32c_segments would
            assert (d["crc_batches"], d["crc_ranges"]) == (2, 8 + 6)
            assert d["crc_bytes"] == sum(len(p) for p in pages) + sum(len(want[i][2]) for i in ok)
        other = "zstdc_blocks" if codec == E.CODEC_LZ4 else "lz4c_blocks"
        assert d[other] == 0 and d["open_blocks"] == 0
    finally:
        b.free()


# ---------------------------------------------------------------------------
# the same inputs through the separate calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [E.AES256GCM, E.CHACHA20P1305], ids=["gcm", "chacha"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_equals_separate_calls(eng, codec, algo):
    rng = np.random.default_rng(17)
    lens = [int(x) for x in rng.integers(1, 300000, 16)]
    pages = [lz4_data.sample(lz4_data.KINDS[i % len(lz4_data.KINDS)], n, seed=300 + i) for i, n in enumerate(lens)]
    keys = [orc.gen_key(SEED, 700 + i) for i in range(16)]
    # compress_batch, then seal_batch(GEN | CT) on its output with jfsx_object_crc32c, then crc32c_segments
    comps = eng.lz4_compress(pages) if codec == E.CODEC_LZ4 else eng.zstd_compress(pages)
    srcs = [np.frombuffer(c, np.uint8).copy() for c in comps]
    outs = [np.zeros(s.size, np.uint8) for s in srcs]
    segs = [np.zeros(4 * _nseg(s.size), np.uint8) for s in srcs]
    arr, n = eng.make_blocks([{"key": k, "nonce": nn, "src": s.ctypes.data, "dst": o.ctypes.data, "len": s.size,
                               "crc": g.ctypes.data} for (k, nn), s, o, g in zip(keys, srcs, outs, segs)])
    eng.seal_batch(algo, arr, n, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
    seq = []
    for i in range(16):
        tag = bytes(arr[i].tag)
        seq.append((outs[i].tobytes(), tag, eng.object_crc32c(HDR, segs[i], srcs[i].size, tag),
                    eng.checksum(pages[i])))
    # one call
    got = eng.store(algo, codec, [(k, nn, p) for (k, nn), p in zip(keys, pages)], crc=True, headers=[HDR] * 16)
    for i, ((st, img, tag, crc, obj), (img2, tag2, obj2, crc2)) in enumerate(zip(got, seq)):
        assert st == E.OK, i
        assert (img, tag, obj, crc) == (img2, tag2, obj2, crc2), i
        # and both are what the checkers say
        assert _image(algo, 700 + i, _compress(codec, pages[i]))[2:] == (img, tag, obj), i


# ---------------------------------------------------------------------------
# round trip through jfsx_load_batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS, ids=["gcm", "chacha", "none"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_round_trip_through_load_batch(eng, codec, algo):
    pages = [lz4_data.sample(k, n, seed=90 + i) for i, (k, n) in
             enumerate([("text", 1 << 20), ("random", 70000), ("zeros", 32768), ("runs", 12345), ("text", 5),
                        ("text", 0)])]
    keys = [orc.gen_key(SEED, 900 + i) for i in range(len(pages))]
    items = pages if algo == E.CIPHER_NONE else [(k, nn, p) for (k, nn), p in zip(keys, pages)]
    stored = eng.store(algo, codec, items, crc=True)
    assert [s[0] for s in stored] == [E.OK] * len(pages)
    imgs = [s[1] if algo == E.CIPHER_NONE else (k, nn, s[1], s[2]) for s, (k, nn) in zip(stored, keys)]
    back = eng.load(algo, codec, imgs, [len(p) for p in pages], crc=True)
    for i, ((st, page, crc), p) in enumerate(zip(back, pages)):
        assert st == E.OK and page == p, i
        assert crc == stored[i][3] == orc.checksum(p, hw=True), i


# ---------------------------------------------------------------------------
# CRC_NONE; CRC_CT alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("mode", [E.CRC_NONE, E.CRC_CT], ids=["none", "ct"])
@pytest.mark.parametrize("algo", [E.CHACHA20P1305, E.CIPHER_NONE], ids=["chacha", "none"])
def test_crc_none_and_ct_alone(eng, algo, mode, mem):
    codec = E.CODEC_LZ4
    pages = [lz4_data.sample("text", n, seed=60) for n in (40000, 100001, 0)]
    want = [_image(algo, 40 + i, _compress(codec, p)) for i, p in enumerate(pages)]
    keys = [(k, nn) for k, nn, _, _, _ in want] if algo != E.CIPHER_NONE else None
    # no page CRC: src may sit at any alignment in device memory too; without a
    # cipher or CT nothing but the compressor touches dst
    free_dst = algo == E.CIPHER_NONE and mode == E.CRC_NONE
    b = Batch(eng, codec, pages, keys, mem, src_skew=1, dst_skew=7 if mem == E.MEM_HOST or free_dst else 0)
    try:
        b.run(algo, mode)
        for i, (_, _, img, tag, obj) in enumerate(want):
            s = b.arr[i]
            assert (s.status, s.out_len) == (E.OK, len(img)) and b.image(i) == img and bytes(s.tag) == tag, i
            assert s.obj_crc == (obj if mode == E.CRC_CT else 0), i
        assert (b.cw == 0xA5).all()
        assert b.dst_untouched(host_exact=mem == E.MEM_HOST)
    finally:
        b.free()


# ---------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------
def test_argument_errors_write_nothing(eng):
    page = lz4_data.sample("text", 5000, seed=61)
    key = orc.gen_key(SEED, 0)

    def fresh(mem=E.MEM_HOST):
        b = Batch(eng, E.CODEC_LZ4, [page], [key], mem)
        b.arr[0].status, b.arr[0].out_len, b.arr[0].obj_crc = 77, 78, 79
        return b

    def untouched(b):
        b.fetch()
        return (b.arr[0].status, b.arr[0].out_len, b.arr[0].obj_crc) == (77, 78, 79) and \
            bytes(b.arr[0].tag) == bytes(16) and bool((b.dst == 0xA5).all() and (b.cw == 0xA5).all())

    L = eng.L
    mode = E.CRC_GEN | E.CRC_CT

    def call(b, codec=E.CODEC_LZ4, mem=None):
        return L.jfsx_store_batch(eng.ctx, E.AES256GCM, codec, 1, b.arr, mode, b.mem if mem is None else mem)

    for codec in CODECS:  # dst_cap one below the codec's bound
        b = fresh()
        b.arr[0].dst_cap = _bound(codec, 5000) - 1
        assert call(b, codec) == E.EINVAL and untouched(b)
        b.arr[0].dst_cap = _bound(codec, 5000)
    b = fresh()
    b.arr[0].reserved = 1
    assert call(b) == E.EINVAL and untouched(b)
    b = fresh(E.MEM_DEVICE)
    try:
        b.arr[0].dst = b.dbuf.ptr + 8  # a cipher writes dst: 16-byte aligned
        assert call(b) == E.EINVAL and untouched(b)
        b.arr[0].dst = b.arr[0].src  # the compressors do not run in place
        assert call(b) == E.EINVAL and untouched(b)
        b.arr[0].dst = b.dbuf.ptr
        b.arr[0].src = b.sbuf.ptr + 4  # the page CRC reads src: 16-byte aligned
        assert call(b) == E.EINVAL and untouched(b)
    finally:
        b.free()
    # n == 0 is a no-op
    assert L.jfsx_store_batch(eng.ctx, E.AES256GCM, E.CODEC_LZ4, 0, None, mode, E.MEM_HOST) == 0


# ---------------------------------------------------------------------------
# compress.upload_blocks_fused against compress.upload_blocks
# ---------------------------------------------------------------------------
class _Stream:
    """A repeatable rand for DataEncryptor: the bytes of a seeded generator."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("cipher", [None, "aes256gcm-rsa", "chacha20-rsa"], ids=["plain", "gcm", "chacha"])
@pytest.mark.parametrize("name", ["lz4", "zstd"])
def test_upload_blocks_fused_mirrors_upload_blocks(eng, name, cipher):
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as EN
    comp = C.NewCompressor(name, eng)
    codec = E.CODEC_LZ4 if name == "lz4" else E.CODEC_ZSTD
    blocks = [lz4_data.sample(k, n, seed=70 + i) for i, (k, n) in
              enumerate([("text", 1 << 20), ("random", 70000), ("zeros", 32768), ("runs", 12345), ("text", 5)])]
    keys = ["chunks/0/0/%d_0_%d" % (i, len(b)) for i, b in enumerate(blocks)]
    lens = [len(b) for b in blocks]
    rsa = EN.NewRSAEncryptor(EN.GenerateRsaKey(2048)) if cipher else None

    def encryptor(seed):
        return EN.DataEncryptor(rsa, EN.NewDataEncryptor(rsa, cipher, eng).algo, eng, rand=_Stream(seed)) \
            if cipher else None

    raw, raw2 = EN.MemStorage(), EN.MemStorage()
    enc = encryptor(5)
    objs, crcs = C.upload_blocks_fused(raw, keys, blocks, comp, enc=enc)
    assert crcs == [orc.checksum(b, hw=True) for b in blocks]
    assert [raw.Get(k) for k in keys] == objs
    assert C.upload_blocks_fused(EN.MemStorage(), keys, blocks, comp, enc=encryptor(5), checksums=False) is not None
    # read back by the existing loaders
    store = EN.NewEncrypted(raw, enc) if enc else raw
    assert C.load_blocks(store, keys, lens, comp) == blocks
    pages, crcs2 = C.load_blocks_fused(raw, keys, lens, comp, enc=enc)
    assert pages == blocks and crcs2 == crcs
    # the same rand stream through upload_blocks: the same C || tag behind the
    # header (the wrapped key differs: OAEP is randomised)
    enc2 = encryptor(5)
    C.upload_blocks(EN.NewEncrypted(raw2, enc2) if enc2 else raw2, keys, blocks, comp)
    for k, b in zip(keys, blocks):
        a, c = raw.Get(k), raw2.Get(k)
        if not cipher:
            assert a == c == _compress(codec, b), k
            continue
        hl = 3 + ((a[0] << 8) | a[1]) + a[2]
        assert len(a) == len(c) and a[:3] == c[:3] and a[hl - 12:] == c[hl - 12:], k  # nonce, C, tag
        assert len(a) == hl + len(_compress(codec, b)) + 16, k
