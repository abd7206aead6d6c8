"""GPU tests of the one-call block load (jfsx_load_batch): Open, decompress
and checksum() of a batch of stored block images with every intermediate in
device memory.

A stored image is seal(algo, key, nonce, compress(plain)); the expected page is
plain and the expected CRC array oracle.checksum(plain).  Every expected value
comes from the suite's checkers (oracle.seal / checksum / lz4_compress /
lz4_decompress, tests.zstd_lib, tests.lz4_data), never from the engine."""
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
# a segment edge (32767..32769), the codecs' minimum match and end-of-block
# rules (0, 1, 13), an AES / ChaCha tail (4095, 65536 + 5, 4 MiB - 1), one
# multi-task block (4 MiB - 1; 1 MiB)
LENGTHS = [0, 1, 13, 4095, 32767, 32768, 32769, 65536 + 5, 102400, 1 << 20, (4 << 20) - 1]
KINDS = ["text", "runs", "zeros", "random"]
SEED = 0x10AD


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _compress(codec, plain):
    return orc.lz4_compress(plain) if codec == E.CODEC_LZ4 else zstd_lib.compress_simple(plain)


def _orc_algo(algo):
    return orc.AES256GCM if algo == E.AES256GCM else orc.CHACHA20P1305


def _store(algo, blk, comp):
    """The stored image of a compressed block: (key, nonce, C, tag), or comp itself."""
    if algo == E.CIPHER_NONE:
        return (None, None, comp, None)
    key, nonce = orc.gen_key(SEED, blk)
    c, tag = orc.seal(_orc_algo(algo), key, nonce, comp, fast=True)
    return (key, nonce, c, tag)


_cache = {}


def _grid(codec):
    """(plain, compressed, checksum) of every (kind, length), computed once."""
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
        _cache[("img", codec, algo)] = [_store(algo, i, c) for i, (_, c, _) in enumerate(_grid(codec))]
    return _cache[("img", codec, algo)]


def _nseg(n):
    return max(1, -(-n // E.SEG))


class Batch:
    """A batch laid out in host or device memory, pages and CRC arrays
    pre-filled with 0xA5 so that an untouched byte is caught."""

    def __init__(self, eng, algo, images, lengths, mem, crc=True, src_skew=0, dst_skew=0):
        self.eng, self.mem, self.lengths, self.crc = eng, mem, [int(n) for n in lengths], crc
        n = len(images)
        al = lambda x: (x + 31) & ~15  # noqa: E731  16-byte slots with room for a skew
        self.soff, self.doff, self.coff = [], [], []
        so = do = co = 0
        for (_, _, c, _), ln in zip(images, self.lengths):
            self.soff.append(so + src_skew)
            self.doff.append(do + dst_skew)
            self.coff.append(co)
            so += al(len(c))
            do += al(ln)
            co += 4 * _nseg(ln)
        src = np.zeros(max(so, 16), np.uint8)
        for (_, _, c, _), o in zip(images, self.soff):
            src[o:o + len(c)] = np.frombuffer(c, np.uint8)
        self.fill_d = np.full(max(do, 16), 0xA5, np.uint8)
        self.fill_c = np.full(max(co, 16), 0xA5, np.uint8)
        if mem == E.MEM_DEVICE:
            self.sbuf, self.dbuf, self.cbuf = eng.alloc(src.size), eng.alloc(self.fill_d.size), eng.alloc(self.fill_c.size)
            self.sbuf.upload(src)
            self.dbuf.upload(self.fill_d)
            self.cbuf.upload(self.fill_c)
            sp, dp, cp = self.sbuf.ptr, self.dbuf.ptr, self.cbuf.ptr
        else:
            self.src, self.dst, self.cw = src, self.fill_d.copy(), self.fill_c.copy()
            sp, dp, cp = src.ctypes.data, self.dst.ctypes.data, self.cw.ctypes.data
        specs = []
        for i, (key, nonce, c, tag) in enumerate(images):
            specs.append({"key": key, "nonce": nonce, "tag": tag, "src": sp + self.soff[i] if len(c) else None,
                          "src_len": len(c), "dst": dp + self.doff[i] if self.lengths[i] else None,
                          "len": self.lengths[i], "crc": cp + self.coff[i]})
        self.arr, self.n = eng.make_lblocks(specs)

    def run(self, algo, codec):
        self.eng.load_batch(algo, codec, self.arr, self.n, E.CRC_GEN if self.crc else E.CRC_NONE, self.mem)
        if self.mem == E.MEM_DEVICE:
            self.dst, self.cw = self.dbuf.download(), self.cbuf.download()
        return self

    def page(self, i):
        return self.dst[self.doff[i]:self.doff[i] + self.lengths[i]].tobytes()

    def crcs(self, i):
        return self.cw[self.coff[i]:self.coff[i] + 4 * _nseg(self.lengths[i])].tobytes()

    def outside_untouched(self):
        """Every byte of the page and CRC buffers outside the blocks' ranges still holds 0xA5."""
        md, mc = np.ones(self.dst.size, bool), np.ones(self.cw.size, bool)
        for i, ln in enumerate(self.lengths):
            md[self.doff[i]:self.doff[i] + ln] = False
            if self.crc:
                mc[self.coff[i]:self.coff[i] + 4 * _nseg(ln)] = False
        return bool((self.dst[md] == 0xA5).all() and (self.cw[mc] == 0xA5).all())

    def free(self):
        if self.mem == E.MEM_DEVICE:
            for b in (self.sbuf, self.dbuf, self.cbuf):
                b.free()


# ---------------------------------------------------------------------------
# lengths: one batch of 44 blocks per (codec, cipher, memory)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("algo", ALGOS, ids=["gcm", "chacha", "none"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_lengths_and_kinds(eng, codec, algo, mem):
    grid, images = _grid(codec), _images(codec, algo)
    assert any(len(c) > len(p) for p, c, _ in grid)  # random: src_len > len
    # odd offsets where the rule allows: host anywhere; device src with no
    # cipher (Open reads 16-byte aligned images), dst never (the CRC pass reads it)
    src_skew = 3 if mem == E.MEM_HOST or algo == E.CIPHER_NONE else 0
    dst_skew = 5 if mem == E.MEM_HOST else 0
    b = Batch(eng, algo, images, [len(p) for p, _, _ in grid], mem, src_skew=src_skew, dst_skew=dst_skew)
    try:
        b.run(algo, codec)
        for i, (p, _, crc) in enumerate(grid):
            tagd = (KINDS[i // len(LENGTHS)], len(p))
            assert b.arr[i].status == E.OK and b.arr[i].out_len == len(p), tagd
            assert b.page(i) == p, tagd
            assert b.crcs(i) == crc, tagd
        assert b.outside_untouched()
    finally:
        b.free()


# ---------------------------------------------------------------------------
# a batch whose blocks fail in every way the table names
# ---------------------------------------------------------------------------
def _mixed(codec, algo):
    L = 70001
    lz4 = codec == E.CODEC_LZ4
    plain = [lz4_data.sample(k, L, seed=40 + i) for i, k in enumerate(["text", "runs", "text", "text", "random"])]
    garbage = lz4_data.sample("random", 5000, seed=99)
    short, long_ = lz4_data.sample("text", L - 7, seed=50), lz4_data.sample("text", L + 9, seed=51)
    comps = [_compress(codec, plain[0]), _compress(codec, plain[1]), _compress(codec, plain[2]), garbage,
             _compress(codec, short), _compress(codec, long_), _compress(codec, plain[3])[:-1],
             _compress(codec, plain[4])]
    images = [_store(algo, 100 + i, c) for i, c in enumerate(comps)]
    if algo != E.CIPHER_NONE:  # a flipped tag bit over a valid compressed image
        key, nonce, c, tag = images[2]
        images[2] = (key, nonce, c, bytes([tag[0] ^ 0x10]) + tag[1:])
    # what the checkers say of each image, decoded into L bytes
    want = []
    for i, c in enumerate(comps):
        if i == 2 and algo != E.CIPHER_NONE:
            want.append((E.ETAG, 0, None))
            continue
        if lz4:
            r, d = orc.lz4_decompress(c, L)
        else:
            r, d = zstd_lib.decompress(c, L)
        if r < 0:
            # the zstd library reports one error code here; the frame that is
            # well formed but larger than the page is the table's EDSTSIZE
            want.append((E.EDSTSIZE if (not lz4 and i == 5) else E.EFORMAT, 0, None))
        elif r < L:
            want.append((E.ESHORT, r, None))
        else:
            want.append((E.OK, L, d))
    return L, images, want, plain


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("algo", ALGOS, ids=["gcm", "chacha", "none"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_mixed_fate_batch(eng, codec, algo, mem):
    L, images, want, plain = _mixed(codec, algo)
    lz4 = codec == E.CODEC_LZ4
    # the construction gives the fates the table names
    assert [w[0] for w in want] == [E.OK, E.OK, E.OK if algo == E.CIPHER_NONE else E.ETAG, E.EFORMAT, E.ESHORT,
                                    E.EFORMAT if lz4 else E.EDSTSIZE, E.EFORMAT, E.OK]
    assert want[4][1] == L - 7 and want[0][2] == plain[0] and want[7][2] == plain[4]
    b = Batch(eng, algo, images, [L] * 8, mem)
    m0 = eng.metrics()
    try:
        b.run(algo, codec)
        m1 = eng.metrics()
        for i, (st, out_len, page) in enumerate(want):
            assert (b.arr[i].status, b.arr[i].out_len) == (st, out_len), i
            if st == E.OK:
                assert b.page(i) == page, i
                assert b.crcs(i) == orc.checksum(page, hw=True), i
            else:
                assert b.page(i) == bytes(L), i
                assert b.crcs(i) == bytes(4 * _nseg(L)), i
        assert b.outside_untouched()
        reached = sum(1 for w in want if w[0] != E.ETAG)
        key = "lz4d_blocks" if lz4 else "zstdd_blocks"
        assert m1[key] - m0[key] == reached
        assert m1["lz4d_fail" if lz4 else "zstdd_fail"] - m0["lz4d_fail" if lz4 else "zstdd_fail"] == \
            sum(1 for w in want if w[0] in (E.EFORMAT, E.EDSTSIZE))
        if algo != E.CIPHER_NONE:
            assert m1["open_blocks"] - m0["open_blocks"] == 8 and m1["open_fail"] - m0["open_fail"] == 1
        else:
            assert m1["open_blocks"] == m0["open_blocks"]
        assert m1["crc_ranges"] - m0["crc_ranges"] == 8
    finally:
        b.free()


# ---------------------------------------------------------------------------
# the same inputs through the three existing calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [E.AES256GCM, E.CHACHA20P1305], ids=["gcm", "chacha"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_equals_three_calls(eng, codec, algo):
    rng = np.random.default_rng(16)
    lens = [int(x) for x in rng.integers(1, 300000, 16)]
    plains = [lz4_data.sample(lz4_data.KINDS[i % len(lz4_data.KINDS)], n, seed=200 + i) for i, n in enumerate(lens)]
    comps = [_compress(codec, p) for p in plains]
    comps[9] = comps[9][:-1]
    images = [_store(algo, 300 + i, c) for i, c in enumerate(comps)]
    key, nonce, c, tag = images[5]
    images[5] = (key, nonce, c, tag[:15] + bytes([tag[15] ^ 1]))
    # three calls: open_batch, the decoder on what opened, checksum of what decoded in full
    srcs = [np.frombuffer(c, np.uint8).copy() for _, _, c, _ in images]
    outs = [np.zeros(max(s.size, 1), np.uint8) for s in srcs]
    arr, n = eng.make_blocks([{"key": k, "nonce": nn, "src": s.ctypes.data, "dst": o.ctypes.data, "len": s.size,
                               "tag": t} for (k, nn, _, t), s, o in zip(images, srcs, outs)])
    eng.open_batch(algo, arr, n, E.CRC_NONE, E.MEM_HOST)
    ok = [i for i in range(16) if arr[i].status == E.OK]
    dec = eng.lz4_decompress if codec == E.CODEC_LZ4 else eng.zstd_decompress
    res = dict(zip(ok, dec([outs[i][:srcs[i].size] for i in ok], [lens[i] for i in ok])))
    seq = []
    for i in range(16):
        if i not in res:
            seq.append((E.ETAG, None, None))
        elif res[i][0] != E.OK:
            seq.append((res[i][0], None, None))
        elif len(res[i][1]) < lens[i]:
            seq.append((E.ESHORT, None, None))
        else:
            seq.append((E.OK, res[i][1], eng.checksum(res[i][1])))
    assert [s[0] for s in seq].count(E.OK) == 14 and seq[5][0] == E.ETAG and seq[9][0] == E.EFORMAT
    # one call
    got = eng.load(algo, codec, images, lens, crc=True)
    for i, ((st, page, crc), (st2, page2, crc2)) in enumerate(zip(got, seq)):
        assert st == st2, i
        if st == E.OK:
            assert page == page2 == plains[i] and crc == crc2, i
        else:
            assert page == bytes(lens[i]) and crc == bytes(4 * _nseg(lens[i])), i


# ---------------------------------------------------------------------------
# CRC_NONE; argument errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=["lz4", "zstd"])
def test_crc_none_leaves_crc_untouched(eng, codec, mem):
    plains = [lz4_data.sample("text", n, seed=60) for n in (40000, 100001)]
    comps = [_compress(codec, p) for p in plains]
    comps.append(comps[1][:-2])  # a failed block: its page is wiped, its CRC array still untouched
    images = [_store(E.CIPHER_NONE, 0, c) for c in comps]
    # without a CRC pass the page may sit at any alignment in device memory too
    b = Batch(eng, E.CIPHER_NONE, images, [40000, 100001, 100001], mem, crc=False, src_skew=1, dst_skew=7)
    try:
        b.run(E.CIPHER_NONE, codec)
        assert [b.arr[i].status for i in range(3)] == [E.OK, E.OK, E.EFORMAT]
        assert b.page(0) == plains[0] and b.page(1) == plains[1] and b.page(2) == bytes(100001)
        assert (b.cw == 0xA5).all()
        assert b.outside_untouched()
    finally:
        b.free()


def test_argument_errors_write_nothing(eng):
    p = lz4_data.sample("text", 5000, seed=61)
    img = _store(E.AES256GCM, 0, orc.lz4_compress(p))

    def fresh(mem=E.MEM_HOST):
        b = Batch(eng, E.AES256GCM, [img], [5000], mem)
        b.arr[0].status, b.arr[0].out_len, b.arr[0].codec_info = 77, 78, 79
        return b

    def untouched(b):
        if b.mem == E.MEM_DEVICE:
            b.dst, b.cw = b.dbuf.download(), b.cbuf.download()
        return (b.arr[0].status, b.arr[0].out_len, b.arr[0].codec_info) == (77, 78, 79) and \
            bool((b.dst == 0xA5).all() and (b.cw == 0xA5).all())

    L = eng.L
    for algo, codec in ((E.AES256GCM, 0), (E.AES256GCM, 3), (2, E.CODEC_LZ4), (-2, E.CODEC_ZSTD)):
        b = fresh()
        assert L.jfsx_load_batch(eng.ctx, algo, codec, 1, b.arr, E.CRC_GEN, E.MEM_HOST) == E.EINVAL
        assert untouched(b)
    for crc_mode, mem in ((E.CRC_VERIFY, E.MEM_HOST), (E.CRC_GEN | E.CRC_CT, E.MEM_HOST), (E.CRC_GEN, 2)):
        b = fresh()
        assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_LZ4, 1, b.arr, crc_mode, mem) == E.EINVAL
        assert untouched(b)
    # zstd pages are addressed with 32-bit frame positions
    b = fresh()
    b.arr[0].len = 1 << 31
    assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_ZSTD, 1, b.arr, E.CRC_GEN, E.MEM_HOST) == E.EINVAL
    assert untouched(b)
    b.arr[0].len = (1 << 31) - 1
    b.arr[0].src_len = 0x7E000001
    assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_ZSTD, 1, b.arr, E.CRC_GEN, E.MEM_HOST) == E.EINVAL
    assert untouched(b)
    # device memory: the decoders do not run in place; Open reads aligned images
    b = fresh(E.MEM_DEVICE)
    try:
        b.arr[0].dst = b.arr[0].src
        assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_LZ4, 1, b.arr, E.CRC_GEN, E.MEM_DEVICE) == E.EINVAL
        b.arr[0].dst = b.dbuf.ptr
        b.arr[0].src = b.sbuf.ptr + 1
        assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_LZ4, 1, b.arr, E.CRC_GEN, E.MEM_DEVICE) == E.EINVAL
        assert untouched(b)
    finally:
        b.free()
    # n == 0 is a no-op
    assert L.jfsx_load_batch(eng.ctx, E.AES256GCM, E.CODEC_LZ4, 0, None, E.CRC_GEN, E.MEM_HOST) == 0


# ---------------------------------------------------------------------------
# compress.load_blocks_fused against compress.load_blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cipher", [None, "aes256gcm-rsa", "chacha20-rsa"], ids=["plain", "gcm", "chacha"])
@pytest.mark.parametrize("name", ["lz4", "zstd"])
def test_load_blocks_fused_mirrors_load_blocks(eng, name, cipher):
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as EN
    comp = C.NewCompressor(name, eng)
    raw = EN.MemStorage()
    enc = EN.NewDataEncryptor(EN.NewRSAEncryptor(EN.GenerateRsaKey(2048)), cipher, eng) if cipher else None
    store = EN.NewEncrypted(raw, enc) if enc else raw
    blocks = [lz4_data.sample(k, n, seed=70 + i) for i, (k, n) in
              enumerate([("text", 1 << 20), ("random", 70000), ("zeros", 32768), ("runs", 12345), ("text", 5)])]
    keys = ["chunks/0/0/%d_0_%d" % (i, len(b)) for i, b in enumerate(blocks)]
    lens = [len(b) for b in blocks]
    for k, b in zip(keys, blocks):
        store.Put(k, _compress(E.CODEC_LZ4 if name == "lz4" else E.CODEC_ZSTD, b))
    want = C.load_blocks(store, keys, lens, comp)
    assert want == blocks
    pages, crcs = C.load_blocks_fused(raw, keys, lens, comp, enc=enc)
    assert pages == want
    assert crcs == [orc.checksum(b, hw=True) for b in blocks]
    assert C.load_blocks_fused(raw, keys, lens, comp, enc=enc, checksums=False) == want

    def message(fn):
        with pytest.raises((C.CompressError, EN.EncryptError)) as ei:
            fn()
        return type(ei.value), str(ei.value)

    # a block whose object decodes short of its length
    store.Put(keys[3], _compress(E.CODEC_LZ4 if name == "lz4" else E.CODEC_ZSTD, blocks[3][:-1]))
    a = message(lambda: C.load_blocks(store, keys, lens, comp))
    assert a == message(lambda: C.load_blocks_fused(raw, keys, lens, comp, enc=enc))
    assert a == (C.CompressError, "read %s fully: None (12344 < 12345)" % keys[3])
    # a corrupted object: with a cipher one flipped byte of the stored bytes (the
    # tag no longer verifies); without one, an image cut short (a flipped
    # literal byte would decode, to other bytes)
    obj = bytearray(raw.Get(keys[1]))
    if enc:
        obj[len(obj) // 2] ^= 0x40
    else:
        del obj[-3:]
    raw.Put(keys[1], bytes(obj))
    a = message(lambda: C.load_blocks(store, keys[:3], lens[:3], comp))
    assert a == message(lambda: C.load_blocks_fused(raw, keys[:3], lens[:3], comp, enc=enc))
    if enc:
        assert a[0] is EN.EncryptError and "message authentication failed" in a[1]
    else:
        assert a == (C.CompressError, "read %s fully: %s (0 < 70000)"
                     % (keys[1], "lz4: malformed block" if name == "lz4" else "zstd: corrupted frame"))
    # an empty object
    if not enc:
        raw.Put(keys[0], b"")
        a = message(lambda: C.load_blocks(store, keys[:1], lens[:1], comp))
        assert a == message(lambda: C.load_blocks_fused(raw, keys[:1], lens[:1], comp))
        assert ("decompress an empty input" if name == "lz4" else "Bytes slice is empty") in a[1]
