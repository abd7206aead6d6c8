"""GPU tests of the one-call object store (jfsx_store_objects): the data-key
wrap, the page's verify or checksum(), compress, Seal, the object's header and
tag, and the object checksum of a batch of pages, with nothing assembled or
folded on the host.

A stored object is BE16(256) | 12 | wrapped key | nonce | seal(compress(page))
| tag.  No expected value comes from the engine: the wrapped key is
tests/rsa_model.py's oaep_encode + encrypt_em on the fixed keys of
tests/golden/rsa_keys.json, the compressed bytes are oracle.lz4_compress or
tests.zstd_lib.compress_simple, C and the tag are oracle.seal, the checksums
oracle.checksum and oracle.object_checksum."""
import functools

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import lz4_data, zstd_lib
from tests import rsa_model as M

pytestmark = pytest.mark.gpu

CIPHERS = [E.AES256GCM, E.CHACHA20P1305]
CODECS = [E.CODEC_NONE, E.CODEC_LZ4, E.CODEC_ZSTD]
MEMS = [E.MEM_HOST, E.MEM_DEVICE]
CODEC_IDS = ["none", "lz4", "zstd"]
LENGTHS = [0, 1, 13, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 5, 102400, 1 << 20]
KINDS = ["text", "runs", "zeros", "random"]
SEED = 0x50B
KEY_A, KEY_B = "plain_p_gt_q", "wide_q_gt_p"
HDR, TAG = 271, 16
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dkeys(eng):
    """Both fixed RSA keys on the device for the whole module: two keys alive at once."""
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
def wrap(name, key, seed, e=M.E):
    k = M.fixed_keys()[name]
    if e == M.E:
        return M.ct256(M.encrypt_em(k, M.oaep_encode(key, seed)))
    return M.ct256(pow(int.from_bytes(M.oaep_encode(key, seed), "big"), e, k.n))


def draw(blk):
    """(data key, seed, nonce) of block blk; keys repeat every 8 blocks, nonces and seeds do not."""
    key, _ = orc.gen_key(SEED, blk % 8)
    _, nonce = orc.gen_key(SEED, blk)
    return bytes(key), M.det_bytes(32, "sobj seed", blk), bytes(nonce)


@functools.lru_cache(maxsize=None)
def expected(algo, codec, name, blk, page, e=M.E):
    """(object, img_len, page crcs, obj_crc) of one page from the checkers alone."""
    key, seed, nonce = draw(blk)
    c, tag = orc.seal(_orc_algo(algo), key, nonce, _compress(codec, page), fast=True)
    obj = bytes([1, 0, 12]) + wrap(name, key, seed, e) + nonce + bytes(c) + bytes(tag)
    return obj, len(c), bytes(orc.checksum(page, hw=True)), int(orc.object_checksum(obj, hw=True))


class SBatch:
    """A batch laid out in host or device memory.  Object buffers (obj_cap =
    the bound exactly, a guard behind each) and CRC arrays are pre-filled with
    0xA5.  Device objects start 1 mod 16; host pages and objects at odd
    offsets."""

    def __init__(self, eng, codec, pages, blks, mem, crcs=None, obj_mod=1, with_crc=True):
        self.eng, self.mem, self.codec, self.pages = eng, mem, codec, [bytes(p) for p in pages]
        dev = mem == E.MEM_DEVICE
        self.caps = [_bound(codec, len(p)) for p in self.pages]
        self.poff, self.ooff, self.coff = [], [], []
        po = oo = co = 0
        for p, cap in zip(self.pages, self.caps):
            self.poff.append(po + (0 if dev else 3))
            self.ooff.append(oo + (obj_mod if dev else 5))
            self.coff.append(co)
            po += (len(p) + 31) & ~15
            oo += (cap + GUARD + 47) & ~15
            co += 4 * _nseg(len(p))
        src = np.zeros(max(po, 16), np.uint8)
        for p, o in zip(self.pages, self.poff):
            src[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.fill_o = np.full(oo + 16, 0xA5, np.uint8)
        self.crc_end = co
        self.crc_in = np.full(co + GUARD, 0xA5, np.uint8)  # a guard behind the last array
        if crcs is not None:
            for c, o in zip(crcs, self.coff):
                self.crc_in[o:o + len(c)] = np.frombuffer(bytes(c), np.uint8)
        if dev:
            self.sbuf, self.obuf, self.cbuf = eng.alloc(src.size), eng.alloc(self.fill_o.size), eng.alloc(self.crc_in.size)
            self.sbuf.upload(src)
            self.obuf.upload(self.fill_o)
            self.cbuf.upload(self.crc_in)
            sp, op, cp = self.sbuf.ptr, self.obuf.ptr, self.cbuf.ptr
            assert op % 16 == 0
        else:
            self.src, self.obj, self.cw = src, self.fill_o.copy(), self.crc_in.copy()
            sp, op, cp = src.ctypes.data, self.obj.ctypes.data, self.cw.ctypes.data
        specs = []
        for i, p in enumerate(self.pages):
            key, seed, nonce = draw(blks[i])
            specs.append({"key": key, "nonce": nonce, "seed": seed, "src": sp + self.poff[i] if len(p) else None,
                          "len": len(p), "obj": op + self.ooff[i], "obj_cap": self.caps[i],
                          "crc": cp + self.coff[i] if with_crc else None})
        self.arr, self.n = eng.make_soblocks(specs)

    def run(self, key, algo, mode, e=M.E):
        self.eng.store_objects_batch(key, e, algo, self.codec, self.arr, self.n, mode, self.mem)
        if self.mem == E.MEM_DEVICE:
            self.obj, self.cw = self.obuf.download(), self.cbuf.download()
        return self

    def object(self, i):
        return self.obj[self.ooff[i]:self.ooff[i] + self.arr[i].out_len].tobytes()

    def crcs(self, i):
        return self.cw[self.coff[i]:self.coff[i] + 4 * _nseg(len(self.pages[i]))].tobytes()

    def outside_untouched(self):
        """Host: every byte outside obj[0, out_len); device: outside obj[0, obj_cap)."""
        m = np.ones(self.obj.size, bool)
        for i in range(self.n):
            m[self.ooff[i]:self.ooff[i] + (self.arr[i].out_len if self.mem == E.MEM_HOST else self.caps[i])] = False
        return bool((self.obj[m] == 0xA5).all() and (self.cw[self.crc_end:] == 0xA5).all())

    def slot_untouched(self, i):
        return bool((self.obj[self.ooff[i]:self.ooff[i] + self.caps[i] + GUARD] == 0xA5).all())

    def free(self):
        if self.mem == E.MEM_DEVICE:
            for b in (self.sbuf, self.obuf, self.cbuf):
                b.free()


def _check(b, algo, name, blks, skip=(), ct=True, gen=True, e=M.E):
    for i, p in enumerate(b.pages):
        if i in skip:
            continue
        obj, img_len, crc, ocrc = expected(algo, b.codec, name, blks[i], p, e)
        r = b.arr[i]
        assert (r.status, r.out_len, r.img_len) == (E.OK, len(obj), img_len), (i, len(p))
        assert (r.crc_bad_seg, r.crc_got, r.crc_expect) == (-1, 0, 0), i
        got = b.object(i)
        assert got[:HDR] == obj[:HDR], (i, len(p), "header")
        assert got[HDR:-TAG] == obj[HDR:-TAG], (i, len(p), "image")
        assert got[-TAG:] == obj[-TAG:], (i, len(p), "tag")
        assert r.obj_crc == (ocrc if ct else 0), (i, len(p))
        if gen:
            assert b.crcs(i) == crc, (i, len(p))
    assert b.outside_untouched()


_grid_pages = None


def _pages():
    global _grid_pages
    if _grid_pages is None:
        _grid_pages = [lz4_data.sample(k, n, seed=7) for k in KINDS for n in LENGTHS]
    return _grid_pages


# ---------------------------------------------------------------------------
# the grid: 52 pages per (cipher, codec, memory), GEN | CT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_lengths_and_kinds(eng, dkeys, algo, codec, mem):
    pages = _pages()
    blks = list(range(len(pages)))
    b = SBatch(eng, codec, pages, blks, mem)
    try:
        _check(b.run(dkeys[KEY_A], algo, E.CRC_GEN | E.CRC_CT), algo, KEY_A, blks)
    finally:
        b.free()


@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_large_page(eng, dkeys, algo):
    """4 MiB - 1: 128 segment CRCs to fold, two per lane; without a codec from
    host memory and with lz4 from device memory."""
    page = lz4_data.sample("text", (4 << 20) - 1, seed=12)
    for codec, mem in ((E.CODEC_NONE, E.MEM_HOST), (E.CODEC_LZ4, E.MEM_DEVICE)):
        b = SBatch(eng, codec, [page], [90], mem)
        try:
            _check(b.run(dkeys[KEY_B], algo, E.CRC_GEN | E.CRC_CT), algo, KEY_B, [90])
        finally:
            b.free()


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_empty_page(eng, dkeys, algo, mem):
    b = SBatch(eng, E.CODEC_NONE, [b""], [3], mem)
    try:
        b.run(dkeys[KEY_A], algo, E.CRC_GEN | E.CRC_CT)
        r = b.arr[0]
        assert (r.status, r.out_len, r.img_len) == (E.OK, 287, 0)
        _check(b, algo, KEY_A, [3])
        assert b.crcs(0) == bytes(4)
    finally:
        b.free()


# ---------------------------------------------------------------------------
# VERIFY: two of eight pages fail; metrics
# ---------------------------------------------------------------------------
def _delta(m0, m1):
    return {k: m1[k] - m0[k] for k in m1 if isinstance(m1[k], int) and m1[k] != m0[k]}


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
def test_verify_failures(eng, dkeys, codec, mem):
    algo = E.AES256GCM if codec != E.CODEC_LZ4 else E.CHACHA20P1305
    lens = [100000, 32768, 5, 70000, 0, 4096, 65536, 33000]
    pages = [lz4_data.sample("text", n, seed=21 + i) for i, n in enumerate(lens)]
    good = [bytes(orc.checksum(p, hw=True)) for p in pages]
    bad = {1: 0, 3: 2}  # block -> segment
    crcs = [bytearray(g) for g in good]
    for i, seg in bad.items():
        crcs[i][4 * seg + 1] ^= 0x40
    blks = list(range(200, 208))
    b = SBatch(eng, codec, pages, blks, mem, crcs=crcs)
    m0 = eng.metrics()
    try:
        b.run(dkeys[KEY_A], algo, E.CRC_VERIFY | E.CRC_CT)
        m1 = eng.metrics()
        for i, seg in bad.items():
            r = b.arr[i]
            assert (r.status, r.out_len, r.img_len, r.obj_crc, r.crc_bad_seg) == (E.ECRC, 0, 0, 0, seg), i
            assert r.crc_got == int.from_bytes(good[i][4 * seg:4 * seg + 4], "big"), i
            assert r.crc_expect == int.from_bytes(crcs[i][4 * seg:4 * seg + 4], "big"), i
            assert b.slot_untouched(i), i
        _check(b, algo, KEY_A, blks, skip=bad, gen=False)
        assert (b.cw == b.crc_in).all()  # VERIFY reads the arrays
        ok = [i for i in range(8) if i not in bad]
        imgs = sum(b.arr[i].img_len for i in ok)
        want = {"crc_batches": 1, "crc_ranges": 8, "crc_bytes": sum(lens), "crc_fail": 2,
                "seal_batches": 1, "seal_blocks": 6, "seal_bytes": imgs}
        if codec != E.CODEC_NONE:
            pre = "lz4c" if codec == E.CODEC_LZ4 else "zstdc"
            want.update({pre + "_blocks": 6, pre + "_in": sum(lens[i] for i in ok), pre + "_out": imgs})
        want = {k: v for k, v in want.items() if v}
        d = _delta(m0, m1)
        d.pop("kernel_launches", None)
        assert d == want
    finally:
        b.free()


# ---------------------------------------------------------------------------
# modes: CRC_NONE, CT alone, GEN alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("mode", [E.CRC_NONE, E.CRC_CT, E.CRC_GEN], ids=["none", "ct", "gen"])
def test_modes(eng, dkeys, mode, codec, mem):
    pages = [lz4_data.sample("runs", n, seed=31) for n in (0, 17, 32769, 70001)]
    blks = [300, 301, 302, 303]
    for algo in CIPHERS:
        b = SBatch(eng, codec, pages, blks, mem)
        try:
            b.run(dkeys[KEY_B], algo, mode)
            gen, ct = bool(mode & E.CRC_GEN), bool(mode & E.CRC_CT)
            _check(b, algo, KEY_B, blks, ct=ct, gen=gen)
            if not gen:
                assert (b.cw == 0xA5).all()  # a crc pointer that is not used is not written
        finally:
            b.free()
    # and no crc pointer at all
    b = SBatch(eng, codec, pages, blks, mem, with_crc=False)
    try:
        if mode & E.CRC_GEN:
            with pytest.raises(E.EngineError):
                b.run(dkeys[KEY_B], E.AES256GCM, mode)
        else:
            _check(b.run(dkeys[KEY_B], E.AES256GCM, mode), E.AES256GCM, KEY_B, blks, ct=bool(mode & E.CRC_CT), gen=False)
    finally:
        b.free()


# ---------------------------------------------------------------------------
# batch sizes across the wrap's 16-item groups, the encode's 64 and the
# 256-thread kernels; one context, a growing then a shrinking batch
# ---------------------------------------------------------------------------
SIZES = [1, 15, 16, 17, 63, 64, 65, 257]


@pytest.mark.parametrize("order", ["growing", "shrinking"])
def test_batch_sizes(dkeys, order):
    # the module's keys live on device 0; the fresh context shares the device
    e2 = E.Engine(0)
    try:
        for n in (SIZES if order == "growing" else SIZES[::-1]):
            pages = [lz4_data.sample("text", (37 * i) % 4097, seed=41) for i in range(n)]
            blks = list(range(1000, 1000 + n))
            codec = CODECS[n % 3]
            mem = MEMS[n % 2]
            b = SBatch(e2, codec, pages, blks, mem)
            try:
                _check(b.run(dkeys[KEY_A], E.CHACHA20P1305 if n % 2 else E.AES256GCM, E.CRC_GEN | E.CRC_CT),
                       E.CHACHA20P1305 if n % 2 else E.AES256GCM, KEY_A, blks)
            finally:
                b.free()
    finally:
        e2.close()


# ---------------------------------------------------------------------------
# equals the separate calls, on a ragged batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_equals_separate_calls(eng, dkeys, algo, codec):
    lens = [0, 1, 13, 100, 4095, 4096, 32767, 32768, 32769, 50000, 65536, 65541, 100003, 7, 131072, 200000]
    pages = [lz4_data.sample(KINDS[i % 4], n, seed=51) for i, n in enumerate(lens)]
    blks = list(range(400, 416))
    draws = [draw(k) for k in blks]
    items = [(k, s, n, p) for (k, s, n), p in zip(draws, pages)]
    got = eng.store_objects(dkeys[KEY_A], M.E, algo, codec, items, crc=True, object_crc=True)
    wrapped = eng.oaep_encrypt_batch(dkeys[KEY_A], [k for k, _, _ in draws], [s for _, s, _ in draws])
    hdrs = [bytes([1, 0, 12]) + w + n for w, (_, _, n) in zip(wrapped, draws)]
    if codec == E.CODEC_NONE:
        sep = []
        for (k, _, n), p, h in zip(draws, pages, hdrs):
            src = np.frombuffer(p, np.uint8).copy() if p else np.zeros(1, np.uint8)
            dst = np.empty(max(len(p), 1), np.uint8)
            cw = np.empty(8 * _nseg(len(p)), np.uint8)
            arr, cnt = eng.make_blocks([{"key": k, "nonce": n, "src": src.ctypes.data, "dst": dst.ctypes.data,
                                         "len": len(p), "crc": cw.ctypes.data}])
            eng.seal_batch(algo, arr, cnt, E.CRC_GEN | E.CRC_BOTH, E.MEM_HOST)
            tag, half = bytes(arr[0].tag), 4 * _nseg(len(p))
            obj = h + dst[:len(p)].tobytes() + tag
            sep.append((E.OK, obj, cw[:half].tobytes(),
                        E.object_crc32c(h, cw[half:].tobytes(), len(p), tag)))
    else:
        res = eng.store(algo, codec, [(k, n, p) for (k, _, n), p in zip(draws, pages)], crc=True, headers=hdrs)
        sep = [(st, h + img + tag, crc, ocrc) for (st, img, tag, crc, ocrc), h in zip(res, hdrs)]
    for i, (a, b) in enumerate(zip(got, sep)):
        assert a == b, (i, lens[i])


# ---------------------------------------------------------------------------
# round trip: jfsx_load_objects and the oracle's Decrypt give back the pages
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_round_trip(eng, dkeys, algo, codec):
    pages = [lz4_data.sample(KINDS[i % 4], n, seed=61) for i, n in enumerate((1, 4096, 32769, 65541, 150000))]
    if codec == E.CODEC_NONE:
        pages.append(b"")
    items = [draw(500 + i) for i in range(len(pages))]
    got = eng.store_objects(dkeys[KEY_B], M.E, algo, codec, [(k, s, n, p) for (k, s, n), p in zip(items, pages)])
    assert [g[0] for g in got] == [E.OK] * len(pages)
    objs = [g[1] for g in got]
    back = eng.load_objects(dkeys[KEY_B], algo, codec, [(o[:HDR], o[HDR:-TAG], o[-TAG:]) for o in objs],
                            [len(p) for p in pages], crc=True, expect=[g[3] for g in got])
    for i, ((st, page, crc), p) in enumerate(zip(back, pages)):
        assert (st, page, crc) == (E.OK, p, got[i][2]), i
    for i, (o, p) in enumerate(zip(objs, pages)):
        key = M.decrypt(M.fixed_keys()[KEY_B], o[3:259])
        assert key == items[i][0], i
        comp = orc.data_decrypt(_orc_algo(algo), key, o)
        assert comp is not None, i
        assert bytes(comp) == _compress(codec, p), i


# ---------------------------------------------------------------------------
# in turn with the calls that share its workspaces; two RSA keys alive
# ---------------------------------------------------------------------------
def test_in_turn_with_other_calls(eng, dkeys):
    pages = [lz4_data.sample("text", n, seed=71) for n in (9, 40000, 70000)]
    for rnd, (name, algo, codec) in enumerate(((KEY_A, E.AES256GCM, E.CODEC_LZ4), (KEY_B, E.CHACHA20P1305, E.CODEC_NONE),
                                               (KEY_A, E.CHACHA20P1305, E.CODEC_ZSTD), (KEY_B, E.AES256GCM, E.CODEC_LZ4))):
        blks = [600 + 3 * rnd + i for i in range(3)]
        items = [draw(k) for k in blks]
        # the wrap alone: 40 items, more than the one call's three
        batch = [(M.det_bytes(32, "turn", rnd, i), M.det_bytes(32, "turn seed", rnd, i)) for i in range(40)]
        assert eng.oaep_encrypt_batch(dkeys[name], [m for m, _ in batch], [s for _, s in batch]) == \
            [wrap(name, m, s) for m, s in batch]
        got = eng.store_objects(dkeys[name], M.E, algo, codec, [(k, s, n, p) for (k, s, n), p in zip(items, pages)])
        for i, p in enumerate(pages):
            obj, _, crc, ocrc = expected(algo, codec, name, blks[i], p)
            assert got[i] == (E.OK, obj, crc, ocrc), (rnd, i)
        if codec != E.CODEC_NONE:
            res = eng.store(algo, codec, [(k, n, p) for (k, _, n), p in zip(items, pages)], crc=True)
            for i, (st, img, tag, crc, _) in enumerate(res):
                assert (st, img + tag) == (E.OK, got[i][1][HDR:]), (rnd, i)
        back = eng.load_objects(dkeys[name], algo, codec, [(g[1][:HDR], g[1][HDR:-TAG], g[1][-TAG:]) for g in got],
                                [len(p) for p in pages], expect=[g[3] for g in got])
        assert [(st, pg) for st, pg, _ in back] == [(E.OK, p) for p in pages], rnd


# ---------------------------------------------------------------------------
# device alignment; another public exponent
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mod", [0, 2, 8])
def test_device_alignment(eng, dkeys, mod):
    b = SBatch(eng, E.CODEC_LZ4, [lz4_data.sample("text", 500, seed=81)], [700], E.MEM_DEVICE, obj_mod=mod)
    try:
        rc = eng.L.jfsx_store_objects(eng.ctx, dkeys[KEY_A], M.E, E.AES256GCM, E.CODEC_LZ4, 1, b.arr,
                                      E.CRC_GEN | E.CRC_CT, E.MEM_DEVICE)
        assert rc == E.EINVAL
        assert (b.obuf.download() == 0xA5).all()
    finally:
        b.free()


def test_other_exponent_and_foreign_key(eng, dkeys):
    pages = [lz4_data.sample("text", 3000, seed=82)]
    b = SBatch(eng, E.CODEC_ZSTD, pages, [710], E.MEM_HOST)
    _check(b.run(dkeys[KEY_A], E.AES256GCM, E.CRC_GEN | E.CRC_CT, e=17), E.AES256GCM, KEY_A, [710], e=17)
    for e in (0, 1, 1 << 31):
        assert eng.L.jfsx_store_objects(eng.ctx, dkeys[KEY_A], e, E.AES256GCM, E.CODEC_ZSTD, 1, b.arr,
                                        E.CRC_GEN, E.MEM_HOST) == E.EINVAL, e


# ---------------------------------------------------------------------------
# the Python layer: upload_objects_fused against the separate-call paths under
# the same deterministic rand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", ["none", "lz4", "zstd"])
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_upload_objects_fused(eng, algo, codec):
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as EN
    from tests.test_gpu_rsa_wrap import Rand, pem_of
    k = M.fixed_keys()["wide_p_gt_q"]
    rsae = EN.NewRSAEncryptor(EN.ParseRsaPrivateKeyFromPem(pem_of(k)))
    comp = C.NewCompressor(codec, eng)
    blocks = [lz4_data.sample(kind, n, seed=90 + i) for i, (kind, n) in
              enumerate([("text", 70000), ("zeros", 32768), ("text", 5), ("random", 40001)])]
    keys = ["chunks/0/0/%d_0_%d" % (i, len(b)) for i, b in enumerate(blocks)]
    rnd = Rand("objects")
    one = EN.MemStorage()
    objs, crcs, sums = C.upload_objects_fused(one, keys, blocks, comp, EN.DataEncryptor(rsae, algo, eng, rand=rnd),
                                              object_checksums=True)
    assert rnd.calls == [32, 32, 12] * len(blocks)
    assert crcs == [bytes(orc.checksum(b, hw=True)) for b in blocks]
    assert sums == [str(int(orc.object_checksum(o, hw=True))) for o in objs]
    # the separate calls with the same draws
    de = EN.DataEncryptor(rsae, algo, eng, rand=Rand("objects"), wrap="gpu")
    sep = EN.MemStorage()
    if codec == "none":
        want = de.EncryptBatch(blocks)
        for kk, o in zip(keys, want):
            sep.Put(kk, o)
    else:
        want, crcs2 = C.upload_blocks_fused(sep, keys, blocks, comp, enc=de)
        assert crcs2 == crcs
    assert objs == want
    assert [bytes(one.Get(kk, 0, -1)) for kk in keys] == [bytes(sep.Get(kk, 0, -1)) for kk in keys] == want
    replay = Rand("objects")
    for o in objs:
        key, seed, nonce = replay(32), replay(32), replay(12)
        assert o[:HDR] == bytes([1, 0, 12]) + wrap("wide_p_gt_q", key, seed) + nonce
    pages, crcs3 = C.load_objects_fused(one, keys, [len(b) for b in blocks], comp, de, object_checksums=sums)
    assert pages == blocks and crcs3 == crcs
    # None for the compressor of a volume without --compress; fewer outputs on request
    if codec == "none":
        again = C.upload_objects_fused(EN.MemStorage(), keys, blocks, None,
                                       EN.DataEncryptor(rsae, algo, eng, rand=Rand("objects")), checksums=False)
        assert again == objs
