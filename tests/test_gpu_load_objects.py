"""GPU tests of the one-call object load (jfsx_load_objects): the object
store's checksum verify, the data-key unwrap, Open, decompress and checksum()
of a batch of stored objects, with no unwrapped key and no intermediate on the
host.

A stored object is hdr || seal(compress(plain)) || tag with hdr = BE16(klen) |
nlen | wrapped key | nonce.  RSA keys are the fixed ones of
tests/golden/rsa_keys.json; wrapped keys are built by tests/rsa_model.py
(oaep_encode + encrypt_em with seeds from det_bytes), so every run is
identical and needs no libcrypto.  Every expected value comes from the suite's
checkers (oracle, tests.rsa_model, tests.zstd_lib, tests.lz4_data), and
`classify` states from them, before any engine result is looked at, which rule
of include/jfsx.h an object reaches."""
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
LENGTHS = [0, 1, 13, 32767, 32768, 32769, 65541]
KINDS = ["text", "runs", "zeros", "random"]
SEED = 0x0B7
KEY_A, KEY_B = "plain_p_gt_q", "wide_q_gt_p"


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dkeys(eng):
    """Both fixed RSA keys on the device for the whole module: two keys alive at once."""
    assert KEY_A in M.fixed_keys() and KEY_B in M.fixed_keys()
    h = {nm: eng.rsa_key(*M.components(M.fixed_keys()[nm])) for nm in (KEY_A, KEY_B)}
    yield h
    for v in h.values():
        eng.rsa_key_free(v)


def _orc_algo(algo):
    return orc.AES256GCM if algo == E.AES256GCM else orc.CHACHA20P1305


def _compress(codec, plain):
    if codec == E.CODEC_NONE:
        return bytes(plain)
    return orc.lz4_compress(plain) if codec == E.CODEC_LZ4 else zstd_lib.compress_simple(plain)


def _nseg(n):
    return max(1, -(-n // E.SEG))


@functools.lru_cache(maxsize=None)
def wrap(name, msg, salt=0):
    """RSAES-OAEP of msg under the fixed key `name`, 256 bytes."""
    k = M.fixed_keys()[name]
    return M.ct256(M.encrypt_em(k, M.oaep_encode(msg, M.det_bytes(M.HLEN, name, "obj seed", msg.hex(), salt))))


@functools.lru_cache(maxsize=None)
def unwrap(name, w):
    return M.decrypt(M.fixed_keys()[name], w)


def header(w, nonce):
    return bytes([len(w) >> 8, len(w) & 0xFF, len(nonce)]) + w + nonce


def make_obj(algo, name, blk, comp):
    """(hdr, C, tag) of a compressed block sealed under the data key of (SEED, blk % 8)."""
    key, _ = orc.gen_key(SEED, blk % 8)
    _, nonce = orc.gen_key(SEED, blk)
    c, tag = orc.seal(_orc_algo(algo), key, nonce, comp, fast=True)
    return header(wrap(name, key), nonce), c, tag


def crc_of(obj):
    hdr, c, tag = obj
    return int(orc.object_checksum(hdr + c + tag, hw=True))


def classify(name, algo, codec, obj, expect, length, ct):
    """(status, out_len, key_len, page) of one object by the table of
    include/jfsx.h, from the checkers alone."""
    hdr, c, tag = obj
    hdr_ok = len(hdr) >= 3 and len(hdr) == 3 + (hdr[0] << 8) + hdr[1] + hdr[2]
    kl, nl = ((hdr[0] << 8) + hdr[1], hdr[2]) if hdr_ok else (0, 0)
    key = None
    if not hdr_ok:
        key_len = 0
    elif kl == 0 or kl > 256:
        key_len = -1
    else:
        key = unwrap(name, hdr[3:3 + kl])
        key_len = -1 if key is None else len(key)
    if ct and crc_of(obj) != expect:
        return E.ECRC, 0, key_len, None
    if not hdr_ok:
        return E.EHEADER, 0, key_len, None
    if key_len != 32:
        return E.EKEY, 0, key_len, None
    comp = orc.open_(_orc_algo(algo), key, hdr[3 + kl:], c, tag, fast=True) if nl == 12 else None
    if comp is None:
        return E.ETAG, 0, key_len, None
    st, out_len, page = decode(codec, comp, length)
    return st, out_len, key_len, page


def decode(codec, comp, length):
    """(status, out_len, page) of the decoder and length rows."""
    if codec == E.CODEC_NONE:
        return E.OK, length, comp
    if codec == E.CODEC_LZ4:
        r, d = orc.lz4_decompress(comp, length)
    else:
        r, d = zstd_lib.decompress(comp, length)
    if r < 0:
        if codec == E.CODEC_ZSTD:
            # one library error code: a frame that is well formed but larger than the page is EDSTSIZE
            big = zstd_lib.decompress(comp, 4 * length + 64)[0]
            return (E.EDSTSIZE if big > length else E.EFORMAT), 0, None
        return E.EFORMAT, 0, None
    if r < length:
        return E.ESHORT, r, None
    return E.OK, length, d


class OBatch:
    """A batch laid out in host or device memory; pages and CRC arrays are
    pre-filled with 0xA5 so that an untouched byte is caught.  objs: (hdr, C,
    tag), or (b"", image, None) without a cipher."""

    def __init__(self, eng, objs, lengths, mem, expect=None, crc=True, src_skew=0, dst_skew=0):
        self.eng, self.mem, self.lengths, self.crc = eng, mem, [int(n) for n in lengths], crc
        al = lambda x: (x + 31) & ~15  # noqa: E731  16-byte slots with room for a skew
        self.soff, self.doff, self.coff = [], [], []
        so = do = co = 0
        for (_, c, _), ln in zip(objs, self.lengths):
            self.soff.append(so + src_skew)
            self.doff.append(do + dst_skew)
            self.coff.append(co)
            so += al(len(c))
            do += al(ln)
            co += 4 * _nseg(ln)
        src = np.zeros(max(so, 16), np.uint8)
        for (_, c, _), o in zip(objs, self.soff):
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
        self.hdrs = [np.frombuffer(h, np.uint8).copy() if len(h) else None for h, _, _ in objs]  # host, both modes
        specs = []
        for i, (h, c, tag) in enumerate(objs):
            specs.append({"hdr": self.hdrs[i].ctypes.data if len(h) else None, "hdr_len": len(h), "tag": tag,
                          "src": sp + self.soff[i] if len(c) else None, "src_len": len(c),
                          "dst": dp + self.doff[i] if self.lengths[i] else None, "len": self.lengths[i],
                          "crc": cp + self.coff[i] if crc else None,
                          "expect_crc": expect[i] if expect is not None else 0})
        self.arr, self.n = eng.make_oblocks(specs)
        self.ct = expect is not None

    def run(self, key, algo, codec):
        mode = (E.CRC_GEN if self.crc else E.CRC_NONE) | (E.CRC_CT if self.ct else 0)
        self.eng.load_objects_batch(key, algo, codec, self.arr, self.n, mode, self.mem)
        if self.mem == E.MEM_DEVICE:
            self.dst, self.cw = self.dbuf.download(), self.cbuf.download()
        return self

    def page(self, i):
        return self.dst[self.doff[i]:self.doff[i] + self.lengths[i]].tobytes()

    def crcs(self, i):
        return self.cw[self.coff[i]:self.coff[i] + 4 * _nseg(self.lengths[i])].tobytes()

    def outside_untouched(self):
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


_cache = {}


def _grid(codec):
    """(plain, compressed, checksum) of every (kind, length), computed once."""
    if codec not in _cache:
        _cache[codec] = [(p, _compress(codec, p), orc.checksum(p, hw=True))
                         for p in (lz4_data.sample(k, n, seed=7) for k in KINDS for n in LENGTHS)]
    return _cache[codec]


def _check_good(b, grid, expect, keyed=True):
    for i, (p, _, crc) in enumerate(grid):
        r = b.arr[i]
        assert (r.status, r.out_len, r.key_len) == (E.OK, len(p), 32 if keyed else 0), (i, len(p))
        assert r.obj_crc == expect[i], i
        assert b.page(i) == p, (i, len(p))
        assert b.crcs(i) == crc, (i, len(p))
    assert b.outside_untouched()


# ---------------------------------------------------------------------------
# the good path: 28 objects per (cipher, codec, memory), all verified
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_lengths_and_kinds(eng, dkeys, algo, codec, mem):
    grid = _grid(codec)
    objs = [make_obj(algo, KEY_A, i, c) for i, (_, c, _) in enumerate(grid)]
    expect = [crc_of(o) for o in objs]
    # odd offsets where the rule allows them: host memory (device: Open and both CRC passes read aligned)
    skew = (3, 5) if mem == E.MEM_HOST else (0, 0)
    b = OBatch(eng, objs, [len(p) for p, _, _ in grid], mem, expect, src_skew=skew[0], dst_skew=skew[1])
    try:
        _check_good(b.run(dkeys[KEY_A], algo, codec), grid, expect)
    finally:
        b.free()


@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_large_objects(eng, dkeys, algo):
    """1 MiB and 4 MiB - 1: more than one task per block, 128 segment CRCs to
    fold (two per lane), once without a codec from host memory and once with
    zstd from device memory."""
    plains = [lz4_data.sample("text", 1 << 20, seed=11), lz4_data.sample("runs", (4 << 20) - 1, seed=12)]
    for codec, mem in ((E.CODEC_NONE, E.MEM_HOST), (E.CODEC_ZSTD, E.MEM_DEVICE)):
        grid = [(p, _compress(codec, p), orc.checksum(p, hw=True)) for p in plains]
        objs = [make_obj(algo, KEY_B, 40 + i, c) for i, (_, c, _) in enumerate(grid)]
        expect = [crc_of(o) for o in objs]
        b = OBatch(eng, objs, [len(p) for p in plains], mem, expect)
        try:
            _check_good(b.run(dkeys[KEY_B], algo, codec), grid, expect)
        finally:
            b.free()


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", [E.CODEC_LZ4, E.CODEC_ZSTD], ids=["lz4", "zstd"])
def test_no_cipher_verifies_the_image(eng, codec, mem):
    grid = _grid(codec)
    objs = [(b"", c, None) for _, c, _ in grid]
    expect = [int(orc.object_checksum(c, hw=True)) for _, c, _ in grid]
    bad = 9  # one image with a flipped bit and its old checksum
    c = bytearray(objs[bad][1])
    c[len(c) // 2] ^= 4
    objs[bad] = (b"", bytes(c), None)
    b = OBatch(eng, objs, [len(p) for p, _, _ in grid], mem, expect)
    m0 = eng.metrics()
    try:
        b.run(None, E.CIPHER_NONE, codec)
        m1 = eng.metrics()
        r = b.arr[bad]
        assert (r.status, r.out_len, r.key_len) == (E.ECRC, 0, 0)
        assert r.obj_crc == int(orc.object_checksum(objs[bad][1], hw=True)) != expect[bad]
        assert b.page(bad) == bytes(b.lengths[bad]) and b.crcs(bad) == bytes(4 * _nseg(b.lengths[bad]))
        keep = [i for i in range(len(grid)) if i != bad]
        for i in keep:
            assert (b.arr[i].status, b.arr[i].obj_crc, b.page(i), b.crcs(i)) == (E.OK, expect[i], grid[i][0], grid[i][2])
        assert b.outside_untouched()
        key = "lz4d_blocks" if codec == E.CODEC_LZ4 else "zstdd_blocks"
        assert m1[key] - m0[key] == len(keep)  # the failed image never reached the decoder
        assert m1["open_blocks"] == m0["open_blocks"] and m1["crc_fail"] - m0["crc_fail"] == 1
    finally:
        b.free()


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", [E.CODEC_NONE, E.CODEC_LZ4], ids=["none", "lz4"])
@pytest.mark.parametrize("ct", [True, False], ids=["ct-alone", "crc-none"])
def test_without_page_crcs_the_crc_arrays_stay_untouched(eng, dkeys, codec, mem, ct):
    """JFSX_CRC_CT alone and JFSX_CRC_NONE: no crc pointer is needed, and a
    failed block's page is still wiped."""
    plains = [lz4_data.sample("text", n, seed=90) for n in (40000, 100001, 100001)]
    objs = [make_obj(E.AES256GCM, KEY_A, 80 + i, _compress(codec, p)) for i, p in enumerate(plains)]
    expect = [crc_of(o) for o in objs]
    h, c, t = objs[2]
    objs[2] = (h, c[:50] + bytes([c[50] ^ 1]) + c[51:], t)
    b = OBatch(eng, objs, [len(p) for p in plains], mem, expect if ct else None, crc=False)
    try:
        b.run(dkeys[KEY_A], E.AES256GCM, codec)
        assert [b.arr[i].status for i in range(3)] == [E.OK, E.OK, E.ECRC if ct else E.ETAG]
        assert b.page(0) == plains[0] and b.page(1) == plains[1] and b.page(2) == bytes(100001)
        assert [b.arr[i].obj_crc for i in range(3)] == ([crc_of(o) for o in objs] if ct else [0, 0, 0])
        assert (b.cw == 0xA5).all() and b.outside_untouched()
    finally:
        b.free()


# ---------------------------------------------------------------------------
# one failure batch per cipher and codec
# ---------------------------------------------------------------------------
def _failure_batch(algo, codec):
    """[(what, obj, expect_crc)] with every status of the table, OK neighbours
    between them; every page is L bytes."""
    L = 70001
    k = M.fixed_keys()[KEY_A]
    plain = [lz4_data.sample(kd, L, seed=60 + i) for i, kd in enumerate(["text", "runs", "text", "random"])]
    comp = [_compress(codec, p) for p in plain]
    good = lambda blk, j=0: make_obj(algo, KEY_A, blk, comp[j % 4])  # noqa: E731
    out = []

    def add(what, obj, expect=None):
        out.append((what, obj, crc_of(obj) if expect is None else expect))

    def flip(b, at, bit=1):
        b = bytearray(b)
        b[at] ^= bit
        return bytes(b)

    def rewrap(blk, w, nonce_len=12, key=None):
        """An object of block blk whose header carries w in place of its wrapped key."""
        dkey, _ = orc.gen_key(SEED, blk % 8)
        _, nonce = orc.gen_key(SEED, blk)
        c, tag = orc.seal(_orc_algo(algo), key or dkey, nonce, comp[blk % 4], fast=True)
        return header(w, nonce[:nonce_len]), c, tag

    add("ok", good(0))
    h, c, t = good(1, 1)
    add("bit in C", (h, flip(c, len(c) // 3), t), crc_of((h, c, t)))
    add("ok", good(2, 2))
    add("bit in hdr", (flip(h, 100), c, t), crc_of((h, c, t)))
    add("bit in tag", (h, c, flip(t, 15, 0x80)), crc_of((h, c, t)))
    add("ok", good(3, 3))
    dkey = orc.gen_key(SEED, 4)[0]
    bad_em = M.oaep_encode(dkey, M.det_bytes(M.HLEN, "fail", 0), label=b"other")
    add("oaep: other label", rewrap(4, M.ct256(M.encrypt_em(k, bad_em))))
    bad_em = M.oaep_encode(dkey, M.det_bytes(M.HLEN, "fail", 1), patch=lambda db: db.__setitem__(40, 2))
    add("oaep: 0x02 in the padding", rewrap(4, M.ct256(M.encrypt_em(k, bad_em))))
    add("c >= n", rewrap(4, M.ct256(k.n)))
    add("another key's wrap", rewrap(4, wrap(KEY_B, dkey)))
    add("ok", good(5, 1))
    for n in (0, 31, 33):
        add("message of %d bytes" % n, rewrap(6, wrap(KEY_A, M.det_bytes(n, "short key", n))))
    msg, cint = M.short_ciphertext(KEY_A)
    add("klen 255", rewrap(7, cint.to_bytes(255, "big"), key=msg))
    add("klen 257", rewrap(7, b"\0" + M.ct256(cint), key=msg))
    add("klen 0", rewrap(7, b""))
    h, c, t = good(8)
    add("header one byte short", (h[:-1], c, t))
    add("header of 2 bytes", (h[:2], c, t))
    add("ok", good(9, 2))
    add("nlen 11", rewrap(10, wrap(KEY_A, orc.gen_key(SEED, 10 % 8)[0]), nonce_len=11))
    if codec != E.CODEC_NONE:
        add("decoder reject", make_obj(algo, KEY_A, 11, lz4_data.sample("random", 5000, seed=99)))
        add("short page", make_obj(algo, KEY_A, 12, _compress(codec, lz4_data.sample("text", L - 7, seed=50))))
        add("long page", make_obj(algo, KEY_A, 13, _compress(codec, lz4_data.sample("text", L + 9, seed=51))))
    add("ok", good(14, 3))
    return L, out, plain


@pytest.mark.parametrize("mem", MEMS, ids=["host", "device"])
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_failure_batch(eng, dkeys, algo, codec, mem):
    L, cases, plain = _failure_batch(algo, codec)
    what = [w for w, _, _ in cases]
    objs, expect = [o for _, o, _ in cases], [e for _, _, e in cases]
    if codec == E.CODEC_NONE:  # the image is the page
        L = None
    lens = [L if L is not None else len(o[1]) for o in objs]
    for ct in (True, False):
        want = [classify(KEY_A, algo, codec, o, e, n, ct) for o, e, n in zip(objs, expect, lens)]
        # the construction reaches the rules it is meant to reach
        fate = dict(zip(what, [(w[0], w[2]) for w in want]))
        assert fate["ok"] == (E.OK, 32) and [w[0] for w, nm in zip(want, what) if nm == "ok"].count(E.OK) == 6
        assert fate["bit in C"][0] == fate["bit in tag"][0] == (E.ECRC if ct else E.ETAG)
        assert fate["bit in hdr"] == ((E.ECRC, -1) if ct else (E.EKEY, -1))
        for nm in ("oaep: other label", "oaep: 0x02 in the padding", "c >= n", "another key's wrap", "klen 257",
                   "klen 0"):
            assert fate[nm] == (E.EKEY, -1), nm
        assert [fate["message of %d bytes" % n] for n in (0, 31, 33)] == [(E.EKEY, 0), (E.EKEY, 31), (E.EKEY, 33)]
        assert fate["klen 255"] == (E.OK, 32) and fate["nlen 11"] == (E.ETAG, 32)
        assert fate["header one byte short"] == fate["header of 2 bytes"] == (E.EHEADER, 0)
        if codec != E.CODEC_NONE:
            assert fate["decoder reject"][0] == E.EFORMAT and fate["short page"][0] == E.ESHORT
            assert fate["long page"][0] == (E.EFORMAT if codec == E.CODEC_LZ4 else E.EDSTSIZE)
            assert want[what.index("short page")][1] == lens[0] - 7
        b = OBatch(eng, objs, lens, mem, expect if ct else None)
        m0 = eng.metrics()
        try:
            b.run(dkeys[KEY_A], algo, codec)
            m1 = eng.metrics()
            for i, (st, out_len, key_len, page) in enumerate(want):
                r = b.arr[i]
                assert (r.status, r.out_len, r.key_len) == (st, out_len, key_len), (what[i], ct)
                if ct:
                    assert r.obj_crc == crc_of(objs[i]), what[i]
                if st == E.OK:
                    assert b.page(i) == page and b.crcs(i) == orc.checksum(page, hw=True), what[i]
                else:
                    assert b.page(i) == bytes(lens[i]) and b.crcs(i) == bytes(4 * _nseg(lens[i])), what[i]
            assert b.outside_untouched()
            # no failed block reached a decoder, none without its own key reached Open
            early = (E.ECRC, E.EHEADER, E.EKEY)
            d = {k: m1[k] - m0[k] for k in m1 if k != "kernel_ms"}
            assert d["open_blocks"] == sum(1 for w in want if w[0] not in early)
            assert d["open_fail"] == sum(1 for w in want if w[0] == E.ETAG)
            reached = sum(1 for w in want if w[0] not in early + (E.ETAG,)) if codec != E.CODEC_NONE else 0
            assert d["lz4d_blocks"] + d["zstdd_blocks"] == reached
            assert d["lz4d_fail"] + d["zstdd_fail"] == sum(1 for w in want if w[0] in (E.EFORMAT, E.EDSTSIZE))
            assert d["crc_fail"] == sum(1 for w in want if w[0] == E.ECRC)
        finally:
            b.free()


# ---------------------------------------------------------------------------
# the one call against the separate calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_equals_separate_calls(eng, dkeys, algo, codec):
    rng = np.random.default_rng(16)
    lens = [int(x) for x in rng.integers(1, 300000, 16)]
    plains = [lz4_data.sample(lz4_data.KINDS[i % len(lz4_data.KINDS)], n, seed=200 + i) for i, n in enumerate(lens)]
    comps = [_compress(codec, p) for p in plains]
    if codec != E.CODEC_NONE:
        comps[9] = comps[9][:-1]
    objs = [make_obj(algo, KEY_B, 300 + i, c) for i, c in enumerate(comps)]
    h, c, t = objs[5]
    objs[5] = (h, c, t[:15] + bytes([t[15] ^ 1]))
    expect = [crc_of(o) for o in objs]  # the tag flip is in the checksum: it reaches Open
    # separate: unwrap (the keys come to the host), load or open, the checksum fold
    keys = eng.oaep_decrypt_batch(dkeys[KEY_B], [o[0][3:259] for o in objs])
    assert all(k is not None and len(k) == 32 for k in keys)
    srcs = [np.frombuffer(o[1], np.uint8).copy() for o in objs]
    outs = [np.zeros(max(s.size, 1), np.uint8) for s in srcs]
    segs = [np.zeros(4 * _nseg(s.size), np.uint8) for s in srcs]
    arr, n = eng.make_blocks([{"key": k, "nonce": o[0][259:], "src": s.ctypes.data, "dst": d.ctypes.data,
                               "len": s.size, "tag": o[2], "crc": g.ctypes.data}
                              for k, o, s, d, g in zip(keys, objs, srcs, outs, segs)])
    eng.open_batch(algo, arr, n, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
    sep_crc = [eng.object_crc32c(o[0], g, s.size, o[2]) for o, g, s in zip(objs, segs, srcs)]
    if codec == E.CODEC_NONE:
        sep = [(arr[i].status, outs[i][:srcs[i].size].tobytes() if arr[i].status == E.OK else bytes(lens[i]))
               for i in range(16)]
        sep = [(st, p, eng.checksum(p) if st == E.OK else bytes(4 * _nseg(len(p)))) for st, p in sep]
    else:
        sep = eng.load(algo, codec, [(k, o[0][259:], o[1], o[2]) for k, o in zip(keys, objs)], lens, crc=True)
    assert [s[0] for s in sep].count(E.OK) == (15 if codec == E.CODEC_NONE else 14) and sep[5][0] == E.ETAG
    # one call
    got = eng.load_objects(dkeys[KEY_B], algo, codec, objs, lens, crc=True, expect=expect)
    assert got == sep
    assert [i[3] for i in eng.load_info] == sep_crc == expect
    for i, (st, page, _) in enumerate(got):
        assert page == (plains[i] if st == E.OK else bytes(lens[i])), i


# ---------------------------------------------------------------------------
# batch sizes around the kernels' workgroup sizes; workspace reuse
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_objects(algo, name):
    plains = [lz4_data.sample("text", 13, seed=500 + i) for i in range(257)]
    return plains, [make_obj(algo, name, 1000 + i, orc.lz4_compress(p)) for i, p in enumerate(plains)]


def test_batch_sizes_and_reuse(eng, dkeys):
    """32 objects per workgroup of rsa_pair_k, 64 of rsa_finish_k, 256 of the
    one-thread-per-object kernels; a small batch after a large one; the two RSA
    keys in turn."""
    for n in (257, 1, 31, 32, 33, 63, 64, 65, 129, 255, 256, 2):
        name = KEY_A if n % 2 else KEY_B
        plains, objs = _small_objects(E.AES256GCM, name)
        objs, plains = list(objs[:n]), plains[:n]
        expect = [crc_of(o) for o in objs]
        if n > 2:  # the last object of the batch fails alone
            h, c, t = objs[n - 1]
            objs[n - 1] = (h, c, bytes([t[0] ^ 2]) + t[1:])
        got = eng.load_objects(dkeys[name], E.AES256GCM, E.CODEC_LZ4, objs, [13] * n, crc=True, expect=expect)
        for i, (st, page, crc) in enumerate(got):
            if n > 2 and i == n - 1:
                assert (st, page, crc) == (E.ECRC, bytes(13), bytes(4)), (n, i)
            else:
                assert (st, page, crc) == (E.OK, plains[i], orc.checksum(plains[i], hw=True)), (n, i)
                assert eng.load_info[i][2:] == (32, expect[i]), (n, i)


def test_in_turn_with_unwrap_and_load_batch(eng, dkeys):
    """jfsx_load_objects shares the RSA workspace with
    jfsx_rsa_oaep_decrypt_batch and the load path's buffers with
    jfsx_load_batch: each in turn on one context, twice."""
    plains, objs = _small_objects(E.CHACHA20P1305, KEY_A)
    plains, objs = plains[:40], list(objs[:40])
    cases = M.case_set(KEY_A)[:70]
    images = []
    for i in range(5):
        key, nonce = orc.gen_key(SEED, 2000 + i)
        c, tag = orc.seal(orc.CHACHA20P1305, key, nonce, orc.lz4_compress(plains[i]))
        images.append((key, nonce, c, tag))
    for _ in range(2):
        got = eng.load_objects(dkeys[KEY_A], E.CHACHA20P1305, E.CODEC_LZ4, objs, [13] * 40, crc=True)
        assert [(st, p) for st, p, _ in got] == [(E.OK, p) for p in plains]
        assert eng.oaep_decrypt_batch(dkeys[KEY_A], [c.ct for c in cases]) == [c.expect for c in cases]
        assert [(st, p) for st, p, _ in eng.load(E.CHACHA20P1305, E.CODEC_LZ4, images, [13] * 5)] == \
            [(E.OK, p) for p in plains[:5]]


def test_key_of_another_fixed_key_fails_every_block(eng, dkeys):
    """Objects wrapped under KEY_A, loaded with KEY_B's handle: EKEY, and
    nothing of them comes out."""
    plains, objs = _small_objects(E.AES256GCM, KEY_A)
    objs = list(objs[:5])
    assert all(unwrap(KEY_B, o[0][3:259]) is None for o in objs)
    got = eng.load_objects(dkeys[KEY_B], E.AES256GCM, E.CODEC_LZ4, objs, [13] * 5, crc=True)
    assert got == [(E.EKEY, bytes(13), bytes(4))] * 5
    assert [i[2] for i in eng.load_info] == [-1] * 5


# ---------------------------------------------------------------------------
# compress.load_objects_fused against load_blocks_fused and load_blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cipher", ["aes256gcm-rsa", "chacha20-rsa"], ids=["gcm", "chacha"])
@pytest.mark.parametrize("name", ["none", "lz4", "zstd"])
def test_load_objects_fused_mirrors_the_separate_paths(eng, name, cipher):
    from juicefs_amd import checksum as CK
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as EN
    comp = C.NewCompressor(name, eng)
    coded = name != "none"
    codec = {"none": E.CODEC_NONE, "lz4": E.CODEC_LZ4, "zstd": E.CODEC_ZSTD}[name]
    raw = EN.MemStorage()
    enc = EN.NewDataEncryptor(EN.NewRSAEncryptor(EN.GenerateRsaKey(2048)), cipher, eng)
    store = EN.NewEncrypted(raw, enc)
    blocks = [lz4_data.sample(k, n, seed=70 + i) for i, (k, n) in
              enumerate([("text", 1 << 20), ("random", 70000), ("zeros", 32768), ("runs", 12345), ("text", 5)])]
    keys = ["chunks/0/0/%d_0_%d" % (i, len(b)) for i, b in enumerate(blocks)]
    lens = [len(b) for b in blocks]
    for k, b in zip(keys, blocks):
        store.Put(k, _compress(codec, b))
    sums = [orc.object_checksum(raw.Get(k), hw=True) for k in keys]

    def old(ks=keys, ns=lens):
        if coded:
            return C.load_blocks_fused(raw, ks, ns, comp, enc=enc)
        pages = C.load_blocks(store, ks, ns, comp)
        return pages, [orc.checksum(p, hw=True) for p in pages]

    def new(ks=keys, ns=lens, cs=None):
        return C.load_objects_fused(raw, ks, ns, comp, enc, object_checksums=cs)

    def message(fn):
        with pytest.raises((C.CompressError, EN.EncryptError, CK.ChecksumVerifyError)) as ei:
            fn()
        return type(ei.value), str(ei.value)

    want = old()
    assert want[0] == blocks
    assert new() == want and new(cs=sums) == want
    assert C.load_objects_fused(raw, keys, lens, comp, enc, checksums=False, object_checksums=sums) == blocks
    # a block that comes out short of its length
    store.Put(keys[3], _compress(codec, blocks[3][:-1]))
    a = message(old)
    assert a == message(new) == (C.CompressError, "read %s fully: None (12344 < 12345)" % keys[3])
    store.Put(keys[3], _compress(codec, blocks[3]))
    # one flipped byte of the stored bytes: the tag without the store's checksum, the checksum with it
    good = raw.Get(keys[1])
    obj = bytearray(good)
    obj[len(obj) // 2] ^= 0x40
    raw.Put(keys[1], bytes(obj))
    a = message(lambda: old(keys[:3], lens[:3]))
    assert a == message(lambda: new(keys[:3], lens[:3]))
    assert a[0] is EN.EncryptError and "message authentication failed" in a[1]
    a = message(lambda: new(keys[:3], lens[:3], sums[:3]))
    cs_store = CK.ChecksumStorage(raw, eng=eng)
    cs_store.meta = dict(zip(keys, sums))
    assert a == message(lambda: cs_store.Get(keys[1]))
    assert a[0] is CK.ChecksumVerifyError
    # a wrapped key that does not unwrap; a header that does not describe itself
    obj = bytearray(good)
    obj[50] ^= 1
    raw.Put(keys[1], bytes(obj))
    a = message(lambda: old(keys[:3], lens[:3]))
    assert a == message(lambda: new(keys[:3], lens[:3])) == \
        (EN.EncryptError, "Decrypt: decryt key: crypto/rsa: decryption error")
    raw.Put(keys[1], good)
    raw.Put(keys[4], bytes([0xFF, 0xFF]) + raw.Get(keys[4])[2:])  # klen 65535 in an object of 300 bytes
    a = message(lambda: old(keys[2:], lens[2:]))
    assert a == message(lambda: new(keys[2:], lens[2:])) == \
        (EN.EncryptError, "Decrypt: misformed ciphertext: 65535 12")
