"""CPU pin of the one-call object load's contract: jfsx_oblk's layout, header
against binding; the export; the argument errors jfsx_load_objects rejects
before it touches a context; the per-block verdict and the checksum fold of
juicefs_amd/csrc/jfsx_objload.h, the host build of what obj_verdict_k and
obj_fold_k run on the GPU."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "objload_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("objload") / "objload_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.object_verdict.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int32,
                                 ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                 ctypes.POINTER(ctypes.c_int64)]
    L.object_verdict.restype = None
    L.reported_key_len.argtypes = [ctypes.c_uint32, ctypes.c_int32]
    L.reported_key_len.restype = ctypes.c_int32
    L.obj_fold.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.obj_fold.restype = ctypes.c_uint32
    return L


def _flags(L):
    f = (ctypes.c_uint32 * 3)()
    L.obj_flags(f)
    return tuple(f)


def test_oblk_layout_header_vs_binding(host):
    out = (ctypes.c_uint64 * 24)()
    k = host.oblk_layout(out, 24)
    names = ["hdr", "hdr_len", "reserved", "tag", "src", "src_len", "dst", "len", "crc", "expect_crc", "obj_crc",
             "out_len", "status", "codec_info", "key_len", "reserved2"]
    assert k == 1 + len(names)
    assert [f for f, _ in E.jfsx_oblk._fields_] == names
    assert ctypes.sizeof(E.jfsx_oblk) == out[0] == 104
    for i, f in enumerate(names):
        assert getattr(E.jfsx_oblk, f).offset == out[1 + i], f
    # hdr | hdr_len reserved | tag[16] | src src_len dst len crc | expect obj | out_len | status info key_len r2
    assert (E.jfsx_oblk.tag.offset, E.jfsx_oblk.src.offset, E.jfsx_oblk.expect_crc.offset,
            E.jfsx_oblk.out_len.offset, E.jfsx_oblk.status.offset) == (16, 32, 72, 80, 88)
    c = (ctypes.c_int * 4)()
    assert host.obj_constants(c) == 4
    assert tuple(c) == (E.CODEC_NONE, E.EKEY, E.EHEADER, 9) == (0, 7, 8, 9)


def test_library_exports_load_objects():
    L = E.load_library()
    assert "jfsx_load_objects" in E.EXPORTS
    assert L.jfsx_load_objects.argtypes[5] == ctypes.POINTER(E.jfsx_oblk)
    assert L.jfsx_abi_version() == 9


def test_argument_errors_touch_no_context():
    """Every argument error with a context and a key that are not what they
    claim to be (they would fault if they were used): JFSX_EINVAL, the record
    and the buffers unchanged."""
    L = E.load_library()
    hdr = (ctypes.c_uint8 * 271)(*([1, 0, 12] + [7] * 268))
    src = (ctypes.c_uint8 * 112)(*([0x5A] * 112))
    dst = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
    crc = (ctypes.c_uint8 * 4)(*([0xA5] * 4))
    fake, fkey = ctypes.c_void_p(16), ctypes.c_void_p(32)

    def blk(cipher=True, length=100):
        arr, _ = E.Engine.make_oblocks([{"hdr": ctypes.addressof(hdr) if cipher else None,
                                         "hdr_len": 271 if cipher else 0, "tag": bytes(16),
                                         "src": ctypes.addressof(src), "src_len": 100, "dst": ctypes.addressof(dst),
                                         "len": length, "crc": ctypes.addressof(crc), "expect_crc": 5}])
        b = arr[0]
        b.status, b.out_len, b.obj_crc, b.key_len, b.codec_info = 77, 78, 79, 80, 81
        return arr

    def untouched(arr):
        b = arr[0]
        return (b.status, b.out_len, b.obj_crc, b.key_len, b.codec_info) == (77, 78, 79, 80, 81)

    A, Z, G, H = E.AES256GCM, E.CODEC_LZ4, E.CRC_GEN, E.MEM_HOST
    assert L.jfsx_load_objects(None, fkey, A, Z, 0, None, G, H) == E.EINVAL
    assert L.jfsx_load_objects(fake, fkey, A, Z, 1, None, G, H) == E.EINVAL
    bad = [(fkey, 2, Z, G, H), (fkey, -2, Z, G, H), (fkey, A, 3, G, H), (fkey, A, -1, G, H),
           (fkey, A, Z, E.CRC_VERIFY, H), (fkey, A, Z, E.CRC_GEN | E.CRC_VERIFY, H), (fkey, A, Z, E.CRC_GEN | E.CRC_BOTH, H),
           (fkey, A, Z, 16, H), (fkey, A, Z, -1, H), (fkey, A, Z, G, 2), (fkey, A, Z, G, -1),
           (None, A, Z, G, H)]  # a cipher needs the key
    for key, algo, codec, mode, mem in bad:
        arr = blk()
        assert L.jfsx_load_objects(fake, key, algo, codec, 1, arr, mode, mem) == E.EINVAL, (algo, codec, mode, mem)
        assert untouched(arr)
    assert L.jfsx_load_objects(fake, fkey, A, Z, -1, blk(), G, H) == E.EINVAL
    # without a cipher: no key, no header, and a codec
    for key, codec, cipher in ((fkey, Z, False), (None, Z, True), (None, E.CODEC_NONE, False)):
        arr = blk(cipher)
        assert L.jfsx_load_objects(fake, key, E.CIPHER_NONE, codec, 1, arr, G, H) == E.EINVAL, (key, codec, cipher)
        assert untouched(arr)
    # JFSX_CODEC_NONE: the image is the page
    arr = blk(length=99)
    assert L.jfsx_load_objects(fake, fkey, A, E.CODEC_NONE, 1, arr, G, H) == E.EINVAL
    assert untouched(arr)
    # per-block rules
    for field, value, codec, mem in (("reserved", 1, Z, H), ("hdr", None, Z, H), ("src", None, Z, H),
                                     ("dst", None, Z, H), ("crc", None, Z, H), ("src_len", 0x7E000001, Z, H),
                                     ("len", 1 << 32, Z, H), ("len", 1 << 31, E.CODEC_ZSTD, H),
                                     ("src", ctypes.addressof(src) + 1, Z, E.MEM_DEVICE),
                                     ("dst", ctypes.addressof(dst) + 1, Z, E.MEM_DEVICE),
                                     ("dst", ctypes.addressof(src), Z, E.MEM_DEVICE)):
        arr = blk()
        setattr(arr[0], field, value)
        assert L.jfsx_load_objects(fake, fkey, A, codec, 1, arr, G | E.CRC_CT, mem) == E.EINVAL, (field, value)
        assert untouched(arr)
    # device memory without a codec: Open writes the page, so it is aligned even with no page CRC
    arr = blk()
    arr[0].dst = ctypes.addressof(dst) + 1
    assert L.jfsx_load_objects(fake, fkey, A, E.CODEC_NONE, 1, arr, E.CRC_NONE, E.MEM_DEVICE) == E.EINVAL
    # n == 0 is a no-op that touches nothing
    assert L.jfsx_load_objects(fake, fkey, A, Z, 0, None, G, H) == 0
    assert bytes(dst) == b"\xa5" * 256 and bytes(crc) == b"\xa5" * 4 and bytes(src) == b"\x5a" * 112


def _expected(crc_ct, crc_bad, cipher, hdr_bad, key_bad, key_len, nonce_bad, ost, dst, dout, n):
    """The table of include/jfsx.h, written out: the first rule that applies."""
    if crc_ct and crc_bad:
        return (E.ECRC, 0)
    if cipher:
        if hdr_bad:
            return (E.EHEADER, 0)
        if key_bad or key_len != 32:
            return (E.EKEY, 0)
        if nonce_bad or ost != E.OK:
            return (E.ETAG, 0)
    if dst != E.OK:
        return (dst, 0)
    if dout < n:
        return (E.ESHORT, dout)
    return (E.OK, n)


@pytest.mark.parametrize("n", [0, 1, 32768])
def test_object_verdict_cross_product(host, n):
    HB, KB, NB = _flags(host)
    assert sorted((HB, KB, NB)) == [1, 2, 4]
    out = (ctypes.c_int64 * 2)()
    seen = set()
    outs = sorted({0, max(n - 1, 0), n, n + 1})
    for crc_ct, crc_bad, cipher, hb, kb, kl, nb, ost, dst, dout in itertools.product(
            (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (-1, 0, 31, 32, 33), (0, 1), (E.OK, E.ETAG),
            (E.OK, E.EFORMAT, E.EDSTSIZE), outs):
        flags = (HB if hb else 0) | (KB if kb else 0) | (NB if nb else 0)
        host.object_verdict(crc_ct, crc_bad, cipher, flags, kl, ost, dst, dout, n, out)
        want = _expected(crc_ct, crc_bad, cipher, hb, kb, kl, nb, ost, dst, dout, n)
        assert tuple(out) == want, (crc_ct, crc_bad, cipher, hb, kb, kl, nb, ost, dst, dout)
        seen.add(want[0])
    assert seen == {E.OK, E.ECRC, E.EHEADER, E.EKEY, E.ETAG, E.EFORMAT, E.EDSTSIZE} | ({E.ESHORT} if n else set())


def test_verdict_rows_and_key_len(host):
    HB, KB, NB = _flags(host)
    out = (ctypes.c_int64 * 2)()

    def v(*a):
        host.object_verdict(*a, out)
        return tuple(out)

    # a checksum mismatch hides everything behind it, but only in a batch that verifies
    assert v(1, 1, 1, HB | KB | NB, -1, E.ETAG, E.EFORMAT, 0, 9) == (E.ECRC, 0)
    assert v(0, 1, 1, HB | KB | NB, -1, E.ETAG, E.EFORMAT, 0, 9) == (E.EHEADER, 0)
    # a flipped tag with the checksum right, or not asked for
    assert v(1, 0, 1, 0, 32, E.ETAG, E.OK, 9, 9) == (E.ETAG, 0)
    # without a cipher the cipher's rules cannot apply: what is left is jfsx_load_batch's table
    assert v(0, 0, 0, HB | KB | NB, 0, E.ETAG, E.OK, 9, 9) == (E.OK, 9)
    assert v(1, 0, 0, 0, 0, E.OK, E.OK, 8, 9) == (E.ESHORT, 8)
    # the length the record reports: -1 for the size check, 0 where the header names no key
    assert host.reported_key_len(0, 32) == 32 and host.reported_key_len(0, 31) == 31
    assert host.reported_key_len(0, -1) == -1 and host.reported_key_len(NB, 33) == 33
    assert host.reported_key_len(KB, 32) == -1 and host.reported_key_len(HB | KB, 32) == 0


_rng = np.random.default_rng(0x0B1)
_C = _rng.integers(0, 256, (4 << 20) - 1, dtype=np.uint8).tobytes()
_HDR = _rng.integers(0, 256, 271, dtype=np.uint8).tobytes()
_TAG = _rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
C_LENGTHS = [0, 1, 32767, 32768, 32769, 2 << 20, (2 << 20) + 1, (4 << 20) - 1]


@pytest.mark.parametrize("hlen", [0, 270, 271])
@pytest.mark.parametrize("clen", C_LENGTHS)
def test_fold_as_64_lanes_equals_object_checksum(host, clen, hlen):
    """hdr || C || tag as a cipher stores it, and C alone as a volume without
    one does (tail 0, no header): the fold of C's segment CRCs against
    CRC32C of the whole object."""
    c, hdr = _C[:clen], _HDR[:hlen]
    segs = np.frombuffer(orc.checksum(c, hw=True), np.uint8).copy()
    assert segs.size == 4 * max(1, -(-clen // E.SEG))
    assert -(-clen // E.SEG) == {2 << 20: 64, (2 << 20) + 1: 65}.get(clen, -(-clen // E.SEG))
    got = host.obj_fold(segs.ctypes.data, clen, 16, orc.crc32c(hdr), orc.crc32c(_TAG))
    assert got == int(orc.object_checksum(hdr + c + _TAG, hw=True))
    if hlen == 0:
        assert host.obj_fold(segs.ctypes.data, clen, 0, 0, 0) == int(orc.object_checksum(c, hw=True))
