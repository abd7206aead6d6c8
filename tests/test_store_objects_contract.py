"""CPU pin of the one-call object store's contract: jfsx_soblk's layout, header
against binding; the exports; jfsx_object_bound against its formula; the
argument errors jfsx_store_objects rejects before it touches a context or a
key; the frame and the checksum fold of juicefs_amd/csrc/jfsx_objstore.h, the
host build of what sobj_frame_k runs on the GPU, as 64 emulated lanes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "objstore_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("objstore") / "objstore_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    P = ctypes.c_void_p
    L.sobj_frame.argtypes = [P, P, P, P, ctypes.c_uint64]
    L.sobj_frame.restype = None
    L.sobj_span_crc.argtypes = [P, ctypes.c_uint32]
    L.sobj_span_crc.restype = ctypes.c_uint32
    L.sobj_hdr_crc.argtypes = [P, P]
    L.sobj_hdr_crc.restype = ctypes.c_uint32
    L.sobj_object_crc.argtypes = [P, P, P, ctypes.c_uint64, P]
    L.sobj_object_crc.restype = ctypes.c_uint32
    return L


def test_soblk_layout_header_vs_binding(host):
    out = (ctypes.c_uint64 * 24)()
    k = host.soblk_layout(out, 24)
    names = ["key", "nonce", "reserved", "seed", "src", "len", "obj", "obj_cap", "crc", "out_len", "img_len",
             "obj_crc", "status", "crc_bad_seg", "crc_got", "crc_expect", "reserved2"]
    assert k == 1 + len(names)
    assert [f for f, _ in E.jfsx_soblk._fields_] == names
    assert ctypes.sizeof(E.jfsx_soblk) == out[0] == 160
    for i, f in enumerate(names):
        assert getattr(E.jfsx_soblk, f).offset == out[1 + i], f
    # key nonce reserved | seed | src len obj obj_cap crc | out_len img_len | obj_crc status seg got expect r2
    assert (E.jfsx_soblk.seed.offset, E.jfsx_soblk.src.offset, E.jfsx_soblk.out_len.offset,
            E.jfsx_soblk.obj_crc.offset, E.jfsx_soblk.reserved2.offset) == (48, 80, 120, 136, 156)
    c = (ctypes.c_int * 5)()
    assert host.sobj_constants(c) == 5
    assert tuple(c) == (E.OBJ_HDR_BYTES, E.OBJ_TAG_BYTES, 271, 16, 9)


def test_library_exports_store_objects():
    L = E.load_library()
    assert "jfsx_store_objects" in E.EXPORTS and "jfsx_object_bound" in E.EXPORTS
    assert L.jfsx_store_objects.argtypes[6] == ctypes.POINTER(E.jfsx_soblk)
    assert L.jfsx_abi_version() == 9


@pytest.mark.parametrize("n", [0, 1, 32768, (4 << 20) - 1])
def test_object_bound(n):
    assert E.object_bound(E.CODEC_NONE, n) == 271 + n + 16
    assert E.object_bound(E.CODEC_LZ4, n) == 271 + (n + n // 255 + 16) + 16 == 287 + E.lz4_bound(n)
    zb = n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)
    assert E.object_bound(E.CODEC_ZSTD, n) == 271 + zb + 16 == 287 + E.zstd_bound(n)
    assert E.object_bound(3, n) == 0 and E.object_bound(-1, n) == 0


def test_argument_errors_touch_no_context():
    """Every argument error with a context and a key that are not what they
    claim to be (they would fault if they were used): JFSX_EINVAL, the record
    and the buffers unchanged."""
    L = E.load_library()
    src = np.full(128, 0x5A, np.uint8)
    obj = np.full(1024, 0xA5, np.uint8)
    crc = np.full(4, 0xA5, np.uint8)
    fake, fkey = ctypes.c_void_p(16), ctypes.c_void_p(32)
    sp = (src.ctypes.data + 15) & ~15
    op = ((obj.ctypes.data + 15) & ~15) + 1  # 1 mod 16: right for both memory modes

    def blk(length=100, codec=E.CODEC_LZ4):
        arr, _ = E.Engine.make_soblocks([{"key": bytes(32), "nonce": bytes(12), "seed": bytes(32), "src": sp,
                                          "len": length, "obj": op, "obj_cap": E.object_bound(codec, length),
                                          "crc": crc.ctypes.data}])
        b = arr[0]
        b.status, b.out_len, b.img_len, b.obj_crc, b.crc_bad_seg = 77, 78, 79, 80, 81
        return arr

    def untouched(arr):
        b = arr[0]
        return (b.status, b.out_len, b.img_len, b.obj_crc, b.crc_bad_seg) == (77, 78, 79, 80, 81)

    A, Z, G, H, e = E.AES256GCM, E.CODEC_LZ4, E.CRC_GEN, E.MEM_HOST, 65537
    call = L.jfsx_store_objects
    assert call(None, fkey, e, A, Z, 0, None, G, H) == E.EINVAL
    assert call(fake, fkey, e, A, Z, 1, None, G, H) == E.EINVAL
    bad = [(fkey, e, E.CIPHER_NONE, Z, G, H),  # without a cipher the object is the image
           (fkey, e, 2, Z, G, H), (fkey, e, -2, Z, G, H), (fkey, e, A, 3, G, H), (fkey, e, A, -1, G, H),
           (fkey, e, A, Z, E.CRC_GEN | E.CRC_VERIFY, H), (fkey, e, A, Z, E.CRC_GEN | E.CRC_BOTH, H),
           (fkey, e, A, Z, 16, H), (fkey, e, A, Z, -1, H), (fkey, e, A, Z, G, 2), (fkey, e, A, Z, G, -1),
           (None, e, A, Z, G, H),  # a null key
           (fkey, 0, A, Z, G, H), (fkey, 1, A, Z, G, H), (fkey, 1 << 31, A, Z, G, H)]  # e out of Go's checkPub range
    for key, ee, algo, codec, mode, mem in bad:
        arr = blk()
        assert call(fake, key, ee, algo, codec, 1, arr, mode, mem) == E.EINVAL, (ee, algo, codec, mode, mem)
        assert untouched(arr)
    assert call(fake, fkey, e, A, Z, -1, blk(), G, H) == E.EINVAL
    # per-block rules
    for field, value, codec, mode, mem in (
            ("reserved", 1, Z, G, H), ("reserved2", 1, Z, G, H), ("src", None, Z, G, H), ("obj", None, Z, G, H),
            ("crc", None, Z, G, H), ("crc", None, Z, E.CRC_VERIFY | E.CRC_CT, H),
            ("obj_cap", E.object_bound(Z, 100) - 1, Z, G, H),
            ("obj_cap", E.object_bound(E.CODEC_ZSTD, 100) - 1, E.CODEC_ZSTD, G, H),
            ("obj_cap", 286 + 100, E.CODEC_NONE, G, H),
            ("len", 0x7E000001, Z, G, H),  # the compressors' limit
            ("obj", op - 1, Z, G, E.MEM_DEVICE), ("obj", op + 1, Z, G, E.MEM_DEVICE),
            ("obj", op + 7, Z, G, E.MEM_DEVICE),
            ("src", sp + 1, Z, G, E.MEM_DEVICE),  # the page CRC reads it
            ("src", sp + 1, E.CODEC_NONE, E.CRC_NONE, E.MEM_DEVICE)):  # the Seal reads it
        arr = blk(codec=codec)
        setattr(arr[0], field, value)
        assert call(fake, fkey, e, A, codec, 1, arr, mode, mem) == E.EINVAL, (field, value)
        assert untouched(arr)
    # the ciphers' own limits without a codec: GCM's 32-bit counter
    arr = blk(codec=E.CODEC_NONE)
    arr[0].len, arr[0].obj_cap = 1 << 36, (1 << 36) + 287
    assert call(fake, fkey, e, A, E.CODEC_NONE, 1, arr, G, H) == E.EINVAL
    # obj == src in device memory
    arr = blk()
    arr[0].src = op
    assert call(fake, fkey, e, A, Z, 1, arr, E.CRC_NONE, E.MEM_DEVICE) == E.EINVAL
    # n == 0 is a no-op that touches nothing
    assert call(fake, fkey, e, A, Z, 0, None, G, H) == 0
    assert (src == 0x5A).all() and (obj == 0xA5).all() and (crc == 0xA5).all()


_rng = np.random.default_rng(0x50B1)
_C = _rng.integers(0, 256, (4 << 20) - 1, dtype=np.uint8).tobytes()
_W = _rng.integers(0, 256, 256, dtype=np.uint8)
_N = _rng.integers(0, 256, 12, dtype=np.uint8)
_T = _rng.integers(0, 256, 16, dtype=np.uint8)
_HDR = bytes([1, 0, 12]) + _W.tobytes() + _N.tobytes()


def _aligned(n, mod):
    """n writable bytes at an address that is mod (mod 16), 0xA5-filled, with 16 bytes before and behind."""
    buf = np.full(n + 64, 0xA5, np.uint8)
    off = 16 + (mod - (buf.ctypes.data + 16)) % 16
    return buf, off


def test_frame_bytes_as_64_lanes(host):
    w, off = _aligned(256, 0)
    w[off:off + 256] = _W
    for clen in (0, 1, 15, 16, 17, 32769):
        buf, o = _aligned(287 + clen, 1)
        host.sobj_frame(buf.ctypes.data + o, w.ctypes.data + off, _N.ctypes.data, _T.ctypes.data, clen)
        assert buf[o:o + 271].tobytes() == bytes([1, 0, 12]) + _W.tobytes() + _N.tobytes()
        assert buf[o + 271 + clen:o + 287 + clen].tobytes() == _T.tobytes()
        assert (buf[:o] == 0xA5).all() and (buf[o + 271:o + 271 + clen] == 0xA5).all()  # C is the Seal's
        assert (buf[o + 287 + clen:] == 0xA5).all()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 16, 271, 287])
def test_span_crc_as_64_lanes(host, n):
    span = np.frombuffer((_HDR + _T.tobytes())[:n], np.uint8).copy() if n else np.zeros(1, np.uint8)
    assert host.sobj_span_crc(span.ctypes.data, n) == int(orc.object_checksum(span[:n].tobytes(), hw=True))
    if n == 271:
        w, off = _aligned(256, 0)
        w[off:off + 256] = _W
        assert host.sobj_hdr_crc(w.ctypes.data + off, _N.ctypes.data) == int(orc.object_checksum(_HDR, hw=True))


@pytest.mark.parametrize("clen", [0, 1, 32767, 32768, 32769, 65541, (1 << 20) + 3, (4 << 20) - 1])
def test_full_fold_equals_object_checksum(host, clen):
    c = _C[:clen]
    segs = np.frombuffer(orc.checksum(c, hw=True), np.uint8).copy()
    w, off = _aligned(256, 0)
    w[off:off + 256] = _W
    got = host.sobj_object_crc(w.ctypes.data + off, _N.ctypes.data, segs.ctypes.data, clen, _T.ctypes.data)
    assert got == int(orc.object_checksum(_HDR + c + _T.tobytes(), hw=True))


def test_sanitized_standalone_run(tmp_path):
    """The harness with its own main under AddressSanitizer and UBSan, as a
    stand-alone program: the same spans and image lengths against a
    bit-by-bit CRC32C of its own."""
    exe = str(tmp_path / "objstore_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "objstore_host ok" in r.stdout, (r.stdout, r.stderr)
