"""CPU pin of the one-call block store's contract: jfsx_sblk's layout, header
against binding; the per-block verdict (juicefs_amd/csrc/jfsx_store.h, the host
build of what store_verdict_k runs on the GPU); the export; and the argument
errors jfsx_store_batch rejects before it touches a device."""
import ctypes
import itertools
import os
import subprocess

import pytest

from juicefs_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "store_verdict_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("store") / "store_verdict_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.store_verdict.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32,
                                ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int64)]
    L.store_verdict.restype = None
    return L


def _verdict(L, vst, seg, got, exp, cst, cout, cap):
    out = (ctypes.c_int64 * 5)(*([1 << 40] * 5))
    L.store_verdict(vst, seg, got, exp, cst, cout, cap, out)
    return tuple(out)


def test_sblk_layout_header_vs_binding(host):
    out = (ctypes.c_uint64 * 24)()
    k = host.sblk_layout(out, 24)
    names = ["key", "nonce", "reserved", "tag", "src", "len", "dst", "dst_cap", "crc", "hdr", "hdr_len", "obj_crc",
             "out_len", "status", "crc_bad_seg", "crc_got", "crc_expect"]
    assert k == 1 + len(names)
    assert [f for f, _ in E.jfsx_sblk._fields_] == names
    assert ctypes.sizeof(E.jfsx_sblk) == out[0] == 144
    for i, f in enumerate(names):
        assert getattr(E.jfsx_sblk, f).offset == out[1 + i], f
    # key[32] nonce[12] u32 | tag[16] | src len dst dst_cap crc hdr | hdr_len obj_crc | out_len | status ...
    assert (E.jfsx_sblk.tag.offset, E.jfsx_sblk.src.offset, E.jfsx_sblk.hdr_len.offset, E.jfsx_sblk.out_len.offset,
            E.jfsx_sblk.status.offset) == (48, 64, 112, 120, 128)


def _bounds(n):
    """jfsx.h: LZ4_compressBound and ZSTD_compressBound, written out here."""
    return n + n // 255 + 16, n + (n >> 8) + ((((128 << 10) - n) >> 11) if n < (128 << 10) else 0)


@pytest.mark.parametrize("n", [0, 1, 32768, (4 << 20) - 1])
def test_verdict_cross_product(host, n):
    """verify status x compressor out_len: a failed verify wins and reports
    nothing of the compressor; a passed one hands on the compressor's length,
    which must lie in [1, bound(len)]."""
    broken = host.store_broken()
    assert broken not in (E.OK, E.ECRC)
    for cap in _bounds(n):
        outs = sorted({0, 1, 9, n // 2 + 1, cap - 1, cap, cap + 1})
        for vst, cst, cout in itertools.product((E.OK, E.ECRC), (E.OK, E.EFORMAT), outs):
            seg, got, exp = (3, 0xDEADBEEF, 0x01020304) if vst != E.OK else (-1, 0, 0)
            r = _verdict(host, vst, seg, got, exp, cst, cout, cap)
            if vst != E.OK:
                assert r == (E.ECRC, 0, 3, 0xDEADBEEF, 0x01020304), (n, cap, cst, cout)
            elif cst != E.OK or cout == 0 or cout > cap:
                assert r == (broken, 0, -1, 0, 0), (n, cap, cst, cout)
            else:
                assert r == (E.OK, cout, -1, 0, 0), (n, cap, cst, cout)


def test_verdict_rows(host):
    # the gated compressor of a failed block reports the sink's 1 (LZ4) or 9 (zstd) bytes: never handed on
    assert _verdict(host, E.ECRC, 0, 7, 8, E.OK, 1, 16) == (E.ECRC, 0, 0, 7, 8)
    assert _verdict(host, E.ECRC, 127, 7, 8, E.OK, 9, 16) == (E.ECRC, 0, 127, 7, 8)
    # the empty page: a 1-byte LZ4 block, a 9-byte zstd frame
    assert _verdict(host, E.OK, -1, 0, 0, E.OK, 1, 16) == (E.OK, 1, -1, 0, 0)
    assert _verdict(host, E.OK, -1, 0, 0, E.OK, 9, 64) == (E.OK, 9, -1, 0, 0)
    # a record the compressor never wrote (the gate's initial value) is not a length
    assert _verdict(host, E.OK, -1, 0, 0, E.EFORMAT, 0, 4096)[0] == host.store_broken()


def test_library_exports_store_batch():
    L = E.load_library()
    assert "jfsx_store_batch" in E.EXPORTS
    assert L.jfsx_store_batch.argtypes[4] == ctypes.POINTER(E.jfsx_sblk)
    assert E.load_library().jfsx_abi_version() == 9


def test_argument_errors_touch_no_device():
    """NULL context, and every bad algo / codec / crc_mode / mem with a block
    record in hand: JFSX_EINVAL with nothing written (the context here is not a
    context: it would fault if it were used)."""
    L = E.load_library()
    args = (E.AES256GCM, E.CODEC_LZ4, E.CRC_GEN, E.MEM_HOST)
    assert L.jfsx_store_batch(None, args[0], args[1], 0, None, args[2], args[3]) == E.EINVAL
    src = bytearray(b"x" * 100)
    sbuf = (ctypes.c_uint8 * 100).from_buffer(src)
    dst = (ctypes.c_uint8 * 256)(*([0xA5] * 256))
    crc = (ctypes.c_uint8 * 4)(*([0xA5] * 4))

    def blk():
        arr, n = E.Engine.make_sblocks([{"key": bytes(32), "nonce": bytes(12), "src": ctypes.addressof(sbuf),
                                         "len": 100, "dst": ctypes.addressof(dst), "dst_cap": 256,
                                         "crc": ctypes.addressof(crc)}])
        arr[0].status, arr[0].out_len = 77, 78
        return arr

    fake = ctypes.c_void_p(16)  # never dereferenced: the arguments are checked first
    bad = [(2, args[1], args[2], args[3]), (-2, args[1], args[2], args[3]),
           (args[0], 0, args[2], args[3]), (args[0], 3, args[2], args[3]),
           (args[0], args[1], E.CRC_GEN | E.CRC_VERIFY, args[3]),
           (args[0], args[1], E.CRC_GEN | E.CRC_VERIFY | E.CRC_CT, args[3]),
           (args[0], args[1], E.CRC_GEN | E.CRC_BOTH, args[3]), (args[0], args[1], 16, args[3]),
           (args[0], args[1], -1, args[3]), (args[0], args[1], args[2], 2)]
    for algo, codec, mode, mem in bad:
        arr = blk()
        assert L.jfsx_store_batch(fake, algo, codec, 1, arr, mode, mem) == E.EINVAL, (algo, codec, mode, mem)
        assert (arr[0].status, arr[0].out_len) == (77, 78)
    # per-block rules: reserved, dst_cap below the codec's bound, a missing CRC array
    for field, value, codec in (("reserved", 1, E.CODEC_LZ4), ("dst_cap", int(E.lz4_bound(100)) - 1, E.CODEC_LZ4),
                                ("dst_cap", int(E.zstd_bound(100)) - 1, E.CODEC_ZSTD), ("crc", None, E.CODEC_LZ4),
                                ("dst", None, E.CODEC_LZ4), ("len", 0x7E000001, E.CODEC_LZ4)):
        arr = blk()
        setattr(arr[0], field, value)
        assert L.jfsx_store_batch(fake, E.AES256GCM, codec, 1, arr, E.CRC_GEN, E.MEM_HOST) == E.EINVAL, field
        assert (arr[0].status, arr[0].out_len) == (77, 78)
    assert bytes(dst) == b"\xa5" * 256 and bytes(crc) == b"\xa5" * 4
