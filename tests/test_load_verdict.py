"""CPU pin of the one-call block load's per-block verdict
(juicefs_amd/csrc/jfsx_load.h, the host build of what load_verdict_k runs on
the GPU) and of jfsx_lblk's layout, header against binding."""
import ctypes
import itertools
import os
import subprocess

import pytest

from juicefs_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "load_verdict_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("load") / "load_verdict_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.load_verdict.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    L.load_verdict.restype = None
    return L


def _verdict(L, ost, dst, out, n):
    st, ol = ctypes.c_int32(-1), ctypes.c_uint64(1 << 60)
    L.load_verdict(ost, dst, out, n, ctypes.byref(st), ctypes.byref(ol))
    return st.value, ol.value


def _expect(ost, dst, out, n):
    """The table of include/jfsx.h, the first rule that applies."""
    if ost != E.OK:
        return E.ETAG, 0
    if dst != E.OK:
        return dst, 0
    if out < n:
        return E.ESHORT, out
    return E.OK, n


@pytest.mark.parametrize("n", [1, 13, 32768, (4 << 20) - 1, (1 << 32) - 1])
def test_verdict_cross_product(host, n):
    for ost, dst, out in itertools.product((E.OK, E.ETAG), (E.OK, E.EFORMAT, E.EDSTSIZE), (0, n - 1, n)):
        assert _verdict(host, ost, dst, out, n) == _expect(ost, dst, out, n), (ost, dst, out, n)


def test_verdict_rows(host):
    n = 4096
    # a failed tag wins over whatever the (gated) decoder reported
    assert _verdict(host, E.ETAG, E.OK, n, n) == (E.ETAG, 0)
    assert _verdict(host, E.ETAG, E.EFORMAT, 0, n) == (E.ETAG, 0)
    # a rejected image reports no bytes, whatever ZOut.out_len held
    assert _verdict(host, E.OK, E.EFORMAT, n - 1, n) == (E.EFORMAT, 0)
    assert _verdict(host, E.OK, E.EDSTSIZE, n, n) == (E.EDSTSIZE, 0)
    # "read %s fully": n < len keeps n
    assert _verdict(host, E.OK, E.OK, n - 7, n) == (E.ESHORT, n - 7)
    assert _verdict(host, E.OK, E.OK, 0, n) == (E.ESHORT, 0)
    assert _verdict(host, E.OK, E.OK, n, n) == (E.OK, n)
    # the empty page: nothing to decode is a full read
    assert _verdict(host, E.OK, E.OK, 0, 0) == (E.OK, 0)
    assert _verdict(host, E.ETAG, E.OK, 0, 0) == (E.ETAG, 0)


def test_lblk_layout_header_vs_binding(host):
    out = (ctypes.c_uint64 * 16)()
    k = host.lblk_layout(out, 16)
    names = ["key", "nonce", "reserved", "tag", "src", "src_len", "dst", "len", "crc", "out_len", "status",
             "codec_info"]
    assert k == 1 + len(names)
    assert [f for f, _ in E.jfsx_lblk._fields_] == names
    assert ctypes.sizeof(E.jfsx_lblk) == out[0] == 120
    for i, f in enumerate(names):
        assert getattr(E.jfsx_lblk, f).offset == out[1 + i], f
    # key[32] nonce[12] u32 | tag[16] | src src_len dst len crc out_len | status codec_info
    assert (E.jfsx_lblk.tag.offset, E.jfsx_lblk.src.offset, E.jfsx_lblk.status.offset) == (48, 64, 112)


def test_constants_header_vs_binding(host):
    out = (ctypes.c_int * 4)()
    assert host.load_constants(out) == 4
    assert list(out) == [E.CIPHER_NONE, E.CODEC_LZ4, E.CODEC_ZSTD, E.ESHORT]


def test_library_exports_load_batch():
    L = E.load_library()
    assert "jfsx_load_batch" in E.EXPORTS
    assert L.jfsx_load_batch.argtypes[4] == ctypes.POINTER(E.jfsx_lblk)
    # argument errors are rejected before any device is touched
    assert L.jfsx_load_batch(None, E.AES256GCM, E.CODEC_LZ4, 0, None, E.CRC_NONE, E.MEM_HOST) == E.EINVAL
