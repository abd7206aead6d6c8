"""Hadoop file checksum (MD5-of-MD5-of-CRC32C) on the GPU: crc_chunks_k and
md5_blocks_k through jfsx_file_checksum_batch, in device and host memory,
against the five values the reference's Java SDK test holds
(tests/golden/java_filechecksum.json) and the pure-Python model over the
oracle's CRC32C; and the fused Seal kernels' CRC bytes tied to the same
values."""
import ctypes

import numpy as np
import pytest

from juicefs_amd import checksum as C
from juicefs_amd import engine as E
from oracle import oracle as orc  # checker only
from tests import filechecksum_model as M

pytestmark = pytest.mark.gpu

BLOCK = 128 << 20
# every edge of the chunk (512), the span (4096), the 32 KiB run of a wave,
# several waves and tasks, several workgroups
LENS = [0, 1, 5, 6, 511, 512, 513, 1023, 1024, 4095, 4096, 4097, 8192, 8193, 16385, 32767, 32768, 32769,
        (1 << 20) + 777, (40 << 20) + 13]
BLOCKS = (4096, 65536)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _tuple(r):
    return ("CRC32C" if r[0] else "CRC32", r[1], r[2], r[3].hex())


# ---- the five reference values ---------------------------------------------
@pytest.fixture(scope="module")
def zeros(eng):
    """153,600,000 zero bytes, on the device and on the host"""
    host = np.zeros(150 * 1024 * 1000, np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    yield host, dev
    dev.free()


@pytest.mark.parametrize("mem", (E.MEM_DEVICE, E.MEM_HOST), ids=("device", "host"))
def test_java_values(eng, zeros, mem):
    host, dev = zeros
    lit = eng.alloc(16)
    try:
        files, want = [], []
        for case in M.golden_cases():
            assert case["block"] == BLOCK
            span = M.case_span(case)
            c = case["content"]
            if "literal" in c:
                b = np.frombuffer(c["literal"].encode("latin-1"), np.uint8)
                if mem == E.MEM_DEVICE:
                    lit.upload(b)
                files.append((lit if mem == E.MEM_DEVICE else b.copy(), span))
            else:
                assert c["zeros"] <= host.size
                files.append((dev if mem == E.MEM_DEVICE else host, span))
            want.append(M.case_expect(case))
        # one at a time, then the five in one call
        got = [_tuple(eng.file_checksum_batch([f], BLOCK, mem=mem)[0]) for f in files]
        assert got == want
        assert [_tuple(r) for r in eng.file_checksum_batch(files, BLOCK, mem=mem)] == want
    finally:
        lit.free()


# ---- the model, many files in one batch ------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """seeded random files, their chunk CRCs (oracle) and the model's answers"""
    rng = np.random.default_rng(20251)
    datas = [rng.integers(0, 256, n, dtype=np.uint8) for n in LENS]
    crcs = [M.chunk_crcs(d, orc.crc32c) for d in datas]
    want = {blk: [M.fold(c, d.size, blk) for c, d in zip(crcs, datas)] for blk in BLOCKS}
    return datas, want


@pytest.fixture(scope="module")
def corpus_dev(eng, corpus):
    datas, _ = corpus
    offs, o = [], 0
    for d in datas:
        offs.append(o)
        o += (d.size + 4095) & ~4095
    buf = eng.alloc(o)
    for d, off in zip(datas, offs):
        buf.upload(d, off)
    yield buf, offs
    buf.free()


@pytest.mark.parametrize("block", BLOCKS)
def test_device_batch_matches_model(eng, corpus, corpus_dev, block):
    datas, want = corpus
    buf, offs = corpus_dev
    files = [(buf.ptr + off, d.size) for d, off in zip(datas, offs)]
    got = [_tuple(r) for r in eng.file_checksum_batch(files, block, mem=E.MEM_DEVICE)]
    for n, g, w in zip(LENS, got, want[block]):
        assert g == w, n
    # the batch gives what the files give one at a time
    assert [_tuple(eng.file_checksum_batch([f], block, mem=E.MEM_DEVICE)[0]) for f in files] == got


@pytest.mark.parametrize("shift", (0, 1, 3))
@pytest.mark.parametrize("block", BLOCKS)
def test_host_batch_matches_model(eng, corpus, block, shift):
    datas, want = corpus
    # sources `shift` bytes into 64-byte aligned buffers
    bufs = []
    for d in datas:
        raw = np.empty(d.size + 128, np.uint8)
        a = (-raw.ctypes.data) % 64 + shift
        raw[a:a + d.size] = d
        bufs.append(raw[a:a + d.size])
        assert d.size == 0 or bufs[-1].ctypes.data % 64 == shift
    files = [(b, b.size) for b in bufs]
    got = [_tuple(r) for r in eng.file_checksum_batch(files, block, mem=E.MEM_HOST)]
    for n, g, w in zip(LENS, got, want[block]):
        assert g == w, n
    if shift == 0:
        assert [_tuple(eng.file_checksum_batch([f], block, mem=E.MEM_HOST)[0]) for f in files] == got


# ---- getFileChecksum's span rule --------------------------------------------
def test_get_file_checksum_span_cases(eng):
    data = np.random.default_rng(5).integers(0, 256, 2000, dtype=np.uint8)
    for length, span in ((5, 5), (600, 1024), (None, 2000), (2000, 2000), (0, 0)):
        got = C.getFileChecksum(data, length=length, eng=eng) if length is not None else C.getFileChecksum(data, eng=eng)
        assert isinstance(got, C.FileChecksum)
        assert tuple(got) == M.file_checksum(data[:span], orc.crc32c, BLOCK), length
    small = C.getFileChecksum(data, blocksize=512, eng=eng)
    assert tuple(small) == M.file_checksum(data, orc.crc32c, 512) and small.crcPerBlock == 1


# ---- the fused kernels' CRC bytes against the reference values --------------
@pytest.mark.parametrize("algo,flags", ((E.AES256GCM, 0), (E.AES256GCM, E.CTX_BITSLICE), (E.CHACHA20P1305, 0)),
                         ids=("gcm_ttable", "gcm_bitslice", "chacha"))
def test_fused_seal_crc_gives_the_java_values(algo, flags):
    by_name = {c["name"]: M.case_expect(c) for c in M.golden_cases()}
    e = E.Engine(0, flags)
    try:
        key, nonce = E.gen_key(11, 3)
        for text, name in ((b"world\n", "small"), (b"world", "small_length5")):
            _, _, crc = e.seal(algo, key, nonce, text, crc=True)
            assert len(crc) == 4
            assert _tuple(E.file_checksum_fold(crc, len(text), BLOCK)) == by_name[name]
    finally:
        e.close()


# ---- argument errors, metrics ----------------------------------------------
def test_argument_errors(eng):
    L = eng.L
    data = np.zeros(1024, np.uint8)
    f = (E.jfsx_fsum * 1)()
    f[0].data, f[0].len = data.ctypes.data, data.size
    for mem in (E.MEM_DEVICE, E.MEM_HOST):
        assert L.jfsx_file_checksum_batch(eng.ctx, 1, f, 256, BLOCK, mem) == E.EINVAL
        assert L.jfsx_file_checksum_batch(eng.ctx, 1, f, 512, 0, mem) == E.EINVAL
        assert L.jfsx_file_checksum_batch(eng.ctx, 1, f, 512, 1000, mem) == E.EINVAL
        assert L.jfsx_file_checksum_batch(eng.ctx, 0, f, 512, BLOCK, mem) == 0
        assert L.jfsx_file_checksum_batch(eng.ctx, 0, None, 512, BLOCK, mem) == 0
    g = (E.jfsx_fsum * 1)()
    g[0].data, g[0].len = None, 5
    for mem in (E.MEM_DEVICE, E.MEM_HOST):
        assert L.jfsx_file_checksum_batch(eng.ctx, 1, g, 512, BLOCK, mem) == E.EINVAL
    assert L.jfsx_file_checksum_batch(eng.ctx, 1, f, 512, BLOCK, 7) == E.EINVAL
    assert L.jfsx_file_checksum_batch(None, 1, f, 512, BLOCK, E.MEM_HOST) == E.EINVAL


def test_counts_under_the_crc_metrics(eng):
    data = np.arange(3000, dtype=np.uint32).view(np.uint8)
    before = eng.metrics()
    eng.file_checksum_batch([(data, data.size), (data, 100)], 4096, mem=E.MEM_HOST)
    after = eng.metrics()
    assert after["crc_batches"] == before["crc_batches"] + 1
    assert after["crc_ranges"] == before["crc_ranges"] + 2
    assert after["crc_bytes"] == before["crc_bytes"] + data.size + 100
    assert ctypes.sizeof(E.jfsx_metrics) == 28 * 8
