"""Hadoop file checksum (MD5-of-MD5-of-CRC32C), the host side of the C-ABI: the
span rule and the block/file MD5 fold over chunk CRCs from the CPU oracle,
against the five values the reference's Java SDK test holds
(tests/golden/java_filechecksum.json) and a pure-Python model.  No GPU."""
import random

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc
from tests import filechecksum_model as M

SIZES = (0, 1, 5, 6, 511, 512, 513, 600, 1024, 1025)


def test_span_matches_the_read_loop():
    for fs in SIZES:
        for length in SIZES:
            assert E.file_checksum_span(fs, length) == M.span(fs, length), (fs, length)
    # Long.MAX_VALUE, the one-argument getFileChecksum
    for fs in SIZES:
        assert E.file_checksum_span(fs, (1 << 63) - 1) == fs


def _case_chunk_crcs(case):
    """chunk CRC bytes of a golden case's span from the oracle's CRC32C"""
    span = M.case_span(case)
    c = case["content"]
    if "literal" in c:
        return M.chunk_crcs(c["literal"].encode("latin-1")[:span], orc.crc32c), span
    full, tail = divmod(span, 512)
    crcs = np.repeat(np.array([orc.crc32c(np.zeros(512, np.uint8))], ">u4"), full).tobytes()
    if tail:
        crcs += int(orc.crc32c(np.zeros(tail, np.uint8))).to_bytes(4, "big")
    return crcs, span


@pytest.mark.parametrize("case", M.golden_cases(), ids=lambda c: c["name"])
def test_fold_reproduces_the_java_values(case):
    crcs, span = _case_chunk_crcs(case)
    c32c, bpc, cpb, md5 = E.file_checksum_fold(crcs, span, case["block"])
    assert ("CRC32C" if c32c else "CRC32", bpc, cpb, md5.hex()) == M.case_expect(case)


@pytest.mark.parametrize("block", (512, 1536, 4096))
def test_fold_matches_model_on_random_data(block):
    # 0..9 blocks: DataOutputBuffer's padded lengths 32, 64 and 128
    rnd = random.Random(block)
    for nblocks in (0, 1, 2, 3, 4, 5, 8, 9):
        for tail in (0, -1, -511):  # whole blocks; a short last chunk; a one-chunk last block
            n = max(nblocks * block + (tail if nblocks else 0), 0)
            data = rnd.randbytes(n)
            crcs = M.chunk_crcs(data, orc.crc32c)
            c32c, bpc, cpb, md5 = E.file_checksum_fold(crcs, n, block)
            assert ("CRC32C" if c32c else "CRC32", bpc, cpb, md5.hex()) == M.fold(crcs, n, block), (nblocks, tail)


def test_model_padding_rule():
    assert [M.padded(k) for k in (0, 1, 2, 3, 4, 5, 8, 9)] == [32, 32, 32, 64, 64, 128, 128, 256]


def test_fold_argument_errors():
    L = E.load_library()
    f = E.jfsx_fsum()
    crc = bytes(4)
    assert L.jfsx_file_checksum_fold(crc, 1, 6, 256, 128 << 20, f) == E.EINVAL
    assert L.jfsx_file_checksum_fold(crc, 1, 6, 512, 0, f) == E.EINVAL
    assert L.jfsx_file_checksum_fold(crc, 1, 6, 512, 1000, f) == E.EINVAL
    assert L.jfsx_file_checksum_fold(crc, 1, 513, 512, 512, f) == E.EINVAL  # 513 bytes are two chunks
    assert L.jfsx_file_checksum_fold(None, 1, 6, 512, 512, f) == E.EINVAL
    assert L.jfsx_file_checksum_fold(crc, 1, 6, 512, 512, None) == E.EINVAL


def test_struct_layout_matches_header():
    import ctypes
    assert ctypes.sizeof(E.jfsx_fsum) == 48
    assert E.jfsx_fsum.md5.offset == 16 and E.jfsx_fsum.crc_per_block.offset == 40
