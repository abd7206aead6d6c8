"""Pure-Python statement of Hadoop's MD5-of-MD5-of-CRC32C file checksum as the
reference computes it (getFileChecksum, sdk/java/src/main/java/io/juicefs/
JuiceFileSystemImpl.java:1286-1343), for the file-checksum tests.  hashlib's
MD5 and a caller-supplied CRC32C: nothing of the engine."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "java_filechecksum.json")


def span(file_size, length, bpc=512):
    """Bytes the read loop covers: bpc at a time while got < length (a read of
    `length` bytes when length < bpc), stopping at EOF."""
    if length < bpc:
        return min(file_size, length)
    return min(file_size, -(-length // bpc) * bpc)


def chunk_crcs(data, crc32c, bpc=512):
    """Big-endian CRC32C of every bpc-byte chunk (the last may be short)."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    return b"".join(int(crc32c(d[o:o + bpc])).to_bytes(4, "big") for o in range(0, d.size, bpc))


def padded(k):
    """DataOutputBuffer's backing array after k 16-byte appends: 32 bytes,
    grown to max(2 * cap, needed)."""
    cap = 32
    for i in range(1, k + 1):
        if 16 * i > cap:
            cap = max(2 * cap, 16 * i)
    return cap


def fold(crcs, span_len, block, bpc=512):
    """(type, bytesPerCRC, crcPerBlock, md5hex) from the chunk CRC bytes."""
    per = block // bpc
    nch = len(crcs) // 4
    digs = [hashlib.md5(crcs[4 * b:4 * min(b + per, nch)]).digest() for b in range(0, nch, per)]
    if not digs:
        return ("CRC32", 0, 0, hashlib.md5(bytes(32)).hexdigest())
    buf = b"".join(digs)
    buf += bytes(padded(len(digs)) - len(buf))
    return ("CRC32C", bpc, per if span_len > block else 0, hashlib.md5(buf).hexdigest())


def file_checksum(data, crc32c, block, bpc=512):
    return fold(chunk_crcs(data, crc32c, bpc), len(data), block, bpc)


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def case_size(case):
    c = case["content"]
    return c["zeros"] if "zeros" in c else len(c["literal"].encode("latin-1"))


def case_span(case):
    n = case_size(case)
    return span(n, n if case["length"] is None else case["length"])


def case_expect(case):
    e = case["expect"]
    return (e["type"], e["bytesPerCRC"], e["crcPerBlock"], e["md5"])
