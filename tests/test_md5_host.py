"""CPU pin of the MD5 the file checksum uses (juicefs_amd/csrc/jfsx_md5.h),
the host build of the code md5_blocks_k runs per DFS block: the RFC 1321 test
suite, and every padding branch and every chunk-CRC group length against
hashlib."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "md5_host.cpp")

# RFC 1321 A.5
RFC_SUITE = [
    (b"", "d41d8cd98f00b204e9800998ecf8427e"),
    (b"a", "0cc175b9c0f1b6a831c399e269772661"),
    (b"abc", "900150983cd24fb0d6963f7d28e17f72"),
    (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
    (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
    (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
    (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a"),
]


def _data():
    return random.Random(1321).randbytes(256)


@pytest.fixture(scope="module")
def md5(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("md5") / "md5_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.md5_digest.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.md5_stream.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
    L.md5_words.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    return L


def _call(fn, *args):
    out = ctypes.create_string_buffer(16)
    fn(*args, out)
    return out.raw.hex()


def test_rfc1321_suite(md5):
    for msg, want in RFC_SUITE:
        assert _call(md5.md5_digest, msg, len(msg)) == want
        assert _call(md5.md5_stream, msg, len(msg), 3) == want


def test_lengths_0_to_130_match_hashlib(md5):
    d = _data()
    for n in range(131):
        want = hashlib.md5(d[:n]).hexdigest()
        assert _call(md5.md5_digest, d[:n], n) == want, n
        for step in (1, 7, 64, 65):
            assert _call(md5.md5_stream, d[:n], n, step) == want, (n, step)


def test_word_path_group_lengths_match_hashlib(md5):
    # the kernel's message is 4 * (chunks of the block) bytes: 4 x {1..40}
    # covers a remainder of 0..15 words, with and without the extra block
    d = _data()
    for w in range(1, 41):
        assert _call(md5.md5_words, d[:4 * w], w) == hashlib.md5(d[:4 * w]).hexdigest(), w


def test_sanitized_program_length_sweep(tmp_path):
    exe = str(tmp_path / "md5_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DMD5_HOST_MAIN", "-o", exe, SRC])
    d = _data()
    f = tmp_path / "data.bin"
    f.write_bytes(d)
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 2 * 131 + 40
    for ln in lines:
        tag, n, hexd = ln.split()
        assert tag in ("d", "s", "w")
        assert hexd == hashlib.md5(d[:int(n)]).hexdigest(), ln
