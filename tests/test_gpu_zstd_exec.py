"""The Zstandard decoders' match execution on the GPU, on the frames of
tests/zstd_frames.py: frames built sequence by sequence so that each reaches a
chosen step size, copy loop, dependency-mask edge, ring state or repeat-offset
form of decompress_par (juicefs_amd/csrc/jfsx_zstd2.h).  tests/test_zstd_frames.py
has checked every frame against the system zstd library and the host build of
the serial decoder, and that the corpus reaches every cell; here the bytes
must equal the model's exactly, without the serial decoder's help."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import zstd_frames as Z

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def device_batch(eng, items):
    """items: (frame, dst_cap, dst mod 16).  One jfsx_zstd_decompress_batch in
    device memory, every dst between GUARD bytes of FILL.  Returns per item
    (status, out_len, reserved, the dst_cap bytes, guards intact)."""
    ins, outs, io, oo = [], [], 0, 0
    for i, (fr, cap, a) in enumerate(items):
        ins.append(io + i % 4)
        io += len(fr) + 8
        outs.append(oo + GUARD + a)
        oo = (oo + GUARD + a + cap + GUARD + 15) & ~15
    inb, outb = eng.alloc(io + 16), eng.alloc(oo + 16)
    try:
        hin = np.zeros(io + 16, np.uint8)
        for (fr, _, _), p in zip(items, ins):
            hin[p:p + len(fr)] = np.frombuffer(fr, np.uint8)
        inb.upload(hin)
        outb.upload(np.full(oo + 16, FILL, np.uint8))
        arr, n = eng.make_zblocks((inb.ptr + p, len(fr), outb.ptr + q, cap) for (fr, cap, _), p, q in
                                  zip(items, ins, outs))
        assert all((outb.ptr + q) % 16 == a for (_, _, a), q in zip(items, outs))
        eng.zstd_decompress_batch(arr, n, E.MEM_DEVICE)
        h = outb.download(oo + 16)
    finally:
        inb.free()
        outb.free()
    res = []
    for i, ((_, cap, _), q) in enumerate(zip(items, outs)):
        intact = bool((h[q - GUARD:q] == FILL).all() and (h[q + cap:q + cap + GUARD] == FILL).all())
        res.append((arr[i].status, arr[i].out_len, arr[i].reserved, h[q:q + cap].tobytes(), intact))
    return res


def test_corpus_in_device_memory(eng):
    """One batch: every corpus frame at an aligned dst of exactly its size,
    and the ring-wrapping frame again at every other dst mod 16.  Only the
    65-block frame may reach the serial decoder."""
    cs = Z.corpus()
    wrap = next(c for c in cs if c.name == Z.ALIGN_CASE)
    what = [(c, 0) for c in cs] + [(wrap, a) for a in range(1, 16)]
    eng.metrics(reset=True)
    got = device_batch(eng, [(c.frame, len(c.out), a) for c, a in what])
    serial = eng.metrics()["zstd_serial"]
    for (c, a), (st, n, why, data, intact) in zip(what, got):
        assert st == E.OK and n == len(c.out), (c.name, a, st, n)
        assert data == c.out, (c.name, a, next(i for i in range(n) if data[i] != c.out[i]))
        assert intact, (c.name, a)
        assert (why != 0) == c.serial, (c.name, a, why)
    assert serial == 1


def test_corpus_in_host_memory(eng):
    cs = Z.corpus()
    eng.metrics(reset=True)
    got = eng.zstd_decompress([c.frame for c in cs], [len(c.out) for c in cs])
    for c, (st, d), why in zip(cs, got, eng.zstd_serial_reasons):
        assert st == E.OK and d == c.out, c.name
        assert (why != 0) == c.serial, (c.name, why)
    assert eng.metrics()["zstd_serial"] == 1


def test_rejects_in_device_memory(eng):
    """Each reject fails with the library's error class, and neither a guard
    nor a byte past dst_cap is written."""
    rj = Z.rejects()
    got = device_batch(eng, [(fr, cap, i % 16) for i, (_, fr, cap) in enumerate(rj)])
    for (name, _, _), (st, n, why, data, intact) in zip(rj, got):
        assert st in (E.EFORMAT, E.EDSTSIZE), (name, st)
        assert intact, name


def test_corpus_on_the_serial_decoder_in_a_fresh_process():
    """JFSX_ZSTD_SERIAL is read once per process: one child started with it
    set decodes the corpus and the rejects on the serial kernel
    (tests/zstd_serial_child.py); this test compares with the model.  With the
    serial kernel chosen for the batch no frame is a hand-off, the 65-block
    one included, which a process on the block-parallel kernel cannot show."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "zstd_serial_child.py")],
                       env=dict(os.environ, JFSX_ZSTD_SERIAL="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["serial_env"] == "1"
    cs, rj = Z.corpus(), Z.rejects()
    assert len(res["corpus"]) == len(cs) and len(res["rejects"]) == len(rj)
    for c, (st, digest, why) in zip(cs, res["corpus"]):
        assert st == E.OK and digest == hashlib.sha256(c.out).hexdigest(), c.name
        assert why == 0, c.name
    assert res["zstd_serial"] == 0
    for (name, _, _), (st, _) in zip(rj, res["rejects"]):
        assert st in (E.EFORMAT, E.EDSTSIZE), name
