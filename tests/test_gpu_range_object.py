"""The ranged read above the batch call: jfsx_data_decrypt_range against
oracle.data_decrypt sliced, Encrypted.Get on both sides of the reference's
4 * limit <= len rule, and the aggregator's ranged op from 20 threads."""
import ctypes
import threading

import numpy as np
import pytest

from juicefs_amd import engine as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ALGOS = [E.AES256GCM, E.CHACHA20P1305]
ORC = {E.AES256GCM: orc.AES256GCM, E.CHACHA20P1305: orc.CHACHA20P1305}
CT = E.CRC_GEN | E.CRC_CT


def window(length, off, limit):
    """encrypt.go:246-253"""
    o = min(off, length)
    n = length - o if limit == -1 or limit > length - o else limit
    return o, n


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("algo", ALGOS)
def test_data_decrypt_range(eng, algo):
    wrapped = bytes(range(256))
    for i, n in enumerate([0, 5, 32768, 100003]):
        key, nonce = orc.gen_key(31, i)
        obj = orc.data_encrypt(ORC[algo], key, nonce, wrapped, orc.gen_block(31, i, n)[:n])
        plain = orc.data_decrypt(ORC[algo], key, obj)
        crc = int(orc.object_checksum(obj))
        for off, limit in [(0, -1), (0, 0), (1, 3), (n // 2, n // 5), (n - 1 if n else 0, 9), (n, 1), (n + 5, -1),
                           (32767, 2)]:
            o, w = window(n, off, limit)
            rc, got = eng.data_decrypt_range(algo, key, obj, off, limit)
            assert rc == 0 and got == plain[o:o + w], (n, off, limit)
            rc, got = eng.data_decrypt_range(algo, key, obj, off, limit, expect_crc=crc)
            assert rc == 0 and got == plain[o:o + w] and eng.last_got_crc == crc, (n, off, limit)
            rc, got = eng.data_decrypt_range(algo, key, obj, off, limit, expect_crc=crc ^ 1)
            assert rc == E.ECRC and got == b"" and eng.last_got_crc == crc
        # a bad tag alone, and with a checksum mismatch, where the checksum wins
        bad = bytearray(obj)
        bad[-1] ^= 1
        bad = bytes(bad)
        rc, got = eng.data_decrypt_range(algo, key, bad, 0, 3)
        assert rc == E.ETAG and got == b""
        rc, got = eng.data_decrypt_range(algo, key, bad, 0, 3, expect_crc=int(orc.object_checksum(bad)))
        assert rc == E.ETAG
        rc, got = eng.data_decrypt_range(algo, key, bad, 0, 3, expect_crc=crc)
        assert rc == E.ECRC and str(eng.last_got_crc) == orc.object_checksum(bad)
        rc, _ = eng.data_decrypt_range(algo, key, obj[:200], 0, 3)
        assert rc == E.EMISFORMED


@pytest.mark.parametrize("algo", ALGOS)
def test_data_decrypt_range_releases_nothing_on_failure(eng, algo):
    key, nonce = orc.gen_key(32, 0)
    n = 70001
    obj = np.frombuffer(orc.data_encrypt(ORC[algo], key, nonce, bytes(range(256)), orc.gen_block(32, 0, n)[:n]),
                        np.uint8).copy()
    plain = orc.data_decrypt(ORC[algo], key, obj)
    out = np.full(64, 0xC3, np.uint8)
    olen = ctypes.c_uint64(99)
    dr = eng.L.jfsx_data_decrypt_range
    # out_cap one byte short of n: rejected, nothing written
    assert dr(eng.ctx, algo, key, obj.ctypes.data, obj.size, 40000, 33, out.ctypes.data, 32, ctypes.byref(olen),
              None, None) == E.EINVAL
    assert olen.value == 99 and (out == 0xC3).all()
    assert dr(eng.ctx, algo, key, obj.ctypes.data, obj.size, 40000, 33, out.ctypes.data, 33, ctypes.byref(olen),
              None, None) == 0
    assert olen.value == 33 and out[:33].tobytes() == plain[40000:40033] and (out[33:] == 0xC3).all()
    # a bit flipped far outside the window: no plaintext, *out_len untouched
    obj[-5000] ^= 4
    out[:] = 0xC3
    olen.value = 99
    assert dr(eng.ctx, algo, key, obj.ctypes.data, obj.size, 100, 33, out.ctypes.data, 64, ctypes.byref(olen),
              None, None) == E.ETAG
    assert olen.value == 99 and not out[:33].any() and (out[33:] == 0xC3).all()


@pytest.mark.parametrize("with_checksum", [False, True], ids=["plain", "checksum"])
@pytest.mark.parametrize("algo", ["aes256gcm-rsa", "chacha20-rsa"])
def test_encrypted_get(eng, algo, with_checksum):
    from juicefs_amd import checksum as cs
    from juicefs_amd import encrypt as enc
    de = enc.NewDataEncryptor(enc.NewRSAEncryptor(enc.GenerateRsaKey(2048)), algo, eng)
    store = cs.ChecksumStorage(enc.MemStorage(), eng=eng) if with_checksum else enc.MemStorage()
    es = enc.NewEncrypted(store, de)
    n = 200001
    data = orc.gen_block(33, 0, n).tobytes()
    es.Put("k", data)
    inner = store.inner if with_checksum else store

    def calls():
        return getattr(de, "range_calls", 0), eng.metrics()["open_batches"]

    quarter = n // 4
    # at or below a quarter of the object: the ranged call
    for off, limit in [(0, 0), (10, 20), (32760, 100), (n - 7, 50), (n, 5), (n + 9, 1), (5, quarter)]:
        r0, m0 = calls()
        assert es.Get("k", off, limit) == data[off:off + limit], (off, limit)
        r1, m1 = calls()
        assert (r1 - r0, m1 - m0) == (1, 1), (off, limit)
    # above it, or to the end: the whole-object call
    for off, limit in [(5, quarter + 1), (0, -1), (7, -1), (100, n)]:
        r0, m0 = calls()
        want = data[off:] if limit == -1 else data[off:off + limit]
        assert es.Get("k", off, limit) == want, (off, limit)
        r1, m1 = calls()
        assert (r1 - r0, m1 - m0) == (0, 1), (off, limit)
    # the same errors on both sides of the rule: a stored object with a flipped bit
    raw = bytearray(inner.Get("k"))
    raw[-3000] ^= 0x20
    inner.Put("k", bytes(raw))
    err = cs.ChecksumVerifyError if with_checksum else enc.EncryptError
    seen = []
    for off, limit in [(10, 20), (10, -1)]:
        with pytest.raises(err) as ei:
            es.Get("k", off, limit)
        seen.append((type(ei.value), str(ei.value)))
    assert seen[0] == seen[1]
    assert with_checksum or "message authentication failed" in seen[0][1]


@pytest.mark.parametrize("algo", ALGOS)
def test_aggregator_open_range_from_20_threads(eng, algo):
    n = 300007
    blocks = []
    for i in range(20):
        key, nonce = orc.gen_key(34, i)
        c, tag = orc.seal(ORC[algo], key, nonce, orc.gen_block(34, i, n)[:n], fast=True)
        if i % 5 == 4:
            c = c[:n - 9] + bytes([c[n - 9] ^ 1]) + c[n - 8:]  # tampered far outside the window
        blocks.append((key, nonce, np.frombuffer(c, np.uint8).copy(), tag, 1000 * i + 3, 5000 + i))

    def records(crcs):
        dsts = [np.full(b[5] + 16, 0xC3, np.uint8) for b in blocks]
        arr, cnt = E.Engine.make_rblocks([{"key": b[0], "nonce": b[1], "tag": b[3], "src": b[2].ctypes.data, "len": n,
                                           "off": b[4], "limit": b[5], "dst": dsts[i].ctypes.data, "dst_cap": b[5],
                                           "crc": crcs[i].ctypes.data} for i, b in enumerate(blocks)])
        return arr, cnt, dsts

    nw = 4 * -(-n // E.SEG)
    ref_crc = [np.zeros(nw, np.uint8) for _ in blocks]
    ref, cnt, ref_dst = records(ref_crc)
    eng.open_range_batch(algo, ref, cnt, CT, E.MEM_HOST)
    assert [ref[i].status for i in range(20)] == [E.ETAG if i % 5 == 4 else E.OK for i in range(20)]
    got_crc = [np.zeros(nw, np.uint8) for _ in blocks]
    got, _, got_dst = records(got_crc)
    agg = E.Aggregator(eng, window_us=20000)
    try:
        errs = []
        gate = threading.Barrier(20)

        def one(i):
            try:
                gate.wait()
                agg.open_range(algo, got[i], CT, E.MEM_HOST)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=one, args=(i,)) for i in range(20)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        calls, batches, carried = agg.stats()
    finally:
        agg.close()
    assert calls == 20 and carried == 20 and batches < calls
    for i in range(20):
        assert (got[i].status, got[i].out_len) == (ref[i].status, ref[i].out_len), i
        assert got_dst[i].tobytes() == ref_dst[i].tobytes() and (got_dst[i][blocks[i][5]:] == 0xC3).all(), i
        assert got_crc[i].tobytes() == ref_crc[i].tobytes() == orc.checksum(blocks[i][2], hw=True), i
